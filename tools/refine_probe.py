#!/usr/bin/env python3
"""What refining does, measured (a report, not a test; its output is kept as profiles/refine_probe.txt).

    python tools/refine_probe.py [--out profiles/refine_probe.txt] [--legs synthetic,bwas] [--paths 200] [--optimal_seconds 400]

One GPU visit, one process, times by the host clock around calls that end synchronised.  No counters are collected: what bounds
ida_cube3_batch_kernel is not measured here.  Legs:
  synthetic  --paths random-walk solutions of 30 moves (the inverse of a seeded uniform scramble), refined with pdb:korf7 at
             windows 10, 12, 14 and 16: mean length in and out, seconds per path, and — for the paths whose plain IDA* search
             (IDAStar.solve, 5 s of nodes at the measured rate) finishes, tried in order for --optimal_seconds — the share whose
             refined length is that optimal length.  Then the same windows one by one through the single search
             (IDAStar.solve on every window's root, no bound) on the first paths: single, batched, single again, and the ratio.
  bwas       the first 100 shipped cube3 states (tests/golden/golden.npz) solved by the BWAS engine and then refined.  The
             heuristic: a network checkpoint under saved_models/cube3/current if there is one, else pdb:korf at --weight 0.6 — a
             weight below 1 makes the engine greedy, so its solutions are not optimal; the engine runs a bounded number of
             iterations per group and a state it has not solved by then is left out, and counted.  Optimal count and mean
             length before and after, seconds added."""
import argparse
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

WINDOWS = (10, 12, 14, 16)
SINGLE_PATHS = 20  # paths of the single-against-batched comparison
SINGLE_WINDOWS = (12, 14)


class Tee:
    def __init__(self, path):
        self.file = open(path, "w") if path else None

    def __call__(self, text=""):
        print(text, flush=True)
        if self.file:
            self.file.write(text + "\n")
            self.file.flush()


class OneByOne:
    """solve_bounded through the single search: every root a call of IDAStar.solve, which knows no bound and runs on to the
    root's optimal solution; a solution above the bound counts as "bounded"."""

    def __init__(self, search):
        self.search = search

    def solve_bounded(self, roots, max_length, max_nodes=None):
        out = []
        for root, bound in zip(roots, max_length):
            res = dict(self.search.solve(root, max_nodes))
            if res["solved"] and len(res["moves"]) > bound:
                res.update(solved=False, status="bounded", moves=[])
            out.append(res)
        return out


def random_solutions(count, length=30):
    """(roots, solutions): the states that seeded uniform scrambles of `length` moves reach and the inverse scrambles."""
    from deepcubea_amd import _lib
    from deepcubea_amd.search_methods import refine
    perm = _lib.cube3_perm_table()
    solutions = [[int(a) ^ 1 for a in reversed(np.random.default_rng(1000 + i).integers(0, 12, size=length))] for i in range(count)]
    return [refine.window_root(perm, s) for s in solutions], solutions


def refine_all(search, solutions, window, max_nodes=None):
    from deepcubea_amd.search_methods import refine
    start = time.time()
    done = [refine.refine_moves(search, s, window, max_nodes) for s in solutions]
    return [m for m, _ in done], [s for _, s in done], time.time() - start


def synthetic_leg(say, count, optimal_seconds):
    from deepcubea_amd.search_methods import idastar
    from deepcubea_amd.utils.cube3_pdb import Cube3PatternDatabase
    start = time.time()
    pdb = Cube3PatternDatabase("korf7").build()
    search = idastar.IDAStar("cube3", pdb)
    say("cube3 pdb:korf7: %d bytes built in %.2f s" % (pdb.bytes, time.time() - start))
    roots, solutions = random_solutions(count)
    refine_all(search, solutions[:2], 10)  # warm-up: the first launches
    lengths = {}
    for window in WINDOWS:
        moves, stats, seconds = refine_all(search, solutions, window)
        lengths[window] = [len(m) for m in moves]
        say("  window %2d: %d paths, mean length %.3f -> %.3f, %.4f s a path (%.2f s), passes %.2f, windows searched %.1f, nodes %.3g a path, "
            "unfinished windows %d" % (window, count, np.mean([len(s) for s in solutions]), np.mean(lengths[window]), seconds / count, seconds,
                                       np.mean([s["passes"] for s in stats]), np.mean([s["windows"] for s in stats]),
                                       np.mean([s["nodes"] for s in stats]), sum(s["unfinished"] for s in stats)))
    budget = int(5 * idastar.MEASURED_NODES_PER_SECOND["cube3"])
    optimal, tried, start = {}, 0, time.time()
    for i, root in enumerate(roots):
        if time.time() - start > optimal_seconds:
            break
        tried += 1
        res = search.solve(root, budget)
        if res["solved"]:
            optimal[i] = len(res["moves"])
        if tried % 20 == 0:
            say("    ... %d paths tried, %d finished, %.0f s" % (tried, len(optimal), time.time() - start))
    say("  plain IDA* (5 s of nodes: %d): tried the first %d paths in %.1f s, finished %d (optimal length %s .. %s)"
        % (budget, tried, time.time() - start, len(optimal), min(optimal.values(), default="-"), max(optimal.values(), default="-")))
    for window in WINDOWS:
        hit = sum(1 for i, k in optimal.items() if lengths[window][i] == k)
        say("  window %2d: refined length = the optimal length on %d of the %d paths whose plain search finished; mean excess %.3f"
            % (window, hit, len(optimal), np.mean([lengths[window][i] - k for i, k in optimal.items()]) if optimal else 0.0))
    few = solutions[:SINGLE_PATHS]
    for window in SINGLE_WINDOWS:
        first = refine_all(OneByOne(search), few, window)
        batched = refine_all(search, few, window)
        last = refine_all(OneByOne(search), few, window)
        assert [len(m) for m in first[0]] == [len(m) for m in batched[0]] == [len(m) for m in last[0]]
        say("  window %2d, first %d paths: one by one %.3f s, batched %.3f s, one by one again %.3f s: ratio %.2f (the single search "
            "also runs a window's last threshold)" % (window, len(few), first[2], batched[2], last[2], (first[2] + last[2]) / 2 / batched[2]))
    return search


def bwas_solutions(say, states, max_iters):
    """The engine's solutions of `states` -> (solutions or None per state, the model's name, seconds)."""
    import torch  # noqa: F401
    from deepcubea_amd import _lib
    from deepcubea_amd.search_methods import astar
    from deepcubea_amd.search_methods.engine import BwasEngine
    from deepcubea_amd.utils import env_utils
    checkpoint = os.path.join(ROOT, "saved_models", "cube3", "current")
    have = os.path.isdir(checkpoint)
    model = checkpoint if have else "pdb:korf"
    args = astar.build_parser().parse_args(["--states", "-", "--model_dir", model, "--env", "cube3", "--results_dir", "-", "--batch_size",
                                            "10000" if have else "1000", "--weight", "0.6"])
    env = env_utils.get_environment("cube3")
    heuristic_fn, onehot_stride = astar._load_heuristic(args, env)
    K = astar.auto_instances(args, env, len(states), None)
    eng = BwasEngine("cube3", args.weight, args.batch_size, max_nodes=astar._max_nodes(args, K), semantics=_lib.SEM_PY,
                     onehot_dtype=None if onehot_stride == 0 else torch.float32, num_instances=K, packed=onehot_stride is not None,
                     onehot_stride=onehot_stride or None)
    say("  engine: %s, --weight %s, --batch_size %d, %d instances a group, at most %d iterations a group" % (model, args.weight, args.batch_size, K, max_iters))
    out, start = [], time.time()
    for g0 in range(0, len(states), K):
        group = [np.ascontiguousarray(s, dtype=np.uint8) for s in states[g0:g0 + K]]
        results = eng.solve_many(group, heuristic_fn, max_iters=max_iters) if K > 1 else [eng.solve(group[0], heuristic_fn, max_iters=max_iters)]
        out += [[int(a) for a in r["moves"]] if r["solved"] else None for r in results]
    eng.close()
    return out, model, time.time() - start


def bwas_leg(say, search, max_iters):
    from deepcubea_amd.search_methods import idastar
    from deepcubea_amd.utils.cube3_pdb import Cube3PatternDatabase
    z = np.load(os.path.join(ROOT, "tests", "golden", "golden.npz"))
    states, optimal = z["cube3_test_states"][:100], [int(k) for k in z["cube3_test_opt_len"][:100]]
    found, model, seconds = bwas_solutions(say, states, max_iters)
    solved = [i for i, s in enumerate(found) if s is not None]
    say("  the engine solved %d of the first 100 shipped states in %.1f s" % (len(solved), seconds))
    if not solved:
        say("  no source of suboptimal engine solutions here: nothing to refine")
        return
    if search is None:
        search = idastar.IDAStar("cube3", Cube3PatternDatabase("korf7").build())
    before = [len(found[i]) for i in solved]
    say("  before: optimal %d of %d, mean length %.3f (mean optimal length %.3f)"
        % (sum(1 for i, n in zip(solved, before) if n == optimal[i]), len(solved), np.mean(before), np.mean([optimal[i] for i in solved])))
    for window in (12, 14):
        moves, stats, added = refine_all(search, [found[i] for i in solved], window)
        after = [len(m) for m in moves]
        say("  window %2d: optimal %d of %d, mean length %.3f, %.2f s added (%.4f s a state), unfinished windows %d"
            % (window, sum(1 for i, n in zip(solved, after) if n == optimal[i]), len(solved), np.mean(after), added, added / len(solved),
               sum(s["unfinished"] for s in stats)))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=None)
    ap.add_argument("--legs", default="synthetic,bwas")
    ap.add_argument("--paths", type=int, default=200)
    ap.add_argument("--optimal_seconds", type=float, default=400.0, help="wall seconds for the plain searches of the synthetic leg")
    ap.add_argument("--bwas_iters", type=int, default=3000, help="engine iterations a group of the bwas leg gets")
    args = ap.parse_args()
    say = Tee(args.out)
    legs = args.legs.split(",")
    say("refine probe: %s" % " ".join(sys.argv[1:]))
    search = None
    if "synthetic" in legs:
        say("---- leg synthetic")
        search = synthetic_leg(say, args.paths, args.optimal_seconds)
    if "bwas" in legs:
        say("---- leg bwas")
        try:
            bwas_leg(say, search, args.bwas_iters)
        except Exception as err:  # the report says what did not work; a device fault ends the process either way
            say("  the leg ended on %s: %s" % (type(err).__name__, err))


if __name__ == "__main__":
    main()
