"""Pattern databases on the MI355X, measured once -> profiles/pdb_probe.txt.

    python tools/pdb_probe.py [--states 500] [--cap 16777216] [--budget_s 150] [--puzzle24 | --only_puzzle24 | --reflect_eval]

Legs: (1) build time and sweep count of every preset (puzzle24 6-6-6-6 — four tables of 6.1 GB — only with --puzzle24);
(2) dca_pdb_eval rows/s at 131 072 rows; (3) on the shipped puzzle15 test states (tests/golden/golden.npz, with their optimal
lengths): BWAS at weight 1, cpp semantics, batch 10 000 under a node cap (`--cap` ids per search) with pdb:5-5-5, pdb:6-6-3
and builtin:manhattan — how many states each solves at the optimal length inside the cap, and the nodes generated per state.
Each heuristic gets `--budget_s` seconds of wall time and walks the states in file order; the comparison is made on the prefix
every heuristic reached.  `--reflect_eval` runs one leg alone: rows/s of the plain and of the reflected eval (`+reflect`) on
1 048 576 rows of puzzle15 (5-5-5, 6-6-3) and puzzle24 (6-6-6-6), the two timed alternately after a warm-up, with the spread."""
import argparse
import os
import sys
import time

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

from deepcubea_amd import _lib  # noqa: E402
from deepcubea_amd.search_methods.engine import BwasEngine  # noqa: E402
from deepcubea_amd.utils.pattern_db import PRESETS, PatternDatabase  # noqa: E402


def build_leg(env, name):
    torch.cuda.synchronize()
    t0 = time.time()
    pdb = PatternDatabase(env, name).build()
    torch.cuda.synchronize()
    dt = time.time() - t0
    print("build  %-9s %-8s %14d bytes  %8.3f s  sweeps %s" % (env, name, pdb.bytes, dt, pdb.sweeps), flush=True)
    return pdb


def eval_leg(env, name, pdb, rows=131072, reps=20):
    D = pdb.dim * pdb.dim
    rng = np.random.default_rng(0)
    X = torch.from_numpy(rng.permuted(np.tile(np.arange(D, dtype=np.uint8), (rows, 1)), axis=1)).cuda()
    out = torch.empty(rows, dtype=torch.float32, device="cuda")
    for _ in range(3):
        _lib.pdb_eval(pdb.dim, X, pdb.partition, pdb.tables, out=out)
    times = []
    for _ in range(reps):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record()
        _lib.pdb_eval(pdb.dim, X, pdb.partition, pdb.tables, out=out)
        b.record()
        b.synchronize()
        times.append(a.elapsed_time(b) * 1e-3)
    med = float(np.median(times))
    print("eval   %-9s %-8s %d rows (uniform random permutations)  median %.1f us  min %.1f us  %.3g rows/s (median of %d)"
          % (env, name, rows, med * 1e6, min(times) * 1e6, rows / med, reps), flush=True)


def reflect_eval_leg(env, name, pdb, rows=1 << 20, reps=20):
    D = pdb.dim * pdb.dim
    rng = np.random.default_rng(0)
    X = torch.from_numpy(rng.permuted(np.tile(np.arange(D, dtype=np.uint8), (rows, 1)), axis=1)).cuda()
    out = torch.empty(rows, dtype=torch.float32, device="cuda")
    times = {False: [], True: []}
    for rep in range(3 + reps):  # three warm-up rounds, then plain and reflected alternately
        for reflect in (False, True):
            a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            a.record()
            _lib.pdb_eval(pdb.dim, X, pdb.partition, pdb.tables, out=out, reflect=reflect)
            b.record()
            b.synchronize()
            if rep >= 3:
                times[reflect].append(a.elapsed_time(b) * 1e-3)
    med = {r: float(np.median(t)) for r, t in times.items()}
    for reflect in (False, True):
        t = times[reflect]
        print("eval   %-9s %-16s %d rows (uniform random permutations)  median %.1f us  min %.1f us  max %.1f us  %.3g rows/s (median of %d)"
              % (env, name + ("+reflect" if reflect else ""), rows, med[reflect] * 1e6, min(t) * 1e6, max(t) * 1e6, rows / med[reflect], reps), flush=True)
    print("eval   %-9s %-16s reflected / plain time: %.2f" % (env, name, med[True] / med[False]), flush=True)


def search_leg(label, states, opt, cap, budget_s, pdb=None):
    eng = BwasEngine("puzzle15", 1.0, 10000, max_nodes=cap, semantics=_lib.SEM_CPP, packed=pdb is not None)
    fn = pdb.heuristic_fn_dev() if pdb is not None else None
    rows = []
    t0 = time.time()
    for i, root in enumerate(states):
        if time.time() - t0 > budget_s:
            break
        if fn is not None:
            res = eng.solve(root, fn, max_iters=100000)
        else:
            res = eng.solve_builtin(root, _lib.HEUR_MANHATTAN, max_iters=100000, chunk=64, use_graph=True)
        optimal = bool(res["solved"]) and len(res["moves"]) == int(opt[i])
        assert not res["solved"] or len(res["moves"]) >= int(opt[i]), (label, i)
        rows.append((bool(res["solved"]), optimal, int(res["nodes_generated"])))
    eng.close()
    print("search %-18s reached %d states in %.1f s" % (label, len(rows), time.time() - t0), flush=True)
    return rows


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--states", type=int, default=500)
    ap.add_argument("--cap", type=int, default=1 << 24)
    ap.add_argument("--budget_s", type=float, default=150.0)
    ap.add_argument("--puzzle24", action="store_true")
    ap.add_argument("--only_puzzle24", action="store_true", help="the puzzle24 6-6-6-6 build and eval legs alone")
    ap.add_argument("--reflect_eval", action="store_true", help="the plain against the reflected eval on 2^20 rows, alone")
    args = ap.parse_args()
    _lib.require_gpu()
    print("pdb_probe: %s, states %d, node cap %d per search, %.0f s per heuristic" % (torch.cuda.get_device_name(0), args.states, args.cap,
                                                                                     args.budget_s), flush=True)
    if args.reflect_eval:
        for env, name in (("puzzle15", "5-5-5"), ("puzzle15", "6-6-3"), ("puzzle24", "6-6-6-6")):
            pdb = build_leg(env, name)
            reflect_eval_leg(env, name, pdb)
            del pdb
            torch.cuda.empty_cache()
        return
    built = {}
    for env in ("puzzle8", "puzzle15"):
        for name in sorted(PRESETS[env]) if not args.only_puzzle24 else ():
            built[(env, name)] = build_leg(env, name)
            eval_leg(env, name, built[(env, name)])
    if args.puzzle24 or args.only_puzzle24:
        pdb = build_leg("puzzle24", "6-6-6-6")
        eval_leg("puzzle24", "6-6-6-6", pdb)
        del pdb
        torch.cuda.empty_cache()
    else:
        print("build  puzzle24  6-6-6-6  NOT RUN (four tables of 25^7 = 6.1 GB; pass --puzzle24)", flush=True)
    if args.only_puzzle24:
        return
    g = np.load(os.path.join(ROOT, "tests", "golden", "golden.npz"))
    states, opt = g["puzzle15_test_states"][:args.states], g["puzzle15_test_opt_len"][:args.states]
    legs = {"pdb:5-5-5": search_leg("pdb:5-5-5", states, opt, args.cap, args.budget_s, built[("puzzle15", "5-5-5")]),
            "pdb:6-6-3": search_leg("pdb:6-6-3", states, opt, args.cap, args.budget_s, built[("puzzle15", "6-6-3")]),
            "builtin:manhattan": search_leg("builtin:manhattan", states, opt, args.cap, args.budget_s)}
    common = min(len(r) for r in legs.values())
    print("puzzle15, first %d shipped test states (the prefix every heuristic reached), weight 1, cpp semantics, batch 10000, cap %d ids:"
          % (common, args.cap))
    both = [i for i in range(common) if all(r[i][1] for r in legs.values())]
    for label, r in legs.items():
        r = r[:common]
        nodes = np.array([x[2] for x in r], np.float64)
        print("  %-18s solved at the optimal length %d / %d (solved at all: %d); nodes generated per state: median %.3g, mean %.3g, max %.3g"
              % (label, sum(x[1] for x in r), common, sum(x[0] for x in r), np.median(nodes), nodes.mean(), nodes.max()))
    if both:
        print("  on the %d states every heuristic solved optimally, nodes generated per state (mean / median):" % len(both))
        for label, r in legs.items():
            nodes = np.array([r[i][2] for i in both], np.float64)
            print("    %-18s %.4g / %.4g" % (label, nodes.mean(), np.median(nodes)))


if __name__ == "__main__":
    main()
