"""Shorten found cube3 solutions by optimal re-solves of their windows (include/dca.h "Bounded batches").

    python -m deepcubea_amd.search_methods.refine --results results/cube3/results.pkl --env cube3 \
        --model_dir pdb:korf7+dual --window 14 --results_dir results/cube3_refined

A solution of 22..26 moves that astar.py found with the network is seldom optimal, and IDA* on the tables does not reach such a
state in a minute.  But every run of w consecutive moves of the solution is itself a solution — of the state w moves from the
goal that undoing it gives — and a root 12..16 moves deep is a small search.  refine_moves() searches every window of a
solution for a shorter replacement, all windows of a pass as one bounded batch (IDAStar.solve_bounded: one launch per round),
replaces what it finds and repeats until no window gives way.  No network is needed, only an admissible `pdb:` set.

The CLI reads an astar.py-format results.pkl, refines every non-empty solution and writes results.pkl with the same keys
(paths recomputed, `times` = the original seconds plus the refining seconds) and refine.pkl with, per state, `length_in`,
`length_out`, `passes`, `windows`, `nodes` and `unfinished`."""
from __future__ import annotations

import os
import sys
import time
from argparse import ArgumentParser
from typing import Any, Dict, List, Tuple

import numpy as np

from .. import _lib
from ..utils import data_utils
from . import idastar

MIN_WINDOW, MAX_WINDOW = 4, 20  # below 4 moves no window has a shorter form the pruning rules leave; above 20 no search is small
STATS = ("length_in", "length_out", "passes", "windows", "nodes", "unfinished")


def check_window(window: int) -> int:
    if not MIN_WINDOW <= window <= MAX_WINDOW:
        raise ValueError("--window must be in %d..%d, not %d" % (MIN_WINDOW, MAX_WINDOW, window))
    return window


def window_root(perm: np.ndarray, moves) -> np.ndarray:
    """The state that `moves` solves: the goal with the inverse moves (a ^ 1) applied in reverse order, by the perm table alone."""
    cur = np.arange(54, dtype=np.uint8)
    for a in reversed(moves):
        cur = cur[perm[int(a) ^ 1]]
    return cur


def refine_moves(search, moves, window: int, max_nodes: int = None) -> Tuple[List[int], Dict[str, int]]:
    """moves: a cube3 move list (action numbers); search: an IDAStar on cube3 (anything with its solve_bounded) on an admissible
    table set.  -> (moves', stats).

    A pass takes, for every i, the window moves[i : i + w], w = min(window, L - i) >= 4, and asks one solve_bounded call for a
    solution of each window's root of at most w - 2 moves: a quarter turn is an odd permutation of the corners, so in this
    12-move metric every solution of a state has the parity of any other, and a shorter one is shorter by at least 2.  Walking
    left to right, every window that came back solved is replaced, unless it overlaps one replaced in this pass.  Passes repeat
    until none is solved; the length falls by at least 2 per replacing pass.  A window already searched (shown optimal, or out of
    budget) is not searched again in a later pass.

    The guarantee on return: moves' takes every state to where moves takes it (a replacement solves the window's own root), so
    it is a valid solution wherever moves is; it is not longer than moves; and every window of at most `window` moves whose
    search finished is optimal.  A window whose search ran out of max_nodes (per window) is left as it is and counted:
    stats["unfinished"] is the number of such windows in moves'.  stats: length_in, length_out, passes, windows (searched),
    nodes (generated), unfinished."""
    check_window(window)
    perm = _lib.cube3_perm_table()
    moves = [int(a) for a in moves]
    stats = {k: 0 for k in STATS}
    stats["length_in"] = len(moves)
    optimal, gave_up = set(), set()  # windows shown to have no shorter solution; windows whose search ran out of budget
    while True:
        L = len(moves)
        spans = [(i, min(window, L - i)) for i in range(L) if min(window, L - i) >= MIN_WINDOW]
        stats["unfinished"] = sum(1 for i, w in spans if tuple(moves[i:i + w]) in gave_up)
        spans = [(i, w) for i, w in spans if tuple(moves[i:i + w]) not in optimal | gave_up]
        found: Dict[int, List[int]] = {}
        for at in range(0, len(spans), _lib.IDASTAR_MAX_BATCH):
            part = spans[at:at + _lib.IDASTAR_MAX_BATCH]
            roots = np.stack([window_root(perm, moves[i:i + w]) for i, w in part])
            results = search.solve_bounded(roots, [w - 2 for _, w in part], max_nodes)
            for (i, w), res in zip(part, results):
                stats["nodes"] += res["nodes_generated"]
                if res["solved"]:
                    found[i] = res["moves"]
                elif res["status"] == _lib.IDASTAR_STATUS[_lib.IDASTAR_BOUNDED]:
                    optimal.add(tuple(moves[i:i + w]))
                else:
                    gave_up.add(tuple(moves[i:i + w]))
                    stats["unfinished"] += 1
        stats["passes"] += 1
        stats["windows"] += len(spans)
        if not found:
            break
        out, done = [], 0  # done: the first move not yet copied or replaced
        for i, w in spans:
            if i in found and i >= done:
                out += moves[done:i] + found[i]
                done = i + w
        moves = out + moves[done:]
    stats["length_out"] = len(moves)
    return moves, stats


def build_parser() -> ArgumentParser:
    parser = ArgumentParser()
    parser.add_argument('--results', type=str, required=True, help="an astar.py-format results.pkl whose solutions are to be refined")
    parser.add_argument('--env', type=str, required=True, help="Environment: cube3 (a sliding puzzle's window has no root of its own: "
                                                               "the blank is part of the state)")
    parser.add_argument('--model_dir', type=str, required=True,
                        help="pdb:SPEC, as for idastar.py: the cube3 table set the windows are searched on (corners, korf, korf7, "
                             "with +sym, +sym:N, +dual).  Built on the GPU at start-up")
    parser.add_argument('--window', type=int, default=14,
                        help="the longest window re-solved, in moves (%d..%d).  On return every window of at most this many moves "
                             "whose search finished is optimal" % (MIN_WINDOW, MAX_WINDOW))
    parser.add_argument('--results_dir', type=str, required=True, help="Directory to save results.pkl and refine.pkl")
    parser.add_argument('--max_nodes', type=int, default=None,
                        help="node budget of one window's search; a window that runs out of it is left as it is and counted as "
                             "unfinished.  The default is idastar.py's for cube3: %d" % idastar.DEFAULT_MAX_NODES["cube3"])
    parser.add_argument('--start_idx', type=int, default=0, help="")
    parser.add_argument('--debug', action='store_true', default=False, help="do not copy the output to results_dir/output.txt")
    return parser


def refine_file(args, search) -> Dict[str, Any]:
    """The CLI behind its refusals and the table build: reads args.results, refines with `search`, writes the two files.  The
    paths are replayed on the host with the perm table; a refined solution is checked to end where the original ends."""
    data = data_utils.load_pickle(args.results)
    perm = _lib.cube3_perm_table()
    keys = ("states", "solutions", "paths", "times", "num_nodes_generated")
    results: Dict[str, List] = {k: list(data[k][args.start_idx:]) for k in keys}
    report: Dict[str, List] = {k: [] for k in STATS}
    for idx, (state, soln) in enumerate(zip(results["states"], results["solutions"])):
        start = time.time()
        moves, stats = refine_moves(search, soln, args.window, args.max_nodes) if len(soln) else (list(soln), {k: 0 for k in STATS})
        elapsed = time.time() - start
        if len(soln):
            path, end = [state], np.asarray(state.colors)
            for move in soln:
                end = end[perm[int(move)]]
            for move in moves:
                path.append(type(state)(path[-1].colors[perm[move]]))
            assert np.array_equal(path[-1].colors, end) and len(moves) <= len(soln)
            results["solutions"][idx], results["paths"][idx] = moves, path
            results["times"][idx] = results["times"][idx] + elapsed
        for k in STATS:
            report[k].append(stats[k])
        print("State: %i, # Moves: %i -> %i, passes %i, windows %i, # Nodes Gen: %s, unfinished %i, Time: %.3f"
              % (idx, stats["length_in"], stats["length_out"], stats["passes"], stats["windows"], format(stats["nodes"], ","),
                 stats["unfinished"], elapsed))
    n = max(sum(1 for s in results["solutions"] if len(s)), 1)
    print("mean length %.3f -> %.3f over %d solutions" % (sum(report["length_in"]) / n, sum(report["length_out"]) / n, n))
    data_utils.dump_pickle(results, "%s/results.pkl" % args.results_dir)
    data_utils.dump_pickle(report, "%s/refine.pkl" % args.results_dir)
    return report


def main(argv=None):
    args = build_parser().parse_args(argv)
    if str(args.env).lower() != "cube3":  # every refusal: before any device or file work
        raise ValueError("refine is built for cube3, not for %r: a sliding puzzle's window has no root of its own, the blank is part "
                         "of the state" % args.env)
    check_window(args.window)
    pdb = idastar.pattern_database(args)
    if args.max_nodes is None:
        args.max_nodes = idastar.default_max_nodes(args.env)
    if args.max_nodes <= 0:
        raise ValueError("--max_nodes must be positive, not %d" % args.max_nodes)
    os.makedirs(args.results_dir, exist_ok=True)
    if not args.debug:
        sys.stdout = data_utils.Logger("%s/output.txt" % args.results_dir, "w")
    start = time.time()
    pdb.build()
    print("pattern database %s: %d bytes, sweeps %s, built in %.2f s" % (pdb.spec, pdb.bytes, pdb.sweeps, time.time() - start))
    refine_file(args, idastar.IDAStar(args.env, pdb))


if __name__ == "__main__":
    main()
