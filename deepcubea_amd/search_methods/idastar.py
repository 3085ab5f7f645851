"""IDA* on the pattern databases (include/dca.h "IDA*", csrc/dca_idastar.hip): optimal solutions with no node pool.

    python -m deepcubea_amd.search_methods.idastar --states data/puzzle15/test/data_0.pkl --env puzzle15 \
        --model_dir pdb:5-5-5 --results_dir results/puzzle15_idastar

The batched A* engine (astar.py) keeps every generated node and stops at its pool's capacity; iterative-deepening A* keeps a move
stack per lane and runs as long as its node budget lets it.  With an admissible table set — every `pdb:` set is, `+dual`
included — the solution is optimal.  results.pkl has astar.py's format and keys (utils/compare_solutions.py reads it); idastar.pkl next to it holds, per
state, `solved`, `status`, `thresholds` and `nodes_per_threshold`.  A state that ends on "budget exhausted" is reported and
recorded as unsolved — an empty solution in results.pkl, solved = False in idastar.pkl — and the search goes on to the next; so
is a state whose root the library refuses (wrong parity, no permutation), with status "refused (...)".

`--batch K` (sliding puzzles, opt-in) searches the states in groups of K as batches of roots: one launch per round runs the next
threshold of every state of the group that is still searching (include/dca.h, dca_idastar_npuzzle_batch).  Every state's result
is what its single search gives; the files keep their formats, and `times` holds a group's wall seconds over its size."""
from __future__ import annotations

import os
import sys
import time
from argparse import ArgumentParser
from typing import Any, Dict, List

import numpy as np

from .. import _lib
from ..utils import data_utils, env_utils, search_utils

ENVS = ("puzzle8", "puzzle15", "puzzle24", "cube3")  # what the kernel is instantiated for

# The default --max_nodes: what a search gets through in about a minute, 60 s * the family's measured rate.  The rates are the
# lowest that profiles/idastar_probe.txt records for the family on one MI355X, nodes over seconds summed over the searches of at
# least 0.05 s: puzzle15 with 6-6-3 1.14e8 nodes/s (5-5-5: 1.95e8, puzzle24 6-6-6-6: 2.08e8), cube3 with korf 8.52e9 (korf7: 8.59e9).
MEASURED_NODES_PER_SECOND = {"puzzle": 1.14e8, "cube3": 8.52e9}
DEFAULT_MAX_NODES = {family: int(60 * rate) for family, rate in MEASURED_NODES_PER_SECOND.items()}


def default_max_nodes(env_name: str) -> int:
    return DEFAULT_MAX_NODES["cube3" if str(env_name).lower() == "cube3" else "puzzle"]


def pattern_database(args):
    """`--model_dir pdb:SPEC` for one of ENVS -> the pattern database, not built yet.  ValueError, with no device touched, for
    any other model, any other environment, and a spec the environment cannot have."""
    env_name = str(args.env).lower()
    if env_name not in ENVS:
        raise ValueError("IDA* is built for %s, not for %r" % (", ".join(ENVS), args.env))
    model = str(args.model_dir)
    if not model.startswith("pdb:"):
        raise ValueError("IDA* searches on pattern databases only: --model_dir pdb:SPEC, not %r" % model)
    spec = model.split(":", 1)[1]
    if env_name == "cube3":
        from ..utils.cube3_pdb import Cube3PatternDatabase
        return Cube3PatternDatabase(spec)  # (takes +sym / +sym:N and +dual, refuses a +reflect suffix)
    from ..utils.cube3_pdb import DUAL_SUFFIX, SYM_SUFFIX
    if any(t.strip().lower().startswith(DUAL_SUFFIX[1:]) for t in spec.split("+")[1:]):
        raise ValueError("pattern database %r: %s reads a table at the inverse of a state, and is defined for cube3 only; the blank "
                         "makes the inverse of a sliding-puzzle state no state of the same problem" % (spec, DUAL_SUFFIX))
    if spec.partition("+")[2].strip().lower().startswith(SYM_SUFFIX[1:]):
        raise ValueError("pattern database %r: %s reads a table at the images of a state under the cube's 48 symmetries, and is "
                         "defined for cube3 only; a sliding puzzle's one symmetry is +reflect" % (spec, SYM_SUFFIX))
    from ..utils.pattern_db import PatternDatabase
    pdb = PatternDatabase(env_name, spec)
    if len(pdb.partition) > _lib.IDASTAR_MAX_PUZZLE_PATTERNS:
        raise ValueError("IDA* takes at most %d patterns on a sliding puzzle, not %d" % (_lib.IDASTAR_MAX_PUZZLE_PATTERNS, len(pdb.partition)))
    if pdb.reflect and len(pdb.partition) > _lib.IDASTAR_MAX_REFLECT_PATTERNS:
        raise ValueError("IDA* with +reflect takes at most %d patterns (a lane keeps two running indices per pattern), not %d"
                         % (_lib.IDASTAR_MAX_REFLECT_PATTERNS, len(pdb.partition)))
    return pdb


class IDAStar:
    """IDA* for one environment on one built pattern database (utils/pattern_db.PatternDatabase for the sliding puzzles,
    utils/cube3_pdb.Cube3PatternDatabase for cube3)."""

    def __init__(self, env_name: str, pdb):
        self.env_name = str(env_name).lower()
        if self.env_name not in ENVS:
            raise ValueError("IDA* is built for %s, not for %r" % (", ".join(ENVS), env_name))
        self.env, self.dim = _lib.env_ids(self.env_name)[:2]
        self.pdb = pdb
        pdb._ready("build() or load() first")

    def solve(self, root, max_nodes: int = None) -> Dict[str, Any]:
        """-> {solved, moves, path_cost, nodes_generated, status, thresholds, nodes_per_threshold}; status is "solved", "budget
        exhausted" or "unsolvable".  A refused root (wrong parity, no permutation) raises DcaError."""
        if max_nodes is None:
            max_nodes = default_max_nodes(self.env_name)
        if self.env == _lib.ENV_CUBE3:
            return _lib.idastar_cube3(root, self.pdb.patterns, self.pdb.tables, max_nodes, sym=self.pdb.sym, dual=self.pdb.dual)
        return _lib.idastar_npuzzle(self.dim, root, self.pdb.partition, self.pdb.tables, max_nodes, reflect=self.pdb.reflect)

    def solve_batch(self, roots, max_nodes: int = None) -> List[Dict[str, Any]]:
        """A batch of 1 .. IDASTAR_MAX_BATCH sliding-puzzle roots searched in rounds, one launch per round (include/dca.h
        "batch") -> per root what solve() gives for it alone; max_nodes is per root.  One refused root refuses the whole batch:
        DcaError, "roots[i]: ...".  ValueError on cube3: a cube3 search of a shipped state fills the chip by itself."""
        if self.env == _lib.ENV_CUBE3:
            raise ValueError("IDA*: a batch of roots is searched on the sliding puzzles only; a cube3 search fills the chip by itself")
        if max_nodes is None:
            max_nodes = default_max_nodes(self.env_name)
        return _lib.idastar_npuzzle_batch(self.dim, roots, self.pdb.partition, self.pdb.tables, max_nodes, reflect=self.pdb.reflect)

    def solve_bounded(self, roots, max_length, max_nodes: int = None) -> List[Dict[str, Any]]:
        """A bounded batch of 1 .. IDASTAR_MAX_BATCH SHALLOW cube3 roots, one launch per round (include/dca.h "Bounded batches") ->
        per root what solve() gives for it alone, except that a root with no solution of at most max_length moves (an int, or
        one per root) ends with status "bounded" after the thresholds up to it.  max_nodes is per root.  This is what
        search_methods/refine.py searches a solution's windows with; a shipped state belongs to solve().  ValueError on the
        sliding puzzles, which have solve_batch."""
        if self.env != _lib.ENV_CUBE3:
            raise ValueError("IDA*: a bounded batch is searched on cube3 only; the sliding puzzles have solve_batch")
        if max_nodes is None:
            max_nodes = default_max_nodes(self.env_name)
        return _lib.idastar_cube3_batch(roots, self.pdb.patterns, self.pdb.tables, max_nodes, max_length=max_length, sym=self.pdb.sym,
                                        dual=self.pdb.dual)


def refused_root(err: Exception) -> Dict[str, Any]:
    """The result the CLI records for a root the library refuses (wrong parity, no permutation): unsolved, nothing searched."""
    return {"solved": False, "status": "refused (%s)" % str(err).split("bad argument: ", 1)[-1], "moves": [], "path_cost": float("inf"),
            "nodes_generated": 0, "thresholds": [], "nodes_per_threshold": []}


def solve_one(search: IDAStar, root, max_nodes: int) -> Dict[str, Any]:
    """The single search of one root; a root the library refuses is a result (refused_root), any other error is raised."""
    try:
        return search.solve(root, max_nodes)
    except _lib.DcaError as err:
        if "bad argument" not in str(err) or ": root:" not in str(err):
            raise  # a failed device call is no property of this state
        return refused_root(err)


def solve_group(search: IDAStar, roots, max_nodes: int) -> List[Dict[str, Any]]:
    """One group of the CLI's states: a single root on the single search, several as one batch.  A batch the library refuses for
    one of its roots ("roots[i]: ...") is run again root by root on the single search, which records the refused root and
    searches the others."""
    if len(roots) > 1:
        try:
            return search.solve_batch(np.stack(roots), max_nodes)
        except _lib.DcaError as err:
            if "bad argument" not in str(err) or ": roots[" not in str(err):
                raise
    return [solve_one(search, root, max_nodes) for root in roots]


def check_batch(env_name: str, batch: int) -> int:
    """--batch: 1 .. IDASTAR_MAX_BATCH, and 1 on cube3.  ValueError with no device touched."""
    if not 1 <= batch <= _lib.IDASTAR_MAX_BATCH:
        raise ValueError("--batch must be in 1..%d, not %d" % (_lib.IDASTAR_MAX_BATCH, batch))
    if batch > 1 and str(env_name).lower() == "cube3":
        raise ValueError("--batch %d: a batch of roots is searched on the sliding puzzles only; a cube3 search fills the chip by itself" % batch)
    return batch


def build_parser() -> ArgumentParser:
    parser = ArgumentParser()
    parser.add_argument('--states', type=str, required=True, help="File containing states to solve")
    parser.add_argument('--env', type=str, required=True, help="Environment: %s" % ", ".join(ENVS))
    parser.add_argument('--model_dir', type=str, required=True,
                        help="pdb:SPEC, as for astar.py: a preset (puzzle8 4-4; puzzle15 5-5-5, 6-6-3; puzzle24 6-6-6-6; auto; cube3 "
                             "corners, korf, korf7) or explicit groups.  On a sliding puzzle SPEC+reflect searches on the reflected "
                             "look-up (at most 4 patterns); on cube3 SPEC+sym searches on the symmetric look-ups, every table read again at "
                             "the state's images under the cube's 48 symmetries (SPEC+sym:N: the first N images of each pattern), and SPEC+dual "
                             "or SPEC+sym:N+dual reads every look-up a second time at the inverse state (d(s^-1) = d(s): admissible but "
                             "not consistent, which IDA* does not need; cube3 only).  Built on the GPU at start-up")
    parser.add_argument('--results_dir', type=str, required=True, help="Directory to save results")
    parser.add_argument('--start_idx', type=int, default=0, help="")
    parser.add_argument('--max_nodes', type=int, default=None,
                        help="node budget of one search; a state that runs out of it is recorded as unsolved.  The default is "
                             "about a minute of search on one MI355X at the measured rate: %d on the puzzles, %d on cube3"
                             % (DEFAULT_MAX_NODES["puzzle"], DEFAULT_MAX_NODES["cube3"]))
    parser.add_argument('--batch', type=int, default=1,
                        help="sliding puzzles: search the states in groups of this many consecutive states, every group as one batch "
                             "(one launch per round runs the next threshold of every state of the group still searching; 1 .. %d).  "
                             "Each state's result is what its single search gives; --max_nodes is per state; `times` holds the group's "
                             "wall seconds divided by the group's size.  A group with a state the library refuses is run again state by "
                             "state.  The default, 1, searches state by state; cube3 takes no other value (a shipped cube3 state fills the chip "
                             "by itself; batches of shallow cube3 roots are what search_methods/refine.py searches a solution's "
                             "windows with)" % _lib.IDASTAR_MAX_BATCH)
    parser.add_argument('--verbose', action='store_true', default=False, help="print every threshold's node count")
    parser.add_argument('--debug', action='store_true', default=False, help="do not copy the output to results_dir/output.txt")
    return parser


def main(argv=None):
    args = build_parser().parse_args(argv)
    pdb = pattern_database(args)  # every refusal of the model and the environment: before any device or file work
    check_batch(args.env, args.batch)
    if args.max_nodes is None:
        args.max_nodes = default_max_nodes(args.env)
    if args.max_nodes <= 0:
        raise ValueError("--max_nodes must be positive, not %d" % args.max_nodes)
    os.makedirs(args.results_dir, exist_ok=True)
    if not args.debug:
        sys.stdout = data_utils.Logger("%s/output.txt" % args.results_dir, "w")
    states = data_utils.load_pickle(args.states)['states'][args.start_idx:]
    env = env_utils.get_environment(args.env)
    start = time.time()
    pdb.build()
    print("pattern database %s: %d bytes, sweeps %s, built in %.2f s" % (pdb.spec, pdb.bytes, pdb.sweeps, time.time() - start))
    search = IDAStar(args.env, pdb)
    results: Dict[str, List] = {k: [] for k in ("solutions", "paths", "times", "num_nodes_generated", "solved", "status", "thresholds",
                                                "nodes_per_threshold")}
    results["states"] = states
    for idx, state in enumerate(states):
        if idx % args.batch == 0:  # the next group of --batch consecutive states (1: this state alone, on the single search)
            group = [np.ascontiguousarray(env._get_arr(s), dtype=np.uint8) for s in states[idx:idx + args.batch]]
            start = time.time()
            found = solve_group(search, group, args.max_nodes)
            elapsed = (time.time() - start) / len(group)
        res = found[idx % args.batch]
        soln: List[int] = res["moves"]
        path, cur = [state], state
        for move in soln:
            cur = env.next_state([cur], move)[0][0]
            path.append(cur)
        if res["solved"]:
            assert search_utils.is_valid_soln(state, soln, env)
        for key, value in (("solutions", soln), ("paths", path), ("times", elapsed), ("num_nodes_generated", res["nodes_generated"]),
                           ("solved", res["solved"]), ("status", res["status"]), ("thresholds", res["thresholds"]),
                           ("nodes_per_threshold", res["nodes_per_threshold"])):
            results[key].append(value)
        if res["solved"]:
            print("State: %i, SolnCost: %.2f, # Moves: %i, # Nodes Gen: %s, Time: %.2f"
                  % (idx, res["path_cost"], len(soln), format(res["nodes_generated"], ","), elapsed))
        else:
            print("State: %i, UNSOLVED (%s after %s nodes, last threshold %s), Time: %.2f"
                  % (idx, res["status"], format(res["nodes_generated"], ","), res["thresholds"][-1:] or "none", elapsed))
        if args.verbose:
            print("  thresholds %s\n  nodes      %s" % (res["thresholds"], res["nodes_per_threshold"]))
    unsolved = [i for i, ok in enumerate(results["solved"]) if not ok]
    print("%d of %d solved%s" % (len(states) - len(unsolved), len(states), "; unsolved: %s" % unsolved if unsolved else ""))
    keys = ("states", "solutions", "paths", "times", "num_nodes_generated")  # astar.py's results.pkl
    data_utils.dump_pickle({k: results[k] for k in keys}, "%s/results.pkl" % args.results_dir)
    data_utils.dump_pickle({k: v for k, v in results.items() if k not in keys}, "%s/idastar.pkl" % args.results_dir)


if __name__ == "__main__":
    main()
