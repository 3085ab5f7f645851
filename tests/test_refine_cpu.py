"""Bounded batches of cube3 roots and the window refiner, host side (no device needed): dca_idastar_host_cube3_batch
(include/dca_debug.h) runs the driver of dca_idastar_cube3_batch with the sequential lane in place of the kernel, and
search_methods/refine.py shortens a move list by re-solving its windows on it.  The batch's claim is equality with the single
searches, root by root; the bound's is a prefix of the unbounded search; the refiner's is a valid, no longer solution whose
short windows are all optimal."""
import ctypes as C
import os
import re
from functools import lru_cache

import numpy as np
import pytest

from tests import test_cube3_pdb_cpu as c3
from tests import test_cube3_sym_cpu as sym
from tests import test_idastar_cpu as ida
from tests.test_cube3_sym_cpu import no_device, prefix  # noqa: F401  (fixtures)

ROOT = sym.ROOT
BIG = ida.BIG
IDA_SET = sym.IDA_SET
CASES = ((2, 7), (0, 8), (0, 7), (1, 8))
MODES = {"plain": (0, False), "sym4": (4, False), "sym+dual": (sym.ALL, True)}
DEPTHS = (-1, 0, 2, 3)
GOAL = np.arange(54, dtype=np.uint8)


@lru_cache(maxsize=None)
def batch_roots():
    """The four recorded roots, the goal, and the first root again -> ([6, 54], each root's distance)."""
    roots = [ida.cube3_suffix_root(*case) for case in CASES] + [GOAL, ida.cube3_suffix_root(*CASES[0])]
    return np.stack(roots), [k for _, k in CASES] + [0, CASES[0][1]]


def completed(res):
    """The counts that are a property of the tree: all but the last of a search that a lane ended (the goal, the budget)."""
    per = res["nodes_per_threshold"]
    return per if res["status"] in ("unsolvable", "bounded") else per[:-1]


def same_search(got, want, root):
    """Root r of a batch against its single search: status, length, thresholds, completed counts; a valid move list."""
    assert got["status"] == want["status"] and got["solved"] == want["solved"] and got["path_cost"] == want["path_cost"], (got, want)
    assert len(got["moves"]) == len(want["moves"]) and got["thresholds"] == want["thresholds"], (got, want)
    assert completed(got) == completed(want) and len(got["nodes_per_threshold"]) == len(want["nodes_per_threshold"]), (got, want)
    assert got["nodes_generated"] == sum(got["nodes_per_threshold"])
    if got["solved"]:
        assert (ida.replay_cube3(root, got["moves"]) == GOAL).all()


def single(root, mode, max_nodes=BIG):
    from deepcubea_amd import _lib
    n, dual = MODES[mode]
    return _lib.idastar_host(_lib.ENV_CUBE3, 0, root, IDA_SET, sym.tables_of(IDA_SET), max_nodes, sym=n, dual=dual)


def batch(roots, mode, max_length=None, max_nodes=BIG):
    from deepcubea_amd import _lib
    n, dual = MODES[mode]
    return _lib.idastar_host_cube3_batch(roots, IDA_SET, sym.tables_of(IDA_SET), max_nodes, max_length=max_length, sym=n, dual=dual)


# ------------------------------------------------------------------------------------------------ the batch against the single searches
@pytest.mark.parametrize("mode", list(MODES))
def test_batch_equals_the_single_searches(prefix, mode):
    roots, distances = batch_roots()
    for depth in DEPTHS:
        prefix(depth)
        got = batch(roots, mode)
        assert len(got) == len(roots)
        for root, k, res in zip(roots, distances, got):
            same_search(res, single(root, mode), root)
            assert res["solved"] and len(res["moves"]) == k, (depth, k, res)
        assert got[5]["thresholds"] == got[0]["thresholds"] and completed(got[5]) == completed(got[0])  # the duplicate


@pytest.mark.parametrize("mode", list(MODES))
def test_the_bound_cuts_a_search_to_a_prefix_of_its_thresholds(prefix, mode):
    roots, distances = batch_roots()
    roots, distances = roots[:4], distances[:4]
    for depth in (-1, 3):
        prefix(depth)
        free = batch(roots, mode)
        below = batch(roots, mode, max_length=[k - 2 for k in distances])
        for res, want, k in zip(below, free, distances):
            n = len(res["thresholds"])
            assert res["status"] == "bounded" and not res["solved"] and res["moves"] == [] and res["path_cost"] == float("inf")
            assert res["thresholds"] == [T for T in want["thresholds"] if T <= k - 2] == want["thresholds"][:n]
            assert res["nodes_per_threshold"] == want["nodes_per_threshold"][:n] and n < len(want["thresholds"])
            assert res["nodes_generated"] == sum(res["nodes_per_threshold"])
        for bound in ([k for k in distances], None, 254, 1000):
            for root, res, want in zip(roots, batch(roots, mode, max_length=bound), free):
                same_search(res, want, root)
                assert res["solved"]
        # h(root) > B: nothing runs; a bound per root ends no other root's search; the goal is solved under any bound
        h_roots = [res["thresholds"][0] for res in free]
        mixed = batch(np.concatenate([roots, GOAL[None]]), mode, max_length=[h_roots[0] - 1, distances[1], 0, distances[3], 0])
        assert [r["status"] for r in mixed] == ["bounded", "solved", "bounded", "solved", "solved"]
        assert mixed[0]["thresholds"] == mixed[2]["thresholds"] == [] and mixed[0]["nodes_generated"] == 0
        same_search(mixed[1], free[1], roots[1])
        assert mixed[4]["moves"] == [] and mixed[4]["thresholds"] == []


def test_one_roots_budget_does_not_end_anothers_search():
    roots, _ = batch_roots()
    roots = roots[:5]  # the first root's plain search is the largest by far
    free = [single(r, "plain") for r in roots]
    max_nodes = max(res["nodes_generated"] for res in free[1:]) + 1
    assert max_nodes < sum(completed(free[0])), "the first root must run out before its last threshold"
    got = batch(roots, "plain", max_nodes=max_nodes)
    for root, res, want in zip(roots[1:], got[1:], free[1:]):
        same_search(res, want, root)
        assert res["solved"] and res == want
    assert got[0]["status"] == "budget exhausted" and got[0]["moves"] == [] and got[0]["path_cost"] == float("inf")
    same_search(got[0], single(roots[0], "plain", max_nodes), roots[0])
    assert max_nodes <= got[0]["nodes_generated"] <= max_nodes + 512  # the header's bound for one lane in flight: one poll interval


# ------------------------------------------------------------------------------------------------ refusals, ABI
SENTINEL = 77


def raw_batch(symbol="dca_idastar_host_cube3_batch", roots=None, n_roots=None, patterns=IDA_SET, tables=None, max_images=0, dual=0,
              max_length=None, max_nodes=1000000, null=(), extra=()):
    """The entry point called with ctypes, every output array pre-filled with SENTINEL -> (rc, message, outputs)."""
    from deepcubea_amd import _lib
    L = _lib.lib()
    roots = np.ascontiguousarray(batch_roots()[0][:3] if roots is None else roots, dtype=np.uint8)
    n = len(roots) if n_roots is None else n_roots
    m = max(len(roots), 1)
    out = {"status": np.full(m, SENTINEL, np.int32), "length": np.full(m, SENTINEL, np.int32), "moves": np.full((m, 64), SENTINEL, np.uint8),
           "count": np.full(m, SENTINEL, np.int32), "thresholds": np.full((m, 64), SENTINEL, np.int32),
           "per": np.full((m, 64), SENTINEL, np.int64), "total": np.full(m, SENTINEL, np.int64)}
    keep = [t if isinstance(t, int) else np.ascontiguousarray(t, dtype=np.uint8) for t in (sym.tables_of(patterns) if tables is None else tables)]
    arg = {"roots": roots, "kinds": np.array([k for k, _ in patterns], np.int32), "ids": np.array([c for _, g in patterns for c in g], np.uint8),
           "ks": np.array([len(g) for _, g in patterns], np.int32), **out}
    if max_length is not None:
        arg["bound"] = np.ascontiguousarray(max_length, dtype=np.int32)
    ptrs = (C.c_void_p * max(len(keep), 1))(*[t if isinstance(t, int) else t.ctypes.data for t in keep])

    def p(name):
        return None if name in null or name not in arg and name != "tables" else ptrs if name == "tables" else arg[name].ctypes.data_as(C.c_void_p)
    rc = getattr(L, symbol)(p("roots"), n, len(patterns), p("kinds"), p("ids"), p("ks"), p("tables"), max_images, dual, p("bound"), max_nodes,
                            p("status"), p("length"), p("moves"), 64, p("count"), p("thresholds"), p("per"), 64, p("total"), *extra)
    return rc, L.dca_last_error().decode(), out


def untouched(out):
    return all(bool((a == SENTINEL).all()) for a in out.values())


def test_refusals_need_no_device_and_write_no_output():
    from deepcubea_amd import _lib
    rc, _, out = raw_batch()
    assert rc == 0 and out["status"].tolist() == [0, 0, 0] and out["length"].tolist() == [7, 8, 7]
    assert bool((out["moves"][0, 7:] == SENTINEL).all()) and bool((out["thresholds"][1, out["count"][1]:] == SENTINEL).all())
    for n in (0, -1, 1025):
        rc, msg, out = raw_batch(n_roots=n)
        assert rc == -1 and "n_roots" in msg and "1..1024" in msg and untouched(out), msg
    for name in ("roots", "kinds", "ids", "ks", "tables", "status", "length", "count", "total", "moves", "thresholds", "per"):
        rc, msg, out = raw_batch(null=(name,))
        assert rc == -1 and "NULL" in msg and untouched(out), (name, msg)
    rc, msg, out = raw_batch(max_length=[5, -1, 5])
    assert rc == -1 and "max_length[1] = -1" in msg and "negative" in msg and untouched(out), msg
    twice = batch_roots()[0][:3].copy()
    twice[2][5] = twice[2][6]
    nostate = batch_roots()[0][:3].copy()
    nostate[1][[0, 10, 8, 12]] = nostate[1][[10, 0, 12, 8]]  # 54 distinct ids, two corner cubies in one slot
    for max_images, dual in ((0, 0), (4, 0), (48, 1)):
        rc, msg, out = raw_batch(roots=twice, max_images=max_images, dual=dual)
        assert rc == -1 and "dca_idastar_host_cube3_batch: roots[2]: " in msg and "once each" in msg and untouched(out), msg
    rc, msg, out = raw_batch(roots=nostate, max_images=48, dual=1)
    assert rc == -1 and "roots[1]: " in msg and "no cube state" in msg and untouched(out), msg
    assert raw_batch(roots=nostate, max_images=48, dual=0, max_nodes=100)[0] == 0  # only the dual search needs the slots
    for kw, word in ((dict(max_nodes=0), "max_nodes"), (dict(max_images=49), "max_images"), (dict(max_images=-1), "max_images"),
                     (dict(max_images=0, dual=1), "max_images"), (dict(patterns=((2, (0,)),), tables=[np.zeros(16, np.uint8)]), "kind"),
                     (dict(patterns=((0, (0, 0)),), tables=[np.zeros(16, np.uint8)]), "appears twice")):
        rc, msg, out = raw_batch(**kw)
        assert rc == -1 and word in msg and untouched(out), (kw, msg)
    # the Python wrappers: a bad root refuses the whole batch; roots of the wrong width and a short table are theirs to refuse
    with pytest.raises(_lib.DcaError, match=r"roots\[2\]: .*once each"):
        batch(twice, "plain")
    with pytest.raises(ValueError):
        batch(twice[:, :53], "plain")
    with pytest.raises(ValueError):
        _lib.idastar_host_cube3_batch(twice, IDA_SET, [sym.tables_of(IDA_SET)[0], sym.tables_of(IDA_SET)[1][:-1]], BIG)
    assert [r["solved"] for r in batch(batch_roots()[0], "sym4")] == [True] * 6  # the next valid call works


def test_abi_additions_are_declared_exported_and_version_6():
    from deepcubea_amd import _lib
    hdr = open(os.path.join(ROOT, "include", "dca.h")).read()
    dbg = open(os.path.join(ROOT, "include", "dca_debug.h")).read()
    L = _lib.lib()
    for name, where, other in (("dca_idastar_cube3_batch", hdr, dbg), ("dca_idastar_host_cube3_batch", dbg, hdr)):
        assert re.search(r"\bint %s\(" % name, where) and not re.search(r"\bint %s\(" % name, other), name
        assert name in _lib._SIGNATURES and name in _lib.ABI_SYMBOLS and hasattr(L, name), name
        decl = re.search(r"\bint %s\((.*?)\);" % name, where, re.S).group(1)
        params = [a.split() for a in re.sub(r"/\*.*?\*/", "", decl, flags=re.S).split(",")]
        letters = "".join("p" if "*" in " ".join(a) else {"int": "i", "int64_t": "l"}[a[0]] for a in params)
        assert _lib._SIGNATURES[name] == "i " + letters, (name, letters)
    assert _lib._SIGNATURES["dca_idastar_cube3_batch"] == _lib._SIGNATURES["dca_idastar_host_cube3_batch"] + "p"  # the stream
    assert "#define DCA_ABI_VERSION 6" in hdr and L.dca_abi_version() == 6
    assert int(re.search(r"#define DCA_IDASTAR_BOUNDED (\d+)", hdr).group(1)) == 3 == _lib.IDASTAR_BOUNDED
    assert _lib.IDASTAR_STATUS[3] == "bounded"
    flat = re.sub(r"\s*\n \*\s*", " ", hdr)
    for phrase in ("root r's status, length, thresholds and completed counts are those of the matching single entry point",
                   "no solution of at most B moves", "nothing is launched for it", "n_roots outside 1..DCA_IDASTAR_MAX_BATCH",
                   "roots[i]", "no cube state", "the whole call is refused", "with no output written", "max_nodes is per root",
                   "one memset, one upload, one launch and one read-back", "once per call"):
        assert phrase in flat, phrase


# ------------------------------------------------------------------------------------------------ refine_moves
class HostSearch:
    """IDAStar.solve_bounded on the host twin and IDA_SET's tables, in one look-up mode."""

    def __init__(self, mode="sym+dual"):
        self.mode = mode
        self.calls = 0

    def solve_bounded(self, roots, max_length, max_nodes=None):
        self.calls += 1
        return batch(roots, self.mode, max_length=max_length, max_nodes=BIG if max_nodes is None else max_nodes)


@lru_cache(maxsize=None)
def optimal_suffix(instance=0, k=10):
    """(root, moves): the state k moves from the goal on a shipped instance's optimal path and the k moves that solve it."""
    z = np.load(os.path.join(ROOT, "tests", "golden", "golden.npz"))
    L = int(z["cube3_test_opt_len"][instance])
    return ida.cube3_suffix_root(instance, k, z), tuple(int(a) for a in z["cube3_test_opt_moves"][instance][L - k:L])


def commuting_cycle(after):
    """a b a^1 b^1 on two opposite faces (they commute: the identity), on an axis other than the move in front of it."""
    face = next(f for f in (0, 2, 4) if f != (after >> 1) & ~1)
    a, b = 2 * face, 2 * (face ^ 1)
    return [a, b, a ^ 1, b ^ 1]


def padded_paths(at):
    """The optimal 10-move suffix made longer at position `at` in three ways -> {name: moves}, each still a solution."""
    _, moves = optimal_suffix()
    moves = list(moves)
    a = next(x for x in range(12) if x >> 1 not in (moves[at - 1] >> 1, moves[at] >> 1))
    return {"a a^1": moves[:at] + [a, a ^ 1] + moves[at:],
            "4-cycle": moves[:at] + commuting_cycle(moves[at - 1]) + moves[at:],
            "three quarter turns": moves[:at] + [moves[at] ^ 1] * 3 + moves[at + 1:]}


@lru_cache(maxsize=None)
def levels_to_5():
    """{state bytes: distance} for every state of the breadth-first levels 0..5 from the goal."""
    p = c3.perm_table()
    dist = {GOAL.tobytes(): 0}
    level = GOAL[None]
    for d in range(1, 6):
        nxt = np.unique(np.concatenate([level[:, p[a]] for a in range(12)]), axis=0)
        level = nxt[np.array([row.tobytes() not in dist for row in nxt])]
        dist.update((row.tobytes(), d) for row in level)
        assert len(level) == ida.LEVELS[d - 1]
    return dist


def assert_short_windows_optimal(moves, longest=6):
    from deepcubea_amd.search_methods import refine
    p, dist = c3.perm_table(), levels_to_5()
    for w in range(1, longest + 1):
        for i in range(len(moves) - w + 1):
            root = refine.window_root(p, moves[i:i + w])
            assert dist.get(root.tobytes(), 6) == w, (i, w, moves[i:i + w])  # (not in the levels 0..5: at least 6 away)


def test_window_root_is_solved_by_its_window():
    from deepcubea_amd.search_methods import refine
    root, moves = optimal_suffix()
    p = c3.perm_table()
    assert (refine.window_root(p, moves) == root).all() and (refine.window_root(p, []) == GOAL).all()
    for i in range(7):
        assert (ida.replay_cube3(refine.window_root(p, moves[i:i + 4]), moves[i:i + 4]) == GOAL).all()


@pytest.mark.parametrize("at", [1, 5])
@pytest.mark.parametrize("name", ["a a^1", "4-cycle", "three quarter turns"])
def test_refine_takes_the_padding_out(name, at):
    from deepcubea_amd.search_methods import refine
    root, _ = optimal_suffix()
    padded = padded_paths(at)[name]
    assert len(padded) > 10 and (ida.replay_cube3(root, padded) == GOAL).all()
    search = HostSearch()
    moves, stats = refine.refine_moves(search, padded, 8)
    assert (ida.replay_cube3(root, moves) == GOAL).all() and len(moves) == 10, (moves, stats)
    assert stats["length_in"] == len(padded) and stats["length_out"] == 10 and stats["unfinished"] == 0
    assert stats["passes"] == search.calls >= 2 and stats["windows"] > 0 and stats["nodes"] > 0
    assert_short_windows_optimal(moves)


def test_refine_leaves_an_optimal_path_alone_after_one_pass():
    from deepcubea_amd.search_methods import refine
    root, optimal = optimal_suffix()
    for mode in MODES:
        search = HostSearch(mode)
        moves, stats = refine.refine_moves(search, optimal, 8)
        assert moves == list(optimal) and search.calls == 1
        assert stats == {"length_in": 10, "length_out": 10, "passes": 1, "windows": 7, "nodes": stats["nodes"], "unfinished": 0}
    assert_short_windows_optimal(moves)
    short, stats = refine.refine_moves(HostSearch(), optimal[:3], 8)  # no window of 4 moves: nothing to search
    assert short == list(optimal[:3]) and stats["windows"] == 0 and stats["passes"] == 1
    for window in (3, 21, 0):
        with pytest.raises(ValueError, match="--window"):
            refine.refine_moves(HostSearch(), optimal, window)


def test_a_budget_of_one_node_leaves_the_path_as_it_is():
    from deepcubea_amd.search_methods import refine
    root, _ = optimal_suffix()
    padded = padded_paths(5)["a a^1"]
    search = HostSearch()
    first = batch(np.stack([refine.window_root(c3.perm_table(), padded[i:i + min(8, 12 - i)]) for i in range(9)]), "sym+dual",
                  max_length=[min(8, 12 - i) - 2 for i in range(9)], max_nodes=1)
    out_of_budget = sum(1 for res in first if res["status"] == "budget exhausted")
    assert out_of_budget >= 5 and all(res["status"] in ("budget exhausted", "bounded") for res in first)
    moves, stats = refine.refine_moves(search, padded, 8, max_nodes=1)
    assert moves == padded and (ida.replay_cube3(root, moves) == GOAL).all()
    assert stats["unfinished"] == out_of_budget and stats["passes"] == 1 and stats["windows"] == 9 and stats["length_out"] == 12


# ------------------------------------------------------------------------------------------------ the CLI
def cli_args(tmp_path, *more):
    from deepcubea_amd.search_methods import refine
    return refine.build_parser().parse_args(["--results", str(tmp_path / "in" / "results.pkl"), "--env", "cube3", "--model_dir", "pdb:korf7+dual",
                                             "--window", "8", "--results_dir", str(tmp_path / "out"), *more])


def test_cli_round_trip_on_three_states(tmp_path, no_device):
    from deepcubea_amd.environments.cube3 import Cube3State
    from deepcubea_amd.search_methods import refine
    from deepcubea_amd.utils import data_utils
    root, optimal = optimal_suffix()
    p = c3.perm_table()
    solutions = [padded_paths(5)["a a^1"], [], list(optimal)]
    states = [Cube3State(root.copy()), Cube3State(GOAL.copy()), Cube3State(root.copy())]
    data = {"states": states, "solutions": solutions, "paths": [[s] for s in states], "times": [1.0, 2.0, 3.0],
            "num_nodes_generated": [10, 0, 30]}
    os.makedirs(tmp_path / "in")
    os.makedirs(tmp_path / "out")
    data_utils.dump_pickle(data, str(tmp_path / "in" / "results.pkl"))
    report = refine.refine_file(cli_args(tmp_path), HostSearch())
    got = data_utils.load_pickle(str(tmp_path / "out" / "results.pkl"))
    assert data_utils.load_pickle(str(tmp_path / "out" / "refine.pkl")) == report
    assert set(got) == set(data) and got["num_nodes_generated"] == [10, 0, 30]
    assert [len(s) for s in got["solutions"]] == [10, 0, 10] and got["solutions"][2] == list(optimal)
    assert report["length_in"] == [12, 0, 10] and report["length_out"] == [10, 0, 10] and report["unfinished"] == [0, 0, 0]
    assert report["passes"][1] == 0 and report["windows"][1] == 0 and set(report) == set(refine.STATS)
    for i, (state, moves, path, before) in enumerate(zip(got["states"], got["solutions"], got["paths"], data["times"])):
        assert len(path) == len(moves) + 1 and (path[0].colors == state.colors).all() and got["times"][i] >= before
        for a, prev, cur in zip(moves, path, path[1:]):
            assert (cur.colors == prev.colors[p[a]]).all()
        assert (path[-1].colors == GOAL).all()
    assert got["times"][1] == 2.0
    tail = refine.refine_file(cli_args(tmp_path, "--start_idx", "2"), HostSearch())
    assert tail["length_in"] == [10]


def test_cli_refusals_touch_no_device_and_no_file(tmp_path, no_device):
    from deepcubea_amd.search_methods import refine
    base = ["--results", str(tmp_path / "none.pkl"), "--results_dir", str(tmp_path / "out")]
    for env, model in (("puzzle15", "pdb:5-5-5"), ("puzzle8", "pdb:4-4"), ("lightsout7", "exact:gf2")):
        with pytest.raises(ValueError, match="built for cube3.*the blank is part of the state"):
            refine.main(base + ["--env", env, "--model_dir", model])
    for window in ("3", "21", "0", "-4"):
        with pytest.raises(ValueError, match=r"--window must be in 4\.\.20"):
            refine.main(base + ["--env", "cube3", "--model_dir", "pdb:korf7+dual", "--window", window])
    with pytest.raises(ValueError, match="pattern databases only"):
        refine.main(base + ["--env", "cube3", "--model_dir", "saved_models/cube3/current"])
    with pytest.raises(ValueError, match="--max_nodes"):
        refine.main(base + ["--env", "cube3", "--model_dir", "pdb:korf7", "--max_nodes", "0"])
    assert not (tmp_path / "out").exists()
    help_text = " ".join(refine.build_parser().format_help().split())
    assert "--window" in help_text and "whose search finished is optimal" in help_text and "counted as unfinished" in help_text
    assert refine.build_parser().parse_args(base + ["--env", "cube3", "--model_dir", "pdb:korf7"]).window == 14


def test_solve_bounded_is_cube3s_and_solve_batch_stays_the_puzzles():
    from deepcubea_amd.search_methods import idastar
    search = idastar.IDAStar.__new__(idastar.IDAStar)
    search.env = idastar._lib.ENV_NPUZZLE
    with pytest.raises(ValueError, match="cube3 only"):
        search.solve_bounded(None, 4)
    search.env = idastar._lib.ENV_CUBE3
    with pytest.raises(ValueError, match="sliding puzzles only"):
        search.solve_batch(None)
