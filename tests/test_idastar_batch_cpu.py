"""Batches of sliding-puzzle roots, host side (no device needed): dca_idastar_host_batch (include/dca_debug.h) runs the batch
driver of dca_idastar_npuzzle_batch — an IdaRun per root, rounds of one threshold per active root — with the sequential lane in
place of the kernel.  The claim is equality: root r's outputs are those of the single search of that root alone."""
import ctypes as C
import os
import re

import numpy as np
import pytest

from tests.test_cube3_sym_cpu import no_device  # noqa: F401  (fixture)
from tests.test_idastar_cpu import P8_PARTITION, p8_states_at, p8_tables, prefix, puzzle_goal, replay_puzzle  # noqa: F401  (prefix: fixture)

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
BIG = 1 << 40
DISTANCES = (0, 1, 2, 3, 10, 20, 26, 30, 31)  # 0: the goal; 31: the deepest an 8-puzzle gets
DEPTHS = (-1, 0, 2, 7)


def p8_roots(distances=DISTANCES):
    return np.stack([p8_states_at(d, 1, seed=13)[0] for d in distances])


def completed(res):
    """The counts that are a property of the tree: all but the last of a search that a lane ended (the goal, the budget)."""
    per = res["nodes_per_threshold"]
    return per if res["status"] == "unsolvable" else per[:-1]


def same_search(got, want, root, dim=3):
    """Root r of a batch against its single search: status, length, thresholds, completed counts; a valid move list."""
    assert got["status"] == want["status"] and got["solved"] == want["solved"] and got["path_cost"] == want["path_cost"], (got, want)
    assert len(got["moves"]) == len(want["moves"]) and got["thresholds"] == want["thresholds"], (got, want)
    assert completed(got) == completed(want) and len(got["nodes_per_threshold"]) == len(want["nodes_per_threshold"]), (got, want)
    assert got["nodes_generated"] == sum(got["nodes_per_threshold"])
    if got["solved"]:
        assert np.array_equal(replay_puzzle(dim, root, got["moves"]), puzzle_goal(dim))


def single(root, max_nodes=BIG, reflect=False):
    from deepcubea_amd import _lib
    return _lib.idastar_host(_lib.ENV_NPUZZLE, 3, root, P8_PARTITION, p8_tables(), max_nodes, reflect=reflect)


def batch(roots, max_nodes=BIG, reflect=False):
    from deepcubea_amd import _lib
    return _lib.idastar_host_batch(3, roots, P8_PARTITION, p8_tables(), max_nodes, reflect=reflect)


# ------------------------------------------------------------------------------------------------ equality with the single searches
@pytest.mark.parametrize("reflect", [False, True])
def test_batch_equals_the_single_searches(prefix, reflect):
    roots = p8_roots()
    for depth in DEPTHS:
        prefix(depth)
        got = batch(roots, reflect=reflect)
        assert len(got) == len(roots)
        for root, distance, res in zip(roots, DISTANCES, got):
            same_search(res, single(root, reflect=reflect), root)
            assert res["solved"] and len(res["moves"]) == distance, (depth, distance, res)


def test_no_state_leaks_between_roots_or_calls():
    root = p8_states_at(26, 1, seed=13)[0]
    want = single(root)
    got = batch(np.stack([root, root, root]))
    for res in got:
        assert res["thresholds"] == want["thresholds"] and res["nodes_per_threshold"] == got[0]["nodes_per_threshold"]
        same_search(res, want, root)
    one = batch(root[None])
    assert len(one) == 1 and one[0] == want  # the same driver steps on the same sequential lane: every field


def test_one_roots_budget_does_not_end_anothers_search():
    shallow, deep = (0, 1, 2, 3, 10, 20), 31
    roots = p8_roots(shallow + (deep,))
    free = [single(r) for r in roots]
    max_nodes = max(res["nodes_generated"] for res in free[:-1]) + 1
    assert max_nodes < sum(completed(free[-1])), "the deep root must run out before its last threshold"
    got = batch(roots, max_nodes)
    for root, res, want in zip(roots[:-1], got[:-1], free[:-1]):
        same_search(res, want, root)
        assert res["solved"] and res == want
    last = got[-1]
    assert last["status"] == "budget exhausted" and not last["solved"] and last["moves"] == [] and last["path_cost"] == float("inf")
    same_search(last, single(roots[-1], max_nodes), roots[-1])
    assert max_nodes <= last["nodes_generated"] <= max_nodes + 512  # the header's bound for one lane in flight: one poll interval


# ------------------------------------------------------------------------------------------------ refusals, ABI, CLI
SENTINEL = 77


def raw_batch(symbol="dca_idastar_host_batch", dim=3, roots=None, n_roots=None, np_=2, ids=(1, 2, 3, 4, 5, 6, 7, 8), ks=(4, 4),
              tables=None, reflect=0, max_nodes=1000000, null=(), extra=()):
    """The entry point called with ctypes, every output array pre-filled with SENTINEL -> (rc, message, outputs).  tables: host
    arrays, or addresses (the device entry point's); extra: that entry point's stream."""
    from deepcubea_amd import _lib
    L = _lib.lib()
    roots = np.ascontiguousarray(p8_roots((10, 12, 14)) if roots is None else roots, dtype=np.uint8)
    n = len(roots) if n_roots is None else n_roots
    m = max(len(roots), 1)
    out = {"status": np.full(m, SENTINEL, np.int32), "length": np.full(m, SENTINEL, np.int32), "moves": np.full((m, 64), SENTINEL, np.uint8),
           "count": np.full(m, SENTINEL, np.int32), "thresholds": np.full((m, 64), SENTINEL, np.int32),
           "per": np.full((m, 64), SENTINEL, np.int64), "total": np.full(m, SENTINEL, np.int64)}
    keep = [t if isinstance(t, int) else np.ascontiguousarray(t, dtype=np.uint8) for t in (p8_tables() if tables is None else tables)]
    arg = {"roots": roots, "ids": np.ascontiguousarray(ids, dtype=np.uint8), "ks": np.ascontiguousarray(ks, dtype=np.int32), **out}
    ptrs = (C.c_void_p * max(len(keep), 1))(*[t if isinstance(t, int) else t.ctypes.data for t in keep])

    def p(name):
        return None if name in null else ptrs if name == "tables" else arg[name].ctypes.data_as(C.c_void_p)
    rc = getattr(L, symbol)(dim, p("roots"), n, np_, p("ids"), p("ks"), p("tables"), reflect, max_nodes, p("status"), p("length"), p("moves"),
                            64, p("count"), p("thresholds"), p("per"), 64, p("total"), *extra)
    return rc, L.dca_last_error().decode(), out


def untouched(out):
    return all(bool((a == SENTINEL).all()) for a in out.values())


def bad_roots():
    """(roots, index of the bad one, the message's word): a wrong parity at 1, a tile twice at 2, a byte >= N at 0."""
    good = p8_roots((10, 12, 14))
    a, b = [i for i in range(9) if good[1][i] != 0][:2]
    odd = good.copy()
    odd[1][a], odd[1][b] = odd[1][b], odd[1][a]
    twice = good.copy()
    twice[2][a] = twice[2][b]
    big = good.copy()
    big[0][a] = 9
    return (odd, 1, "parity"), (twice, 2, "appears twice"), (big, 0, "is not a tile")


def test_refusals_need_no_device_and_write_no_output():
    from deepcubea_amd import _lib
    rc, _, out = raw_batch()
    assert rc == 0 and out["status"].tolist() == [0, 0, 0] and out["length"].tolist() == [10, 12, 14]
    assert bool((out["moves"][0, 10:] == SENTINEL).all()) and bool((out["thresholds"][1, out["count"][1]:] == SENTINEL).all())
    for n in (0, -1, 1025):
        rc, msg, out = raw_batch(n_roots=n)
        assert rc == -1 and "n_roots" in msg and "1..1024" in msg and untouched(out), msg
    for name in ("roots", "ids", "ks", "tables", "status", "length", "count", "total", "moves", "thresholds", "per"):
        rc, msg, out = raw_batch(null=(name,))
        assert rc == -1 and "NULL" in msg and untouched(out), (name, msg)
    for roots, i, word in bad_roots():
        for reflect in (0, 1):
            rc, msg, out = raw_batch(roots=roots, reflect=reflect)
            assert rc == -1 and "roots[%d]: " % i in msg and word in msg and "dca_idastar_host_batch" in msg and untouched(out), msg
    pairs = [t for t in range(1, 9)]
    five = dict(dim=3, np_=5, ids=pairs[:5], ks=(1,) * 5, tables=[np.zeros(81, np.uint8)] * 5)
    rc, msg, out = raw_batch(reflect=1, **five)
    assert rc == -1 and "num_patterns" in msg and "1..4" in msg and untouched(out), msg
    assert raw_batch(reflect=0, **five)[0] == 0  # five patterns are the plain search's to take
    for kw, word in ((dict(max_nodes=0), "max_nodes"), (dict(dim=6, roots=np.zeros((1, 36))), "3..5"), (dict(dim=2), "dim"),
                     (dict(np_=0), "num_patterns"), (dict(np_=9), "num_patterns"), (dict(ids=(1, 2, 3, 4, 4, 6, 7, 8)), "appears twice")):
        rc, msg, out = raw_batch(**kw)
        assert rc == -1 and word in msg and untouched(out), (kw, msg)
    # the Python wrappers: a bad root refuses the whole batch; roots of the wrong width and a short table are theirs to refuse
    odd = bad_roots()[0][0]
    with pytest.raises(_lib.DcaError, match=r"roots\[1\]: .*parity"):
        batch(odd)
    with pytest.raises(ValueError):
        batch(odd[:, :8])
    with pytest.raises(ValueError):
        _lib.idastar_host_batch(3, odd, P8_PARTITION, [p8_tables()[0], p8_tables()[1][:-1]], BIG)
    assert [r["solved"] for r in batch(p8_roots((10, 12, 14)))] == [True] * 3  # the next valid call works


def test_abi_additions_are_declared_exported_and_version_6():
    from deepcubea_amd import _lib
    hdr = open(os.path.join(ROOT, "include", "dca.h")).read()
    dbg = open(os.path.join(ROOT, "include", "dca_debug.h")).read()
    L = _lib.lib()
    for name, where, other in (("dca_idastar_npuzzle_batch", hdr, dbg), ("dca_idastar_host_batch", dbg, hdr)):
        assert re.search(r"\bint %s\(" % name, where) and not re.search(r"\bint %s\(" % name, other), name
        assert name in _lib._SIGNATURES and name in _lib.ABI_SYMBOLS and hasattr(L, name), name
        decl = re.search(r"\bint %s\((.*?)\);" % name, where, re.S).group(1)
        params = [a.split() for a in re.sub(r"/\*.*?\*/", "", decl, flags=re.S).split(",")]
        letters = "".join("p" if "*" in " ".join(a) else {"int": "i", "int64_t": "l"}[a[0]] for a in params)
        assert _lib._SIGNATURES[name] == "i " + letters, (name, letters)
    assert _lib._SIGNATURES["dca_idastar_npuzzle_batch"] == _lib._SIGNATURES["dca_idastar_host_batch"] + "p"  # the stream
    assert "#define DCA_ABI_VERSION 6" in hdr and L.dca_abi_version() == 6
    assert int(re.search(r"#define DCA_IDASTAR_MAX_BATCH (\d+)", hdr).group(1)) == 1024 == _lib.IDASTAR_MAX_BATCH
    flat = re.sub(r"\s*\n \*\s*", " ", hdr)
    for phrase in ("root r's outputs are those of dca_idastar_npuzzle (or dca_idastar_npuzzle_reflected where reflect != 0) called on "
                   "that root alone with the same max_nodes", "a move list that solves the root at that length (it need not be the same list)",
                   "every completed threshold's count", "the last threshold's count varies", "the budget bounds are the single search's, per root",
                   "One root's budget or solution does not end another's search", "roots[i]", "the whole call is refused",
                   "n_roots outside 1..DCA_IDASTAR_MAX_BATCH", "with no output written"):
        assert phrase in flat, phrase


def test_cli_refuses_a_bad_batch_before_any_device_or_file_work(no_device, tmp_path):
    from deepcubea_amd.search_methods import idastar
    args = idastar.build_parser().parse_args(["--states", "s.pkl", "--env", "puzzle15", "--model_dir", "pdb:5-5-5", "--results_dir", "r"])
    assert args.batch == 1
    help_text = " ".join(idastar.build_parser().format_help().split())
    assert "--batch" in help_text and "wall seconds divided by the group's size" in help_text
    for env, model, value in (("puzzle8", "pdb:4-4", "0"), ("puzzle15", "pdb:5-5-5", "-3"), ("puzzle15", "pdb:5-5-5", "2000"),
                              ("puzzle24", "pdb:6-6-6-6", "1025"), ("cube3", "pdb:korf", "4"), ("cube3", "pdb:corners", "2")):
        with pytest.raises(ValueError, match="--batch"):
            idastar.main(["--states", str(tmp_path / "none.pkl"), "--env", env, "--model_dir", model, "--results_dir", str(tmp_path / "out"),
                          "--batch", value])
    assert not (tmp_path / "out").exists()
    assert idastar.check_batch("cube3", 1) == 1 and idastar.check_batch("puzzle15", 1024) == 1024
    with pytest.raises(ValueError, match="sliding puzzles only"):  # the class refuses a cube3 batch before it reads its arguments
        search = idastar.IDAStar.__new__(idastar.IDAStar)
        search.env = idastar._lib.ENV_CUBE3
        search.solve_batch(None)
