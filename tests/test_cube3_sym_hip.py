"""GPU: the symmetric look-ups for the cube3 pattern databases (dca_cube3_pdb_eval_sym, dca_idastar_cube3_sym, `pdb:<spec>+sym`).
Integer arithmetic throughout, so every comparison is exact: the eval kernel against its host twin (which tests/test_cube3_sym_cpu.py
checks against rows conjugated in numpy), the kernel's IDA* against the same frame run on the host, lengths against the shipped
optimal paths."""
import os
import sys

import numpy as np
import pytest
import torch

from tests import test_cube3_pdb_cpu as c3
from tests import test_cube3_sym_cpu as sym
from tests import test_idastar_cpu as ida

pytestmark = pytest.mark.gpu

BIG = 1 << 40
ALL = sym.ALL
SMALL4 = tuple(c3.SMALL.values())


@pytest.fixture(scope="module")
def L():
    from deepcubea_amd import _lib
    _lib.require_gpu()
    yield _lib
    _lib.idastar_set_prefix(-1)


@pytest.fixture
def prefix(L):
    yield L.idastar_set_prefix
    L.idastar_set_prefix(-1)


def dev(a):
    a = np.ascontiguousarray(a)
    return torch.from_numpy(a if a.flags.writeable else a.copy()).cuda()  # (the host reference's arrays are read-only)


@pytest.fixture(scope="module")
def small(L):
    """The four small patterns: (host tables, device tables)."""
    host = sym.tables_of(SMALL4)
    return host, [dev(t) for t in host]


@pytest.fixture(scope="module")
def korf(L):
    """korf built once: the plain search and the searches on its images share the tables."""
    from deepcubea_amd.search_methods.idastar import IDAStar
    from deepcubea_amd.utils.cube3_pdb import Cube3PatternDatabase
    plain = Cube3PatternDatabase("korf").build()

    def search(n):
        pdb = Cube3PatternDatabase("korf", sym=n)
        pdb.tables, pdb.sweeps = plain.tables, plain.sweeps
        return IDAStar("cube3", pdb)
    return search


@pytest.fixture(scope="module")
def eval_rows():
    """A few thousand rows: scrambles, path states, rows of valid bytes that are no cube states, and any bytes."""
    rng = np.random.default_rng(51)
    junk = rng.integers(0, 256, (600, 54)).astype(np.uint8)
    junk[:300] %= 54
    rows = np.concatenate([c3.scrambles(2200, 40, 52), c3.path_states()[0][::31], junk])
    rows.setflags(write=False)
    return rows


# ------------------------------------------------------------------------------------------------ eval
@pytest.mark.parametrize("row_kind", [c3.ROWS_STATE, c3.ROWS_NNET])
@pytest.mark.parametrize("n", [1, 3, ALL])
def test_eval_kernel_equals_the_host_twin(L, small, eval_rows, n, row_kind):
    host, tables = small
    rows = eval_rows if row_kind == c3.ROWS_STATE else np.where(eval_rows < 54, eval_rows // 9, eval_rows).astype(np.uint8)
    want = L.cube3_pdb_eval_host(rows, row_kind, SMALL4, host, sym=n)
    if n == 1:
        assert torch.equal(L.cube3_pdb_eval(dev(rows), row_kind, SMALL4, tables).cpu(), torch.from_numpy(want))  # the plain kernel
    for ld in (54, 56, 64):
        for offset in (0, 1):  # aligned and unaligned bases: the word-load and the byte-load kernel
            flat = torch.full((len(rows) * ld + 8,), 0xA5, dtype=torch.uint8, device="cuda")
            view = flat[offset:offset + len(rows) * ld].view(len(rows), ld)[:, :54]
            view.copy_(dev(rows))
            got = L.cube3_pdb_eval(view, row_kind, SMALL4, tables, sym=n)
            assert got.dtype == torch.float32 and torch.equal(got.cpu(), torch.from_numpy(want)), (n, row_kind, ld, offset)
    assert L.cube3_pdb_eval(dev(rows[:0]), row_kind, SMALL4, tables, sym=n).numel() == 0


def test_eval_through_the_class_and_the_engine_closure(L, small):
    from deepcubea_amd.utils.cube3_pdb import Cube3PatternDatabase
    host, _ = small
    states, dist, _ = c3.path_states()
    plain, full = sym.path_values()
    pdb = Cube3PatternDatabase(SMALL4, sym=ALL).set_tables(host)
    assert pdb.spec.endswith("+sym") and pdb.bytes == sum(t.size for t in host)
    assert np.array_equal(pdb.heuristic(dev(states)).cpu().numpy(), full.astype(np.float32))
    assert np.array_equal(pdb.heuristic_fn_dev()(dev(states // 9)).cpu().numpy(), full.astype(np.float32))  # the closure: colour rows
    one = Cube3PatternDatabase(SMALL4, sym=1).set_tables(host)
    assert np.array_equal(one.heuristic(dev(states)).cpu().numpy(), plain.astype(np.float32))


# ------------------------------------------------------------------------------------------------ IDA*
@pytest.mark.parametrize("depth", [-1, 3])
@pytest.mark.parametrize("case", list(sym.IDA_CASES), ids=lambda c: "root%d-%d" % c)
def test_kernel_idastar_equals_the_host_frame(L, prefix, case, depth):
    root = ida.cube3_suffix_root(*case)
    host = sym.tables_of(sym.IDA_SET)
    tables = [dev(t) for t in host]
    prefix(depth)
    for n in (ALL, 2):
        want = L.idastar_host(L.ENV_CUBE3, 0, root, sym.IDA_SET, host, BIG, sym=n)
        got = L.idastar_cube3(root, sym.IDA_SET, tables, BIG, sym=n)
        assert got["solved"] and len(got["moves"]) == case[1] == len(want["moves"])
        assert np.array_equal(ida.replay_cube3(root, got["moves"]), np.arange(54))
        assert got["thresholds"] == want["thresholds"] and got["nodes_per_threshold"][:-1] == want["nodes_per_threshold"][:-1]
        assert got["nodes_generated"] == sum(got["nodes_per_threshold"])
        if n == ALL:
            assert got["thresholds"][:-1] == sym.IDA_CASES[case][1][0] and got["nodes_per_threshold"][:-1] == sym.IDA_CASES[case][1][1]


@pytest.mark.parametrize("instance", [0, 1])
def test_korf_sym_solves_the_suffix_roots_at_their_length(korf, instance):
    search, plain = korf(ALL), korf(0)
    for k in (0, 1, 2, 3, 4, 5, 6, 8, 10, 12, 14):
        root = ida.cube3_suffix_root(instance, k)
        res = search.solve(root, BIG)
        print("cube3 instance %d, %d from the goal: nodes %d, thresholds %s" % (instance, k, res["nodes_generated"], res["thresholds"]))
        assert res["solved"] and len(res["moves"]) == k == res["path_cost"], res
        assert np.array_equal(ida.replay_cube3(root, res["moves"]), np.arange(54))
        assert res["nodes_generated"] == sum(res["nodes_per_threshold"]) and (not k or res["thresholds"][-1] == k)
        assert all(a < b for a, b in zip(res["thresholds"], res["thresholds"][1:]))
        if k in (10, 12):  # an admissible, larger h: the first threshold is no lower, a shared completed threshold's tree no larger
            ref = plain.solve(root, BIG)
            assert res["thresholds"][0] >= ref["thresholds"][0]
            for T, count in zip(res["thresholds"][:-1], res["nodes_per_threshold"][:-1]):
                if T in ref["thresholds"][:-1]:
                    assert count <= ref["nodes_per_threshold"][ref["thresholds"].index(T)], (k, T)


def test_korf_sym_1_is_the_plain_search(korf, prefix):
    one, plain = korf(1), korf(0)
    assert one.pdb.spec.endswith("+sym:1") and plain.pdb.sym == 0
    for depth in (-1, 3):
        prefix(depth)
        for instance, k in ((0, 12), (1, 13)):
            root = ida.cube3_suffix_root(instance, k)
            a, b = one.solve(root, BIG), plain.solve(root, BIG)
            assert a["thresholds"] == b["thresholds"] and a["nodes_per_threshold"][:-1] == b["nodes_per_threshold"][:-1]
            assert len(a["moves"]) == len(b["moves"]) == k


def test_budget_exhausted_is_never_solved_and_bounded(L, korf):
    search = korf(ALL)
    root = ida.cube3_suffix_root(0, 14)
    full = search.solve(root, BIG)
    assert full["solved"] and sum(full["nodes_per_threshold"][:-1]) > 1000
    for max_nodes in (1, 1000):  # budgets that end before the last threshold starts
        res = search.solve(root, max_nodes)
        print("budget %d: %s" % (max_nodes, res))
        assert res["status"] == "budget exhausted" and not res["solved"] and res["moves"] == [] and res["path_cost"] == float("inf")
        assert res["nodes_generated"] == sum(res["nodes_per_threshold"]) and res["thresholds"][-1] < 14
        assert max_nodes <= res["nodes_generated"] <= max_nodes + max(max_nodes // 2, L.IDASTAR_MAX_LANES)  # the header's bounds
        assert res["nodes_generated"] <= max_nodes + L.IDASTAR_OVERSHOOT
    assert search.solve(root, 1)["nodes_generated"] <= 2  # one item, one lane, an interval of 1


def test_device_refusals(L, korf, small):
    host, tables = small
    root = ida.cube3_suffix_root(0, 3)
    rows = dev(c3.scrambles(8, 10, 1))
    for bad in (-1, 49):
        with pytest.raises(L.DcaError, match="max_images"):
            L.idastar_cube3(root, SMALL4, tables, 1000, sym=bad)
        with pytest.raises(L.DcaError, match="max_images"):
            L.cube3_pdb_eval(rows, c3.ROWS_STATE, SMALL4, tables, sym=bad)
    three = (c3.SMALL["c0,c1,c2"], (c3.CORNERS, (5, 6, 7)), (c3.CORNERS, (1, 2, 4)))  # 72 look-ups
    for call in (lambda n: L.idastar_cube3(root, three, [tables[0]] * 3, 1000, sym=n),
                 lambda n: L.cube3_pdb_eval(rows, c3.ROWS_STATE, three, [tables[0]] * 3, sym=n)):
        with pytest.raises(L.DcaError, match=r"DCA_CUBE3_SYM_MAX_LOOKUPS = 64.*\+sym:N"):
            call(ALL)
        call(21)
    for n in (0, -5):
        with pytest.raises(L.DcaError, match="max_nodes"):
            korf(ALL).solve(root, n)
    bad = np.arange(54)
    bad[7] = 8
    with pytest.raises(L.DcaError, match="once each"):
        korf(ALL).solve(bad, 1000)
    with pytest.raises(ValueError, match="uint8 device tensor"):  # a host address must never reach the kernel's gathers
        L.idastar_cube3(root, SMALL4, host, 1000, sym=ALL)
    with pytest.raises(ValueError):
        L.cube3_pdb_eval(rows, c3.ROWS_STATE, SMALL4, tables[:3] + [tables[3][:-1]], sym=ALL)
    with pytest.raises(L.DcaError, match="ld"):
        L.cube3_pdb_eval(rows[:, :50], c3.ROWS_STATE, SMALL4, tables, sym=ALL)


# ------------------------------------------------------------------------------------------------ the CLIs
def test_both_clis_on_a_ten_move_root(tmp_path, L):
    from deepcubea_amd.environments.cube3 import Cube3State
    from deepcubea_amd.search_methods import astar, idastar
    from deepcubea_amd.utils import data_utils
    root = np.asarray(ida.cube3_suffix_root(1, 10), dtype=np.uint8)
    spath = str(tmp_path / "states.pkl")
    data_utils.dump_pickle({"states": [Cube3State(root.copy())]}, spath)
    for name, run in (("astar", lambda d: astar.main(["--states", spath, "--env", "cube3", "--model_dir", "pdb:korf+sym", "--weight", "1",
                                                      "--semantics", "cpp", "--batch_size", "1000", "--results_dir", d,
                                                      "--max_nodes", str(1 << 24)])),
                      ("idastar", lambda d: idastar.main(["--states", spath, "--env", "cube3", "--model_dir", "pdb:korf+sym:8",
                                                          "--results_dir", d, "--verbose"]))):
        rdir = str(tmp_path / name)
        try:
            run(rdir)
        finally:
            sys.stdout = sys.__stdout__
        res = data_utils.load_pickle(os.path.join(rdir, "results.pkl"))
        assert [len(s) for s in res["solutions"]] == [10], name
        assert np.array_equal(ida.replay_cube3(root, res["solutions"][0]), np.arange(54))
        log = open(os.path.join(rdir, "output.txt")).read()
        assert ("e6,e7,e8,e9,e10,e11%s: 349695360 bytes" % ("+sym" if name == "astar" else "+sym:8")) in log, log
