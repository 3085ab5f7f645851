"""GPU: the dual look-ups for the cube3 pattern databases (dca_cube3_pdb_eval_dual, dca_idastar_cube3_dual, `pdb:<spec>+dual`).
Integer arithmetic throughout, so every comparison is exact: the eval kernel against its host twin (which
tests/test_cube3_dual_cpu.py checks against the symmetric value at the row and at its inverse, and against the replacing rule on
any bytes), the kernel's IDA* against the same frame run on the host, and the search with +dual against the one without."""
import ctypes as C

import numpy as np
import pytest
import torch

from tests import test_cube3_dual_cpu as dual
from tests import test_cube3_pdb_cpu as c3
from tests import test_cube3_sym_cpu as sym
from tests import test_idastar_cpu as ida

pytestmark = pytest.mark.gpu

BIG = 1 << 40
ALL = sym.ALL
SMALL4 = dual.SMALL4
KORF_SHAPED = (c3.SMALL["c4,c5,c6,c7"], c3.SMALL["e0,e1,e2,e3"], c3.SMALL["e8,e9,e10,e11"])  # a corner table and two edge tables


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
def eval_rows():
    """1025 rows, cube states and the any-bytes rows of the CPU test alternating, so that every prefix holds both."""
    states, junk = dual.rule_rows(), dual.any_rows()
    rows = np.empty((1025, 54), np.uint8)
    rows[0::2] = states[:513]
    rows[1::2] = junk[:512]
    rows.setflags(write=False)
    return rows


# ------------------------------------------------------------------------------------------------ 1. eval
@pytest.mark.parametrize("row_kind", [c3.ROWS_STATE, c3.ROWS_NNET])
@pytest.mark.parametrize("n_images", [1, 2, ALL])
def test_eval_kernel_equals_the_host_twin(L, eval_rows, n_images, row_kind):
    patterns = dual.ANY_SETS[2] + (c3.SMALL["e8,e9,e10,e11"],)  # corners and edges, the all-corner pattern in the middle
    host = dual.any_tables(patterns[:3]) + [c3.host_table(*patterns[3])]
    tables = [dev(t) for t in host]
    rows = eval_rows if row_kind == c3.ROWS_STATE else np.where(eval_rows < 54, eval_rows // 9, eval_rows).astype(np.uint8)
    want = L.cube3_pdb_eval_host(rows, row_kind, patterns, host, sym=n_images, dual=True)
    assert (want > L.cube3_pdb_eval_host(rows, row_kind, patterns, host, sym=n_images)).any()  # the second pass matters here
    for ld in (54, 57, 64):
        for offset in (1, 0):  # an odd base: the byte-load kernel; base and ld multiples of 4: the word-load kernel
            flat = torch.full((len(rows) * ld + 8,), 0xA5, dtype=torch.uint8, device="cuda")
            for n in (0, 1, 63, 64, 65, 1025):
                view = flat[offset:offset + n * ld].view(n, ld)[:, :54]
                view.copy_(dev(rows[:n]))
                got = L.cube3_pdb_eval(view, row_kind, patterns, tables, sym=n_images, dual=True)
                assert got.dtype == torch.float32 and got.shape == (n,)
                assert torch.equal(got.cpu(), torch.from_numpy(want[:n])), (n_images, row_kind, ld, offset, n)


def test_eval_through_the_class_and_its_refusals(L):
    from deepcubea_amd.utils.cube3_pdb import Cube3PatternDatabase
    host = sym.tables_of(SMALL4)
    tables = [dev(t) for t in host]
    states = dual.rule_rows()
    want = L.cube3_pdb_eval_host(states, c3.ROWS_STATE, SMALL4, host, sym=8, dual=True)
    pdb = Cube3PatternDatabase(SMALL4, sym=8, dual=True).set_tables(host)
    assert pdb.spec.endswith("+sym:8+dual") and pdb.bytes == sum(t.size for t in host)
    assert np.array_equal(pdb.heuristic(dev(states)).cpu().numpy(), want)
    assert np.array_equal(pdb.heuristic_fn_dev()(dev(states // 9)).cpu().numpy(), want)  # the closure: colour rows
    plain_dual = Cube3PatternDatabase(SMALL4, dual=True).set_tables(host)  # no +sym: max_images = 1
    assert np.array_equal(plain_dual.heuristic(dev(states)).cpu().numpy(), L.cube3_pdb_eval_host(states, c3.ROWS_STATE, SMALL4, host, sym=1, dual=True))
    # the refusals of the symmetric eval
    rows = dev(c3.scrambles(8, 10, 1))
    for bad in (-1, 49):
        with pytest.raises(L.DcaError, match="max_images"):
            L.cube3_pdb_eval(rows, c3.ROWS_STATE, SMALL4, tables, sym=bad, dual=True)
    three = (c3.SMALL["c0,c1,c2"], (c3.CORNERS, (5, 6, 7)), (c3.CORNERS, (1, 2, 4)))  # 72 list entries
    with pytest.raises(L.DcaError, match=r"DCA_CUBE3_SYM_MAX_LOOKUPS = 64.*\+sym:N"):
        L.cube3_pdb_eval(rows, c3.ROWS_STATE, three, [tables[0]] * 3, sym=ALL, dual=True)
    assert L.cube3_pdb_eval(rows, c3.ROWS_STATE, three, [tables[0]] * 3, sym=21, dual=True).shape == (8,)
    with pytest.raises(ValueError):
        L.cube3_pdb_eval(rows, c3.ROWS_STATE, SMALL4, tables[:3] + [tables[3][:-1]], sym=ALL, dual=True)
    with pytest.raises(L.DcaError, match="ld"):
        L.cube3_pdb_eval(rows[:, :50], c3.ROWS_STATE, SMALL4, tables, sym=ALL, dual=True)
    # and NULLs, before any device work: the raw entry point
    kinds, ids, ks = np.array([0], np.int32), np.array([0, 1, 2], np.uint8), np.array([3], np.int32)
    ptrs = (C.c_void_p * 1)(tables[0].data_ptr())
    out = torch.full((8,), -3.0, device="cuda")
    good = dict(states=rows.data_ptr(), kinds=kinds.ctypes.data, ids=ids.ctypes.data, ks=ks.ctypes.data, ptrs=ptrs, out=out.data_ptr())
    for null in ("states", "kinds", "ids", "ks", "ptrs", "out"):
        a = dict(good, **{null: None})
        rc = L.lib().dca_cube3_pdb_eval_dual(a["states"], 8, 54, 0, 1, a["kinds"], a["ids"], a["ks"], a["ptrs"], ALL, a["out"], None)
        assert rc == -1 and L.lib().dca_last_error().startswith(b"bad argument: dca_cube3_pdb_eval_dual"), null
    torch.cuda.synchronize()
    assert bool((out == -3.0).all())


# ------------------------------------------------------------------------------------------------ 2. IDA* against the host frame
@pytest.mark.parametrize("depth", [-1, 0, 2, 3])
@pytest.mark.parametrize("case", dual.IDA_CASES, ids=lambda c: "root%d-%d" % c)
def test_kernel_idastar_equals_the_host_frame(L, prefix, case, depth):
    root = ida.cube3_suffix_root(*case)
    host = sym.tables_of(dual.IDA_SET)
    tables = [dev(t) for t in host]
    prefix(depth)
    for n in (ALL, 2, 0):
        want = L.idastar_host(L.ENV_CUBE3, 0, root, dual.IDA_SET, host, BIG, sym=n, dual=True)
        got = L.idastar_cube3(root, dual.IDA_SET, tables, BIG, sym=n, dual=True)
        assert got["solved"] and len(got["moves"]) == case[1] == len(want["moves"])
        assert np.array_equal(ida.replay_cube3(root, got["moves"]), np.arange(54))
        assert got["thresholds"] == want["thresholds"] and got["nodes_per_threshold"][:-1] == want["nodes_per_threshold"][:-1]
        assert got["nodes_generated"] == sum(got["nodes_per_threshold"])


# ------------------------------------------------------------------------------------------------ 3. a deeper root
def test_a_deeper_root_with_and_without_dual(L):
    from deepcubea_amd.search_methods.idastar import IDAStar
    from deepcubea_amd.utils.cube3_pdb import Cube3PatternDatabase
    host = sym.tables_of(KORF_SHAPED)
    k = 10
    root = ida.cube3_suffix_root(1, k)
    runs = {}
    for is_dual in (False, True):
        pdb = Cube3PatternDatabase(KORF_SHAPED, sym=8, dual=is_dual).set_tables(host)
        assert pdb.spec.endswith("+sym:8+dual" if is_dual else "+sym:8")
        res = IDAStar("cube3", pdb).solve(root, BIG)
        print("%s: thresholds %s nodes %s" % (pdb.spec, res["thresholds"], res["nodes_per_threshold"]))
        assert res["solved"] and len(res["moves"]) == k == res["path_cost"]
        assert np.array_equal(ida.replay_cube3(root, res["moves"]), np.arange(54))
        assert all(a < b for a, b in zip(res["thresholds"], res["thresholds"][1:])) and res["thresholds"][-1] == k
        runs[is_dual] = res
    with_dual, without = runs[True], runs[False]
    assert with_dual["thresholds"][0] >= without["thresholds"][0]
    shared = [T for T in with_dual["thresholds"][:-1] if T in without["thresholds"][:-1]]
    assert shared
    for T in shared:
        a = with_dual["nodes_per_threshold"][with_dual["thresholds"].index(T)]
        b = without["nodes_per_threshold"][without["thresholds"].index(T)]
        assert a <= b, (T, a, b)


# ------------------------------------------------------------------------------------------------ 4. dead root, budget
def test_a_root_that_only_a_dual_byte_kills_and_the_budget(L):
    case = (2, 7)
    root = ida.cube3_suffix_root(*case)
    host = sym.tables_of(dual.IDA_SET)
    reads = dual.root_reads(root, ALL)
    regular = {(p, idx) for p, idx, second in reads if not second}
    p, idx = [(p, idx) for p, idx, second in reads if second and (p, idx) not in regular][0]
    dead = [t.copy() for t in host]
    dead[p][idx] = 0xFE
    tables = [dev(t) for t in dead]
    res = L.idastar_cube3(root, dual.IDA_SET, tables, BIG, sym=ALL, dual=True)
    assert res["status"] == "unsolvable" and not res["solved"] and res["thresholds"] == [] and res["moves"] == []
    alive = L.idastar_cube3(root, dual.IDA_SET, tables, BIG, sym=ALL)
    assert alive["solved"] and len(alive["moves"]) == 7
    # the budget, on a root deep enough to fill the lanes
    tables = [dev(t) for t in sym.tables_of(KORF_SHAPED)]
    k = 12
    deep = ida.cube3_suffix_root(0, k)
    full = L.idastar_cube3(deep, KORF_SHAPED, tables, BIG, sym=8, dual=True)
    print("thresholds %s nodes %s" % (full["thresholds"], full["nodes_per_threshold"]))
    assert full["solved"] and len(full["moves"]) == k and sum(full["nodes_per_threshold"][:-1]) > 1000
    for max_nodes in (1, 1000):  # budgets that end before the last threshold starts
        res = L.idastar_cube3(deep, KORF_SHAPED, tables, max_nodes, sym=8, dual=True)
        assert res["status"] == "budget exhausted" and not res["solved"] and res["moves"] == [] and res["path_cost"] == float("inf")
        assert res["nodes_generated"] == sum(res["nodes_per_threshold"]) and res["thresholds"][-1] < k
        assert max_nodes <= res["nodes_generated"] <= max_nodes + max(max_nodes // 2, L.IDASTAR_MAX_LANES)  # the header's bounds
        assert res["nodes_generated"] <= max_nodes + L.IDASTAR_OVERSHOOT
    bad = np.arange(54, dtype=np.uint8)
    bad[[0, 10, 8, 12]] = bad[[10, 0, 12, 8]]
    with pytest.raises(L.DcaError, match="root: .*no cube state"):
        L.idastar_cube3(bad, KORF_SHAPED, tables, 1000, sym=8, dual=True)
    with pytest.raises(ValueError, match="uint8 device tensor"):  # a host address must never reach the kernel's gathers
        L.idastar_cube3(deep, SMALL4, sym.tables_of(SMALL4), 1000, sym=ALL, dual=True)


# ------------------------------------------------------------------------------------------------ 5. the engine's closure
def test_engine_with_the_dual_closure_returns_valid_solutions(L):
    from deepcubea_amd.search_methods import astar
    from deepcubea_amd.search_methods.engine import BwasEngine
    from types import SimpleNamespace
    spec = "c0,c1,c2/c4,c5,c6,c7/e0,e1,e2,e3/e8,e9,e10,e11+dual"
    pdb = astar._pattern_database(SimpleNamespace(model_dir="pdb:" + spec, env="cube3"))
    assert pdb.dual and pdb.spec == spec and pdb.patterns == SMALL4
    pdb.set_tables(sym.tables_of(SMALL4))
    fn = pdb.heuristic_fn_dev()
    k = 6
    root = ida.cube3_suffix_root(3, k)  # six moves from the goal on a shipped optimal path: the optimal length is 6
    assert float(fn(dev(root[None] // 9))[0]) <= k
    for semantics, batch in ((L.SEM_PY, 1), (L.SEM_CPP, 1000)):
        eng = BwasEngine("cube3", 1.0, batch, semantics=semantics)
        res = eng.solve(root, fn, max_iters=200000)
        eng.close()
        print("semantics %s, batch %d: length %d, nodes generated %d" % (semantics, batch, len(res["moves"]), res["nodes_generated"]))
        assert res["solved"] and np.array_equal(ida.replay_cube3(root, res["moves"]), np.arange(54))
        assert len(res["moves"]) >= k
        if semantics == L.SEM_PY:
            assert len(res["moves"]) == k
