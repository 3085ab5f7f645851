"""GPU: the cube3 pattern databases (dca_cube3_pdb_build / dca_cube3_pdb_eval, utils/cube3_pdb.py, `--env cube3 --model_dir
pdb:<spec>`).  Everything is integer arithmetic, so every comparison is exact: built tables byte for byte against the host
reference of tests/test_cube3_pdb_cpu.py (a breadth-first search written from the header's rules), evaluation against the host
gather on the 21 637 states of the shipped optimal paths, whose exact distances bound every table from above."""
import ctypes as C
import os
import sys

import numpy as np
import pytest
import torch

from tests import test_cube3_pdb_cpu as ref

pytestmark = pytest.mark.gpu

CORNERS, EDGES = ref.CORNERS, ref.EDGES
SMALL4 = tuple(ref.SMALL.values())
BUILD_PATTERNS = {"c0": (CORNERS, (0,)), "e5": (EDGES, (5,)), "e11,e0": (EDGES, (11, 0)), **ref.SMALL}
ENGINE_SPEC = "c0,c1,c2,c3/c4,c5,c6,c7/e0,e1,e2,e3/e8,e9,e10,e11"
CORNERS8 = (CORNERS, tuple(range(8)))


@pytest.fixture(scope="module")
def L():
    from deepcubea_amd import _lib
    _lib.require_gpu()
    return _lib


def dev(a):
    a = np.ascontiguousarray(a)
    return torch.from_numpy(a if a.flags.writeable else a.copy()).cuda()  # (the host reference's arrays are read-only)


@pytest.fixture(scope="module")
def paths():
    """(sticker-id rows, colour rows, remaining distance, is_last) of the shipped optimal paths, on the host."""
    states, dist, last = ref.path_states()
    return states, states // 9, dist, last


@pytest.fixture(scope="module")
def small(L):
    """The four small patterns: (patterns, host tables, device tables, exact host values on the path states)."""
    host = [ref.host_table(*p) for p in SMALL4]
    want = ref.host_eval(ref.path_states()[0], ref.ROWS_STATE, SMALL4, host)
    want.setflags(write=False)
    return SMALL4, host, [dev(t) for t in host], want


@pytest.fixture(scope="module")
def engine_pdb(L):
    from deepcubea_amd.utils.cube3_pdb import Cube3PatternDatabase
    return Cube3PatternDatabase(ENGINE_SPEC).build()


def rows_of(paths, row_kind):
    return paths[0] if row_kind == ref.ROWS_STATE else paths[1]


# ------------------------------------------------------------------------------------------------ 1. build
@pytest.mark.parametrize("name", list(BUILD_PATTERNS))
def test_build_byte_for_byte_against_the_host_reference(L, name):
    kind, cubies = BUILD_PATTERNS[name]
    want = ref.host_table(kind, cubies)
    table, sweeps = L.cube3_pdb_build(kind, cubies)
    got = table.cpu().numpy()
    assert got.shape == want.shape == (L.cube3_pdb_bytes(kind, len(cubies)),)
    assert np.array_equal(got, want), (name, int((got != want).sum()))
    assert sweeps == int(want.max()) + 1  # the deepest level + 1: the last, empty sweep included
    again, sweeps2 = L.cube3_pdb_build(kind, cubies)  # built twice: the same bytes, the same count
    assert torch.equal(table, again) and sweeps2 == sweeps


def test_one_large_build_is_admissible_and_consistent_on_the_paths(L, paths):
    kind, cubies = EDGES, (0, 1, 2, 3, 4, 5)
    table, sweeps = L.cube3_pdb_build(kind, cubies)
    assert table.numel() == 42577920 == ref.table_size(kind, 6)
    hist = torch.bincount(table.to(torch.int64), minlength=256).cpu().numpy()
    assert hist[0] == 1 and hist[ref.UNREACHED] == 0 and hist[0xFF] == 0 and hist.sum() == 42577920  # six edges: all reachable
    deepest = int(np.nonzero(hist)[0].max())
    assert deepest < ref.UNREACHED and sweeps == deepest + 1 and (hist[:deepest + 1] > 0).all()
    goal = ref.rank_locations(kind, np.array([[2 * c for c in cubies]]))[0]
    assert int(table[goal]) == 0
    states, colours, dist, last = paths
    h = L.cube3_pdb_eval(dev(colours), L.ROWS_NNET, [(kind, cubies)], [table]).cpu().numpy().astype(np.int64)
    assert np.array_equal(h, L.cube3_pdb_eval(dev(states), L.ROWS_STATE, [(kind, cubies)], [table]).cpu().numpy())
    assert np.array_equal(h, table.cpu().numpy()[ref.host_index(kind, cubies, states, ref.ROWS_STATE)])
    assert (h <= dist).all() and (h[dist == 0] == 0).all()
    assert np.abs(h[1:] - h[:-1])[~last[:-1]].max() <= 1


# ------------------------------------------------------------------------------------------------ 2. eval
@pytest.mark.parametrize("row_kind", [ref.ROWS_STATE, ref.ROWS_NNET])
def test_eval_against_the_host_gather_on_the_path_states(L, paths, small, row_kind):
    patterns, host, tables, want = small
    X = rows_of(paths, row_kind)
    got = L.cube3_pdb_eval(dev(X), row_kind, patterns, tables).cpu().numpy()
    assert np.array_equal(got, want)
    assert (got <= paths[2]).all() and int((got == paths[2]).sum()) == 6258


@pytest.mark.parametrize("row_kind", [ref.ROWS_STATE, ref.ROWS_NNET])
def test_eval_shapes_strides_offsets_and_guards(L, paths, small, row_kind):
    patterns, host, tables, want_all = small
    X_all = rows_of(paths, row_kind)
    for n in (0, 1, 255, 257, 4099):
        lo = 3000  # a stretch that spans many paths
        X, want = X_all[lo:lo + n], want_all[lo:lo + n]
        for ld in (54, 55, 56, 64):
            buf = torch.full((max(n, 1), ld), 0xA5, dtype=torch.uint8, device="cuda")
            view = buf[:n, :54]
            view.copy_(dev(X))
            out = torch.full((n + 16,), -1.0, dtype=torch.float32, device="cuda")
            L.cube3_pdb_eval(view, row_kind, patterns, tables, out=out[8:8 + n] if n else out[8:8])
            assert np.array_equal(out[8:8 + n].cpu().numpy(), want), (n, ld)
            assert bool((out[:8] == -1.0).all()) and bool((out[8 + n:] == -1.0).all())  # no stray write
        if n == 0:
            continue
        off = torch.zeros(n * 54 + 1, dtype=torch.uint8, device="cuda")  # a base pointer off by one byte
        rows = off[1:].view(n, 54)
        rows.copy_(dev(X))
        assert rows.data_ptr() % 2 == 1 and np.array_equal(L.cube3_pdb_eval(rows, row_kind, patterns, tables).cpu().numpy(), want)
        wide = torch.full((2 * n, 128), 0x5A, dtype=torch.uint8, device="cuda")  # a strided view: every other row of a wider buffer
        view = wide[::2, 8:62]
        view.copy_(dev(X))
        assert np.array_equal(L.cube3_pdb_eval(view, row_kind, patterns, tables).cpu().numpy(), want)


@pytest.mark.parametrize("count", [1, 2, 5, 24])
def test_eval_pattern_counts_cover_the_gather_groups_tail(L, paths, count):
    cycle = list(BUILD_PATTERNS.values())
    patterns = [cycle[(3 * i) % len(cycle)] for i in range(count)]  # patterns may repeat and share cubies
    host = [ref.host_table(*p) for p in patterns]
    X = paths[1][5000:5000 + 1500]
    got = L.cube3_pdb_eval(dev(X), L.ROWS_NNET, patterns, [dev(t) for t in host]).cpu().numpy()
    assert np.array_equal(got, ref.host_eval(X, ref.ROWS_NNET, patterns, host))


def test_any_bytes_stay_in_bounds(L, paths, small):
    from deepcubea_amd.utils.cube3_pdb import Cube3PatternDatabase
    patterns, host, tables, want = small
    rng = np.random.default_rng(11)
    junk = np.concatenate([rng.integers(0, 256, (4096, 54), dtype=np.uint8), np.zeros((1, 54), np.uint8), np.full((1, 54), 0xFF, np.uint8),
                           rng.integers(0, 54, (512, 54), dtype=np.uint8), rng.integers(0, 6, (512, 54), dtype=np.uint8)])
    wide = (CORNERS8, (EDGES, (3, 9, 0, 5, 1))) + tuple(patterns)
    zeros = [np.zeros(ref.table_size(CORNERS, 8), np.uint8), np.full(ref.table_size(EDGES, 5), 7, np.uint8)]
    pdb = Cube3PatternDatabase(wide).set_tables(zeros + host)  # the widest rank through a host-made table: no long build
    for row_kind in (L.ROWS_STATE, L.ROWS_NNET):
        got = pdb.heuristic(dev(junk), row_kind)
        torch.cuda.synchronize()
        got = got.cpu().numpy()
        assert got.shape == (len(junk),) and (got >= 7).all() and (got <= 255).all() and (got == np.floor(got)).all()
        X = rows_of(paths, row_kind)[:4099]
        after = L.cube3_pdb_eval(dev(X), row_kind, patterns, tables).cpu().numpy()  # a following valid launch is still exact
        assert np.array_equal(after, want[:4099])


# ------------------------------------------------------------------------------------------------ 3. refusals
def test_refusals_through_the_c_abi_launch_nothing(L, paths):
    lib = L.lib()
    table = torch.full((9072,), 0x5A, dtype=torch.uint8, device="cuda")
    states = dev(paths[0][:64])
    outbuf = torch.full((66,), -1.0, dtype=torch.float32, device="cuda")
    out = outbuf[1:65]
    p, s = lambda t: C.c_void_p(t.data_ptr()), L.stream_ptr()

    def build(kind=0, cubies=(0, 1, 2), k=None, tab=p(table)):
        c = np.array(cubies, np.uint8)
        return lib.dca_cube3_pdb_build(kind, c.ctypes.data_as(C.c_void_p), len(cubies) if k is None else k, tab, None, s)

    def evaluate(groups=((0, (0, 1, 2)),), ld=54, row_kind=0, tabs=None, np_=None, o=None, n=64):
        kinds = np.array([kind for kind, _ in groups], np.int32)
        c = np.array([x for _, g in groups for x in g], np.uint8)
        ks = np.array([len(g) for _, g in groups], np.int32)
        ptrs = (C.c_void_p * max(len(groups), 1))(*([table.data_ptr()] * len(groups) if tabs is None else tabs))
        return lib.dca_cube3_pdb_eval(p(states), n, ld, row_kind, len(groups) if np_ is None else np_, kinds.ctypes.data_as(C.c_void_p),
                                      c.ctypes.data_as(C.c_void_p), ks.ctypes.data_as(C.c_void_p), ptrs, p(out) if o is None else o, s)

    cases = {"bad kind": (lambda: build(kind=2), b"kind"), "k = 0": (lambda: build(k=0), b"k = 0"),
             "k = 9": (lambda: build(kind=1, cubies=tuple(range(9))), b"k = 9"),
             "cubie >= n": (lambda: build(cubies=(0, 8)), b"cubie 8"), "edge >= n": (lambda: build(kind=1, cubies=(12,)), b"cubie 12"),
             "a cubie twice": (lambda: build(cubies=(2, 1, 2)), b"cubie 2 appears twice"),
             "a null table": (lambda: build(tab=None), b"table"),
             "eval bad kind": (lambda: evaluate(groups=((-1, (0,)),)), b"kind"), "eval k = 0": (lambda: evaluate(groups=((0, (1,)), (1, ()))), b"k = 0"),
             "eval k = 9": (lambda: evaluate(groups=((1, tuple(range(9))),)), b"k = 9"),
             "eval cubie >= n": (lambda: evaluate(groups=((0, (8,)),)), b"cubie 8"),
             "eval a cubie twice": (lambda: evaluate(groups=((1, (4, 4)),)), b"cubie 4 appears twice"),
             "a null table in the set": (lambda: evaluate(groups=((0, (0, 1, 2)), (0, (3,))), tabs=[table.data_ptr(), 0]), b"table 1 is NULL"),
             "25 patterns": (lambda: evaluate(groups=((1, (0,)),) * 25), b"num_patterns"),
             "no patterns": (lambda: evaluate(groups=(), np_=0), b"num_patterns"),
             "ld < 54": (lambda: evaluate(ld=53), b"ld"), "bad row_kind": (lambda: evaluate(row_kind=2), b"row_kind"),
             "negative n": (lambda: evaluate(n=-1), b"n >= 0"), "a null out": (lambda: evaluate(o=C.c_void_p(0)), b"out"),
             "misaligned out": (lambda: evaluate(o=C.c_void_p(out.data_ptr() + 2)), b"out")}
    for what, (fn, word) in cases.items():
        assert fn() == -1, what
        msg = lib.dca_last_error()
        assert msg.startswith(b"bad argument: dca_cube3_pdb_") and word in msg, (what, msg)
    torch.cuda.synchronize()
    assert bool((table == 0x5A).all()) and bool((outbuf == -1.0).all()), "a refused call launches nothing"
    assert build() == 0 and evaluate(groups=((0, (0, 1, 2)), (0, (2, 1, 0)))) == 0  # patterns may share cubies
    torch.cuda.synchronize()
    assert np.array_equal(table.cpu().numpy(), ref.host_table(0, (0, 1, 2))) and bool((out >= 0).all())
    assert float(outbuf[0]) == -1.0 and float(outbuf[65]) == -1.0


# ------------------------------------------------------------------------------------------------ 4. search
def path_roots(paths, distances, instances=3):
    """The shipped-path states at the given remaining distances of the first `instances` shipped instances."""
    states, _, dist, last = paths
    ends = np.nonzero(last)[0][:instances]  # row of each path's goal end: the state at remaining distance d is d rows before it
    return [(states[e - d].copy(), d) for e in ends for d in distances]


def replay(co, root, moves):
    s = root[None].copy()
    for a in moves:
        s = co.next_state("cube3", s, a)
    return bool(co.is_solved("cube3", s)[0])


def test_engine_with_the_pdb_closure_is_optimal_and_prunes(L, paths, engine_pdb):
    from deepcubea_amd.search_methods.engine import BwasEngine
    from oracle import c_oracle as co
    assert engine_pdb.bytes == 2 * 136080 + 2 * 190080 and engine_pdb.spec == ENGINE_SPEC
    fn = engine_pdb.heuristic_fn_dev()
    eng = BwasEngine("cube3", 1.0, 1000, semantics=L.SEM_CPP)
    for root, d in path_roots(paths, (3, 4, 5, 6)):
        assert float(fn(dev(root[None] // 9))[0]) <= d
        res = eng.solve(root, fn, max_iters=20000)
        assert res["solved"], (d, res)
        print("distance %d: closure length %d, nodes generated %d" % (d, len(res["moves"]), res["nodes_generated"]))
        assert len(res["moves"]) == d and replay(co, root, res["moves"]), (d, res["moves"])
        if d <= 5:
            zero = eng.solve_builtin(root, L.HEUR_ZERO)
            print("distance %d: zero-heuristic length %d, nodes generated %d" % (d, len(zero["moves"]), zero["nodes_generated"]))
            assert zero["solved"] and len(zero["moves"]) == d
            assert res["nodes_generated"] <= zero["nodes_generated"], (d, res["nodes_generated"], zero["nodes_generated"])
    eng.close()


def test_astar_cli_pdb_model_on_cube3(tmp_path, L, paths):
    from deepcubea_amd.environments.cube3 import Cube3State
    from deepcubea_amd.search_methods import astar
    from deepcubea_amd.utils import data_utils
    from oracle import c_oracle as co
    roots = path_roots(paths, (5,))
    spath = str(tmp_path / "states.pkl")
    data_utils.dump_pickle({"states": [Cube3State(r.copy()) for r, _ in roots]}, spath)
    rdir = str(tmp_path / "pdb")
    try:
        astar.main(["--states", spath, "--env", "cube3", "--model_dir", "pdb:" + ENGINE_SPEC, "--weight", "1", "--semantics", "cpp",
                    "--batch_size", "1000", "--results_dir", rdir, "--max_nodes", str(1 << 24)])
    finally:
        sys.stdout = sys.__stdout__
    res = data_utils.load_pickle(os.path.join(rdir, "results.pkl"))
    assert sorted(res.keys()) == ["num_nodes_generated", "paths", "solutions", "states", "times"]  # astar.py:382-397
    assert [len(s) for s in res["solutions"]] == [d for _, d in roots] == [5, 5, 5]
    for (root, _), soln, path in zip(roots, res["solutions"], res["paths"]):
        assert replay(co, root, soln) and len(path) == len(soln) + 1
    log = open(os.path.join(rdir, "output.txt")).read()
    assert "pattern database %s: 652320 bytes, sweeps [" % ENGINE_SPEC in log
    for model in ("pdb:auto", "pdb:c0,e1"):
        try:
            with pytest.raises(ValueError):
                astar.main(["--states", spath, "--env", "cube3", "--model_dir", model, "--weight", "1", "--semantics", "cpp",
                            "--results_dir", str(tmp_path / "bad")])
        finally:
            sys.stdout = sys.__stdout__


def test_save_load_on_the_device(tmp_path, L, paths):
    from deepcubea_amd.utils.cube3_pdb import Cube3PatternDatabase
    pdb = Cube3PatternDatabase("c0,c1,c2/e11,e0").build()
    assert pdb.sweeps == [int(ref.host_table(CORNERS, (0, 1, 2)).max()) + 1, int(ref.host_table(EDGES, (11, 0)).max()) + 1]
    path = str(tmp_path / "c3.npz")
    pdb.save(path)
    back = Cube3PatternDatabase.load(path)
    assert back.patterns == ((CORNERS, (0, 1, 2)), (EDGES, (11, 0))) and all(torch.equal(a, b) for a, b in zip(pdb.tables, back.tables))
    X = dev(paths[1][:1000])
    assert torch.equal(pdb.heuristic(X, L.ROWS_NNET), back.heuristic_fn_dev()(X))
    assert torch.equal(pdb.heuristic(dev(paths[0][:1000])), back.heuristic_fn_dev()(X))  # sticker-id rows: the default reading
    with pytest.raises(ValueError):
        back.heuristic_fn_dev()(X, True)
    with pytest.raises(L.DcaError):
        Cube3PatternDatabase("c0").heuristic(X)  # never built
