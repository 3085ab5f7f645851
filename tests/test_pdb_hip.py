"""GPU: the pattern databases (dca_pdb_build / dca_pdb_eval, utils/pattern_db.py, `--model_dir pdb:<spec>`).  Everything is
integer arithmetic, so every comparison is exact: built tables byte for byte against the host reference of
tests/test_pdb_cpu.py (a 0-1 breadth-first search written from the header's rules), evaluation against the host gather, and on
all 181 440 puzzle8 states against the breadth-first distance table of tests/test_puzzle8_cpu.py."""
import ctypes as C
import os
import sys

import numpy as np
import pytest
import torch

from tests import test_pdb_cpu as ref
from tests import test_puzzle8_cpu as p8

pytestmark = pytest.mark.gpu

P8_44 = ((1, 2, 3, 4), (5, 6, 7, 8))
P8_35 = ((1, 2, 3), (4, 5, 6, 7, 8))
P8_ONES = tuple((t,) for t in range(1, 9))
P15_33 = ((1, 2, 5), (12, 15, 14))
P24_2 = ((7, 24),)
P48_2 = ((20, 48),)
P35_2 = ((8, 35),)
P24_TRIPLES = tuple((a, a + 1, a + 2) for a in range(1, 25, 3))
SHAPE_SETS = {9: (3, P8_44), 16: (4, P15_33), 25: (5, P24_2), 36: (6, P35_2), 49: (7, P48_2)}


@pytest.fixture(scope="module")
def L():
    from deepcubea_amd import _lib
    _lib.require_gpu()
    return _lib


@pytest.fixture(scope="module")
def table8():
    """(all 181 440 puzzle8 states in breadth-first order, their exact distances) — computed once, never written to."""
    states, d, _ = p8.bfs_table()
    return states, d.astype(np.int64)


@pytest.fixture(scope="module")
def pdb555(L):
    from deepcubea_amd.utils.pattern_db import PatternDatabase
    return PatternDatabase("puzzle15", "5-5-5").build()


def dev(a):
    a = np.ascontiguousarray(a)
    return torch.from_numpy(a if a.flags.writeable else a.copy()).cuda()  # (the host reference's tables are read-only)


def built(L, dim, partition):
    return [L.pdb_build(dim, g) for g in partition]


def perms(n, D, seed):
    rng = np.random.default_rng(seed)
    return rng.permuted(np.tile(np.arange(D, dtype=np.uint8), (n, 1)), axis=1)


# ------------------------------------------------------------------------------------------------ 1. build
@pytest.mark.parametrize("dim,partition,entries,valid", [
    (3, P8_44, 59049, 15120), (3, P8_35, 531441, 60480), (4, P15_33, 65536, 43680), (5, P24_2, 15625, 13800), (7, P48_2, 117649, 110544),
    (6, P35_2, 46656, 42840)])
def test_build_byte_for_byte_against_the_host_reference(L, dim, partition, entries, valid):
    tables = built(L, dim, partition)
    torch.cuda.synchronize()
    assert max(t.numel() for t, _ in tables) == entries == max(L.pdb_bytes(dim, len(g)) for g in partition)
    for group, (table, sweeps) in zip(partition, tables):
        want = ref.host_table(dim, group)
        got = table.cpu().numpy()
        assert got.shape == want.shape and np.array_equal(got, want), (group, int((got != want).sum()))  # 0xFF entries included
        assert 1 < sweeps < 1000
    got = tables[-1][0].cpu().numpy()
    assert int((got != ref.NO_STATE).sum()) == valid and int((got == ref.UNREACHABLE).sum()) == 0
    again = built(L, dim, partition)  # built twice: the same bytes
    assert all(torch.equal(a[0], b[0]) for a, b in zip(tables, again))


# ------------------------------------------------------------------------------------------------ 2. all puzzle8 states
@pytest.mark.parametrize("partition", [P8_44, P8_35])
def test_all_puzzle8_states_admissible_consistent_and_above_manhattan(L, table8, partition):
    X, dist = table8
    tables = [t for t, _ in built(L, 3, partition)]
    dX = dev(X)
    h = L.pdb_eval(3, dX, partition, tables).cpu().numpy()
    assert np.array_equal(h, ref.host_eval(3, X, partition, [ref.host_table(3, g) for g in partition]))
    mh = p8.manhattan_np(X)
    assert (mh <= h).all() and (h <= dist).all() and h[0] == 0 and dist[0] == 0 and ((h == 0) == (dist == 0)).all()
    ch = L.expand_fused(L.ENV_NPUZZLE, 3, dX, solved=False, hashes=False)["children"].view(-1, 9)  # every move of every state
    hc = L.pdb_eval(3, ch, partition, tables).cpu().numpy().reshape(-1, 4)
    assert (np.abs(hc - h[:, None]) <= 1).all()
    if partition == P8_44:  # more rows than one pass of the capped grid holds: the row loop's second trip
        big = dX.repeat(24, 1)
        assert big.shape[0] > (1 << 14) * 256
        assert np.array_equal(L.pdb_eval(3, big, partition, tables).cpu().numpy(), np.tile(h, 24))


def test_one_tile_patterns_sum_to_the_builtin_manhattan_distance(L, table8):
    X, _ = table8
    tables = [t for t, _ in built(L, 3, P8_ONES)]
    dX = dev(X)
    h = L.pdb_eval(3, dX, P8_ONES, tables)
    assert torch.equal(h, L.heuristic_builtin(L.HEUR_MANHATTAN, dX))
    assert np.array_equal(h.cpu().numpy(), p8.manhattan_np(X).astype(np.float32))


def test_the_eight_tile_pattern_is_the_exact_distance(L, table8):
    """One pattern of all 8 tiles: a table of 9^9 = 387 MB whose states are the 9! placements; half of them cannot reach the goal."""
    X, dist = table8
    everything = (tuple(range(1, 9)),)
    table, sweeps = L.pdb_build(3, everything[0])
    assert table.numel() == 9 ** 9 == 387420489
    h = L.pdb_eval(3, dev(X), everything, [table]).cpu().numpy()
    assert np.array_equal(h, dist.astype(np.float32))
    assert int((table == ref.UNREACHABLE).sum()) == 181440 and int((table < ref.UNREACHABLE).sum()) == 181440
    assert int((table == 31).sum()) == 2 and sweeps > 1  # the two deepest states


# ------------------------------------------------------------------------------------------------ 3. eval shapes, any bytes
@pytest.mark.parametrize("D", [9, 16, 25, 36, 49])
def test_eval_shapes_strides_and_any_bytes(L, D):
    dim, partition = SHAPE_SETS[D]
    host = [ref.host_table(dim, g) for g in partition]
    tables = [dev(t) for t in host]
    rng = np.random.default_rng(D)
    for n in (1, 63, 64, 65, 4099):
        X = perms(n, D, 100 * D + n)
        want = ref.host_eval(dim, X, partition, host)
        for ld in (D, D + 7):
            buf = torch.full((n, ld), 0xA5, dtype=torch.uint8, device="cuda")
            view = buf[:, :D]
            view.copy_(dev(X))
            out = torch.full((n + 8,), -1.0, dtype=torch.float32, device="cuda")
            L.pdb_eval(dim, view, partition, tables, out=out)
            assert np.array_equal(out[:n].cpu().numpy(), want), (D, n, ld)
            assert bool((out[n:] == -1.0).all())  # no stray write
        off = torch.zeros(n * D + 3, dtype=torch.uint8, device="cuda")  # a base pointer off every grid
        rows = off[3:].view(n, D)
        rows.copy_(dev(X))
        assert rows.data_ptr() % 2 == 1 and np.array_equal(L.pdb_eval(dim, rows, partition, tables).cpu().numpy(), want)
    # the any-bytes rule: rows that are no states — all zero, all 0xFF, random bytes, random bytes < N with repeats — give the
    # header's value (last position that holds the tile, 0 if none), and the run ends clean
    n = 1000
    junk = np.concatenate([np.zeros((2, D), np.uint8), np.full((2, D), 0xFF, np.uint8), rng.integers(0, 256, (n, D), dtype=np.uint8),
                           rng.integers(0, D, (n, D), dtype=np.uint8), rng.integers(D, 256, (3, D), dtype=np.uint8)])
    got = L.pdb_eval(dim, dev(junk), partition, tables)
    torch.cuda.synchronize()
    want = ref.host_eval(dim, junk, partition, host)
    assert np.array_equal(got.cpu().numpy(), want)
    # nothing found (no byte < N): every digit 0 -> entry 0 of every table, which is no state
    assert want[2] == want[3] == want[-1] == sum(int(t[0]) for t in host) == ref.NO_STATE * len(partition)
    assert L.pdb_eval(dim, dev(junk[:0]), partition, tables).shape == (0,)


# ------------------------------------------------------------------------------------------------ 4. real instances
def test_puzzle15_555_between_manhattan_and_the_shipped_optimal_lengths(L, golden, pdb555):
    X, opt = golden["puzzle15_test_states"], golden["puzzle15_test_opt_len"].astype(np.int64)
    assert X.shape == (500, 16) and pdb555.bytes == 3 * 16 ** 6 and [t.numel() for t in pdb555.tables] == [16 ** 6] * 3
    h = pdb555.heuristic(dev(X)).cpu().numpy()
    mh = ref.manhattan_np(4, X)
    assert np.array_equal(L.heuristic_builtin(L.HEUR_MANHATTAN, dev(X)).cpu().numpy(), mh.astype(np.float32))
    assert (mh <= h).all() and (h <= opt).all() and (h > mh).any()
    goal = np.array([list(range(1, 16)) + [0]], np.uint8)
    assert float(pdb555.heuristic(dev(goal))[0]) == 0.0


def test_puzzle24_triples_between_manhattan_and_the_shipped_optimal_lengths(L, golden):
    from deepcubea_amd.utils.pattern_db import PatternDatabase
    X, opt = golden["puzzle24_test_states"], golden["puzzle24_test_opt_len"].astype(np.int64)
    assert X.shape == (496, 25)
    pdb = PatternDatabase("puzzle24", P24_TRIPLES).build()
    assert [t.numel() for t in pdb.tables] == [390625] * 8
    h = pdb.heuristic(dev(X)).cpu().numpy()
    mh = ref.manhattan_np(5, X)
    assert (mh <= h).all() and (h <= opt).all() and (h > mh).any()


def test_save_load_on_the_device(tmp_path, L):
    from deepcubea_amd.utils.pattern_db import PatternDatabase
    pdb = PatternDatabase("puzzle8", "4-4").build()
    path = str(tmp_path / "p8_44.npz")
    pdb.save(path)
    back = PatternDatabase.load(path)
    assert back.partition == P8_44 and all(torch.equal(a, b) for a, b in zip(pdb.tables, back.tables))
    X = dev(perms(100, 9, 5))
    assert torch.equal(pdb.heuristic(X), back.heuristic_fn_dev()(X))
    with pytest.raises(ValueError):
        back.heuristic_fn_dev()(X, True)
    with pytest.raises(L.DcaError):
        PatternDatabase("puzzle8", "4-4").heuristic(X)  # never built


# ------------------------------------------------------------------------------------------------ 5. search
def _shortest(golden, count):
    opt = golden["puzzle15_test_opt_len"]
    return np.argsort(opt, kind="stable")[:count]  # the shortest instances of the set, as in tests/test_puzzle_optimal_hip.py


def test_engine_with_the_pdb_closure_finds_the_shipped_optimal_lengths(L, golden, pdb555):
    from deepcubea_amd.search_methods.engine import BwasEngine
    from oracle import c_oracle as co
    states, opt = golden["puzzle15_test_states"], golden["puzzle15_test_opt_len"]
    eng = BwasEngine("puzzle15", 1.0, 10000, max_nodes=1 << 26, semantics=L.SEM_CPP)
    fn = pdb555.heuristic_fn_dev()
    for i in _shortest(golden, 12):
        root = states[i]
        res = eng.solve(root, fn, max_iters=20000)
        assert res["solved"], (i, res)
        assert len(res["moves"]) == opt[i], (i, len(res["moves"]), opt[i], res["nodes_generated"])  # lengths, not node counts
        s = root[None].copy()
        for a in res["moves"]:
            s = co.next_state("puzzle15", s, a)
        assert co.is_solved("puzzle15", s)[0]
    eng.close()


# ------------------------------------------------------------------------------------------------ 6. command line
def test_astar_cli_pdb_model(tmp_path, L, golden):
    from deepcubea_amd.environments.n_puzzle import NPuzzleState
    from deepcubea_amd.search_methods import astar
    from deepcubea_amd.utils import data_utils
    from oracle import c_oracle as co
    states, opt = golden["puzzle15_test_states"], golden["puzzle15_test_opt_len"]
    pick = _shortest(golden, 3)
    spath = str(tmp_path / "states.pkl")
    data_utils.dump_pickle({"states": [NPuzzleState(states[i].copy()) for i in pick]}, spath)
    rdir = str(tmp_path / "pdb")
    try:
        astar.main(["--states", spath, "--env", "puzzle15", "--model_dir", "pdb:5-5-5", "--weight", "1", "--semantics", "cpp",
                    "--batch_size", "1000", "--results_dir", rdir, "--max_nodes", str(1 << 24)])
    finally:
        sys.stdout = sys.__stdout__
    res = data_utils.load_pickle(os.path.join(rdir, "results.pkl"))
    assert sorted(res.keys()) == ["num_nodes_generated", "paths", "solutions", "states", "times"]  # astar.py:382-397
    assert [len(s) for s in res["solutions"]] == [int(opt[i]) for i in pick]
    for i, soln, path in zip(pick, res["solutions"], res["paths"]):
        s = states[i][None].copy()
        for a in soln:
            s = co.next_state("puzzle15", s, a)
        assert co.is_solved("puzzle15", s)[0] and len(path) == len(soln) + 1
    log = open(os.path.join(rdir, "output.txt")).read()
    assert "pattern database 1,2,3,5,6/4,7,8,11,12/9,10,13,14,15: 50331648 bytes" in log
    for env, model in (("cube3", "pdb:auto"), ("puzzle15", "pdb:1,2,3/4,2")):
        try:
            with pytest.raises(ValueError):
                astar.main(["--states", spath, "--env", env, "--model_dir", model, "--weight", "1", "--semantics", "cpp",
                            "--results_dir", str(tmp_path / "bad")])
        finally:
            sys.stdout = sys.__stdout__


# ------------------------------------------------------------------------------------------------ 7. refusals
def test_refusals_through_the_c_abi_launch_nothing(L):
    lib = L.lib()
    table = torch.full((16 ** 4,), 0x5A, dtype=torch.uint8, device="cuda")
    states = dev(perms(64, 16, 1))
    out = torch.full((64,), -1.0, dtype=torch.float32, device="cuda")
    p, s = lambda t: C.c_void_p(t.data_ptr()), L.stream_ptr()

    def build(dim=4, tiles=(1, 2, 3), k=None, tab=p(table)):
        t = np.array(tiles, np.uint8)
        return lib.dca_pdb_build(dim, t.ctypes.data_as(C.c_void_p), len(tiles) if k is None else k, tab, None, s)

    def evaluate(dim=4, groups=((1, 2, 3),), ld=16, tabs=None, np_=None):
        t = np.array([x for g in groups for x in g], np.uint8)
        ks = np.array([len(g) for g in groups], np.int32)
        ptrs = (C.c_void_p * max(len(groups), 1))(*([table.data_ptr()] * len(groups) if tabs is None else tabs))
        return lib.dca_pdb_eval(dim, p(states), 64, ld, len(groups) if np_ is None else np_, t.ctypes.data_as(C.c_void_p),
                                ks.ctypes.data_as(C.c_void_p), ptrs, p(out), s)

    cases = {"k = 0": (lambda: build(k=0), b"k = 0"), "tile 0": (lambda: build(tiles=(0, 1, 2)), b"tile 0"),
             "tile >= N": (lambda: build(tiles=(1, 2, 16)), b"tile 16"), "a tile twice in a pattern": (lambda: build(tiles=(3, 2, 3)), b"tile 3"),
             "a null table": (lambda: build(tab=None), b"table"), "dim 2": (lambda: build(dim=2, tiles=(1,)), b"dim"),
             "dim 8": (lambda: build(dim=8, tiles=(1,)), b"dim"),
             "eval k = 0": (lambda: evaluate(groups=((1,), ())), b"k = 0"), "eval tile 0": (lambda: evaluate(groups=((0,),)), b"tile 0"),
             "eval tile >= N": (lambda: evaluate(groups=((16,),)), b"tile 16"),
             "a tile in two patterns": (lambda: evaluate(groups=((1, 2, 3), (4, 5, 1))), b"tile 1 appears twice"),
             "25 patterns": (lambda: evaluate(dim=7, ld=49, groups=tuple((t,) for t in range(1, 26))), b"num_patterns"),
             "a null table in the set": (lambda: evaluate(tabs=[0]), b"table 0 is NULL"), "ld < N": (lambda: evaluate(ld=15), b"ld"),
             "eval dim 2": (lambda: evaluate(dim=2), b"dim"), "eval dim 8": (lambda: evaluate(dim=8), b"dim")}
    for what, (fn, word) in cases.items():
        assert fn() == -1, what
        msg = lib.dca_last_error()
        assert msg.startswith(b"bad argument: dca_pdb_") and word in msg, (what, msg)
    torch.cuda.synchronize()
    assert bool((table == 0x5A).all()) and bool((out == -1.0).all()), "a refused call launches nothing"
    assert build() == 0 and evaluate() == 0
    torch.cuda.synchronize()
    assert np.array_equal(table.cpu().numpy(), ref.host_table(4, (1, 2, 3))) and bool((out >= 0).all())


def test_eval_refuses_tables_that_do_not_fit_their_pattern_before_any_launch(L):
    """pdb_eval checks what the library cannot see — a table's size and dtype, one table per pattern — in Python, before the
    call: ValueError, `out` untouched, and the valid call that follows returns exactly the host reference."""
    good = ref.host_table(3, (1,))
    assert good.size == 81
    rows = perms(64, 9, 3)
    want = ref.host_eval(3, rows, ((1,),), [good])
    states, table = dev(rows), dev(good)
    refused = {"80 bytes": [table[:80].clone()], "82 bytes": [torch.cat([table, table[:1]])],
               "int8": [table.to(torch.int8)], "two tables for one pattern": [table, table]}
    for what, tables in refused.items():
        out = torch.full((64,), -1.0, dtype=torch.float32, device="cuda")
        with pytest.raises(ValueError):
            L.pdb_eval(3, states, ((1,),), tables, out=out)
        got = L.pdb_eval(3, states, ((1,),), [table])
        torch.cuda.synchronize()
        assert bool((out == -1.0).all()), what
        assert np.array_equal(got.cpu().numpy(), want), what
