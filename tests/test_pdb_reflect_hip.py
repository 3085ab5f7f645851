"""GPU: reflected look-ups for the sliding-puzzle pattern databases (dca_pdb_eval_reflected, dca_idastar_npuzzle_reflected,
`pdb:<spec>+reflect`).  Integer arithmetic throughout, so every comparison is exact: the eval kernel against the host loop over
the same row value and against the numpy restatement of tests/test_pdb_reflect_cpu.py, the search kernel against breadth-first
distances, shipped optimal lengths, the recursive search and the sequential host search."""
import os
import sys

import numpy as np
import pytest
import torch

from tests import test_idastar_cpu as ida
from tests import test_idastar_hip as plain_hip
from tests import test_pdb_cpu as pz
from tests import test_pdb_reflect_cpu as ref
from tests import test_puzzle8_cpu as p8

pytestmark = pytest.mark.gpu

BIG = ida.BIG
P24_FOUR_FOURS = plain_hip.P24_FOURS[:4]
P24_NODE_CAP = 2 * 10 ** 8  # what one puzzle24 search below may generate (it generates far less; see the test)


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


@pytest.fixture(scope="module")
def pdb8(L):
    from deepcubea_amd.utils.pattern_db import PatternDatabase
    return PatternDatabase("puzzle8", "4-4+reflect").build()


@pytest.fixture(scope="module")
def ida8(pdb8):
    from deepcubea_amd.search_methods.idastar import IDAStar
    return IDAStar("puzzle8", pdb8)


def dev(a):
    a = np.ascontiguousarray(a)
    return torch.from_numpy(a if a.flags.writeable else a.copy()).cuda()


def solved_puzzle(dim, root, res, length):
    assert res["solved"] and res["status"] == "solved" and len(res["moves"]) == length == res["path_cost"], (root, res)
    assert np.array_equal(ida.replay_puzzle(dim, root, res["moves"]), ida.puzzle_goal(dim))
    assert res["nodes_generated"] == sum(res["nodes_per_threshold"]) and (not length or res["thresholds"][-1] == length)


# ------------------------------------------------------------------------------------------------ eval
def test_kernel_eval_on_the_whole_puzzle8_space(L, pdb8):
    states, dist, _ = p8.bfs_table()
    assert pdb8.reflect and pdb8.spec == "1,2,3,4/5,6,7,8+reflect"
    host_tables = [t.cpu().numpy() for t in pdb8.tables]
    assert all(np.array_equal(t, w) for t, w in zip(host_tables, ida.p8_tables()))
    dX = dev(states)
    got = pdb8.heuristic(dX).cpu().numpy()
    assert np.array_equal(got, L.pdb_eval_host(3, states, pdb8.partition, host_tables, reflect=True))
    assert np.array_equal(pdb8.heuristic_fn_dev()(dX).cpu().numpy(), got)
    plain = L.pdb_eval(3, dX, pdb8.partition, pdb8.tables).cpu().numpy()
    mirrored = L.pdb_eval(3, dev(ref.mirror_rows(3, states)), pdb8.partition, pdb8.tables).cpu().numpy()
    assert np.array_equal(got, np.maximum(plain, mirrored)) and (got <= dist).all()
    assert (int((mirrored > plain).sum()), int((mirrored < plain).sum()), int((mirrored == plain).sum())) == (49304, 49304, 82832)
    assert int(got.sum()) == 3589500


@pytest.mark.parametrize("dim", [3, 4, 5, 6, 7])
def test_any_bytes_both_load_widths(L, dim):
    """Rows of random bytes on random tables: an aligned base with a row stride that is a multiple of 4 (word loads), with
    ld = N, and a base one byte off with ld = N + 3 (byte loads)."""
    from deepcubea_amd.utils.pattern_db import PatternDatabase
    N = dim * dim
    partition, tables, rows = ref.random_rows_case(dim, 40 + dim)
    want = ref.host_eval_reflected(dim, rows, partition, tables)
    pdb = PatternDatabase("puzzle%d" % (N - 1), partition, reflect=True).set_tables(tables)
    for n in (0, 1, 257, len(rows)):
        for ld, off in ((N, 0), ((N + 3) // 4 * 4, 0), (N + 3, 1)):
            buf = torch.full((n * ld + off + 8,), 0xA5, dtype=torch.uint8, device="cuda")
            view = buf[off:off + n * ld].view(n, ld)[:, :N]
            view.copy_(dev(rows[:n]))
            assert n == 0 or view.data_ptr() % 4 == off
            out = torch.full((n + 8,), -1.0, dtype=torch.float32, device="cuda")
            L.pdb_eval(dim, view, partition, pdb.tables, out=out, reflect=True)
            assert np.array_equal(out[:n].cpu().numpy(), want[:n]), (dim, n, ld, off)
            assert bool((out[n:] == -1.0).all())  # no stray write
    assert np.array_equal(pdb.heuristic(dev(rows)).cpu().numpy(), want)


def test_one_grid_stride_wrap(L, pdb8):
    states = p8.all_states()
    n = (1 << 14) * 256 + 5  # one row loop's second trip for the first five threads
    reps = -(-n // len(states))
    big = dev(states).repeat(reps, 1)[:n]
    want = np.tile(ref.host_eval_reflected(3, states, pdb8.partition, ida.p8_tables()), reps)[:n]
    assert np.array_equal(pdb8.heuristic(big).cpu().numpy(), want)


# ------------------------------------------------------------------------------------------------ IDA*
@pytest.mark.parametrize("distance", [0, 1, 2, 3, 10, 20, 30, 31])
def test_puzzle8_reflected_length_is_the_breadth_first_distance(ida8, distance):
    for root in ida.p8_states_at(distance, 3 if distance not in (0, 31) else 2):
        solved_puzzle(3, root, ida8.solve(root, BIG), distance)


def test_puzzle8_reflected_counts_equal_a_recursive_search(ida8, prefix):
    for root, d, _, (thresholds, counts) in ref.p8_count_cases():
        for depth in (-1, 5):
            prefix(depth)
            res = ida8.solve(root, BIG)
            solved_puzzle(3, root, res, d)
            assert res["thresholds"] == thresholds + [d] and res["nodes_per_threshold"][:len(counts)] == counts, (res, counts)


def test_device_counts_equal_the_host_search_with_eight_live_indices(L, prefix):
    dim, partition, tables, root, k, thresholds, counts = ref.small_case("puzzle15")
    want = L.idastar_host(L.ENV_NPUZZLE, dim, root, partition, tables, BIG, reflect=True)
    assert want["solved"] and len(want["moves"]) == k
    dtables = [dev(t) for t in tables]
    for depth in (-1, 8):
        prefix(depth)
        res = L.idastar_npuzzle(dim, root, partition, dtables, BIG, reflect=True)
        solved_puzzle(dim, root, res, k)
        assert res["thresholds"] == want["thresholds"] == thresholds + [k]
        assert res["nodes_per_threshold"][:-1] == want["nodes_per_threshold"][:-1] == counts


def test_puzzle15_twelve_shortest_shipped_states_plain_and_reflected(L, golden):
    from deepcubea_amd.utils.pattern_db import PatternDatabase
    pdb = PatternDatabase("puzzle15", "5-5-5").build()
    lens = golden["puzzle15_test_opt_len"]
    totals = [0, 0]
    for i in np.argsort(lens, kind="stable")[:12]:
        root = golden["puzzle15_test_states"][i]
        plain = L.idastar_npuzzle(4, root, pdb.partition, pdb.tables, BIG)
        mirrored = L.idastar_npuzzle(4, root, pdb.partition, pdb.tables, BIG, reflect=True)
        solved_puzzle(4, root, plain, int(lens[i]))
        solved_puzzle(4, root, mirrored, int(lens[i]))
        plain_at = dict(zip(plain["thresholds"][:-1], plain["nodes_per_threshold"][:-1]))
        for T, count in zip(mirrored["thresholds"][:-1], mirrored["nodes_per_threshold"][:-1]):
            assert T not in plain_at or count <= plain_at[T], (i, T, count, plain_at)
        totals[0] += plain["nodes_generated"]
        totals[1] += mirrored["nodes_generated"]
        print("puzzle15 state %d, length %d: nodes plain %d, reflected %d" % (i, lens[i], plain["nodes_generated"], mirrored["nodes_generated"]))
    print("puzzle15 5-5-5, twelve shortest shipped states: total nodes plain %d, reflected %d" % tuple(totals))


def test_puzzle24_suffix_roots_with_four_four_tile_groups(L, golden):
    """The 128-bit board with eight live indices.  20 and 30 moves from the goal: on the host, with the 3-tile sub-patterns
    (1,2,3)/(5,6,7)/(9,10,11)/(13,14,15) that these groups dominate, the two reflected searches generate 1 055 and 155 007 nodes, far below the cap."""
    from deepcubea_amd.search_methods.idastar import IDAStar
    from deepcubea_amd.utils.pattern_db import PatternDatabase
    search = IDAStar("puzzle24", PatternDatabase("puzzle24", P24_FOUR_FOURS, reflect=True).build())
    for k in (20, 30):
        root = ref.suffix_root(golden, "puzzle24", 5, 0, k)
        res = search.solve(root, P24_NODE_CAP)
        print("puzzle24 %d from the goal, reflected: nodes %d, thresholds %s" % (k, res["nodes_generated"], res["thresholds"]))
        solved_puzzle(5, root, res, k)


# ------------------------------------------------------------------------------------------------ engine and CLIs
def _far_states():
    states = np.concatenate([ida.p8_states_at(d, 2, seed=9) for d in range(20, 30)])
    assert len(states) == 20
    return states, p8.distance(states)


def test_engine_with_the_reflected_closure_finds_breadth_first_lengths(L, pdb8):
    from deepcubea_amd.search_methods.engine import BwasEngine
    states, dist = _far_states()
    eng = BwasEngine("puzzle8", 1.0, 1000, max_nodes=1 << 22, semantics=L.SEM_CPP)
    fn = pdb8.heuristic_fn_dev()
    for root, d in zip(states, dist):
        res = eng.solve(root, fn, max_iters=20000)
        assert res["solved"] and len(res["moves"]) == d, (root, d, res)
        assert np.array_equal(ida.replay_puzzle(3, root, res["moves"]), ida.puzzle_goal(3))
    eng.close()


@pytest.mark.parametrize("cli", ["astar", "idastar"])
def test_clis_take_the_suffix(tmp_path, L, cli):
    from deepcubea_amd.environments.n_puzzle import NPuzzleState
    from deepcubea_amd.search_methods import astar, idastar
    from deepcubea_amd.utils import data_utils
    states, dist = _far_states()
    spath, rdir = str(tmp_path / "states.pkl"), str(tmp_path / cli)
    data_utils.dump_pickle({"states": [NPuzzleState(s.copy()) for s in states]}, spath)
    common = ["--states", spath, "--env", "puzzle8", "--model_dir", "pdb:4-4+reflect", "--results_dir", rdir]
    try:
        if cli == "astar":
            astar.main(common + ["--weight", "1", "--semantics", "cpp", "--batch_size", "1000", "--max_nodes", str(1 << 22)])
        else:
            idastar.main(common)
    finally:
        sys.stdout = sys.__stdout__
    res = data_utils.load_pickle(os.path.join(rdir, "results.pkl"))
    assert [len(s) for s in res["solutions"]] == [int(d) for d in dist]
    for root, soln in zip(states, res["solutions"]):
        assert np.array_equal(ida.replay_puzzle(3, root, soln), ida.puzzle_goal(3))
    assert "pattern database 1,2,3,4/5,6,7,8+reflect: 118098 bytes" in open(os.path.join(rdir, "output.txt")).read()


# ------------------------------------------------------------------------------------------------ refusals
def test_device_refusals_come_before_any_launch(L, pdb8):
    good = ida.p8_states_at(10, 1)[0]
    ones = tuple((t,) for t in range(1, 6))
    tables = [dev(pz.host_table(3, g)) for g in ones]
    with pytest.raises(L.DcaError, match="num_patterns = 5"):
        L.idastar_npuzzle(3, good, ones, tables, 1000, reflect=True)
    assert L.idastar_npuzzle(3, good, ones, tables, BIG)["solved"] and L.idastar_npuzzle(3, good, ones[:4], tables[:4], BIG, reflect=True)["solved"]
    odd = good.copy()
    a, b = [i for i in range(9) if odd[i] != 0][:2]
    odd[a], odd[b] = odd[b], odd[a]
    with pytest.raises(L.DcaError, match="parity"):
        L.idastar_npuzzle(3, odd, pdb8.partition, pdb8.tables, 1000, reflect=True)
    with pytest.raises(ValueError, match="uint8 device tensor"):
        L.idastar_npuzzle(3, good, pdb8.partition, [t.cpu() for t in pdb8.tables], 1000, reflect=True)
