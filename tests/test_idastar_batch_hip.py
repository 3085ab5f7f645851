"""GPU: batches of sliding-puzzle roots (dca_idastar_npuzzle_batch, IDAStar.solve_batch, idastar.py --batch).  One launch of
ida_puzzle_batch_kernel runs the next threshold of every root still searching; root r's results are those of the single search
of that root alone, so every comparison is an equality: against idastar_npuzzle root by root, and against the host twin."""
import os
import sys

import numpy as np
import pytest
import torch

from tests import test_idastar_batch_cpu as cpu
from tests import test_idastar_cpu as ref
from tests.test_idastar_hip import P24_FOURS

pytestmark = pytest.mark.gpu

BIG = 1 << 40


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


def searches(env_name, spec):
    """(the plain search, the reflected one on the same built tables)"""
    from deepcubea_amd.search_methods.idastar import IDAStar
    from deepcubea_amd.utils.pattern_db import PatternDatabase
    plain = PatternDatabase(env_name, spec).build()
    mirror = PatternDatabase(env_name, plain.partition, reflect=True)
    mirror.tables, mirror.sweeps = plain.tables, plain.sweeps
    return IDAStar(env_name, plain), IDAStar(env_name, mirror)


@pytest.fixture(scope="module")
def p8(L):
    return searches("puzzle8", "4-4")


@pytest.fixture(scope="module")
def p15(L):
    return searches("puzzle15", "5-5-5")


@pytest.fixture(scope="module")
def p8_host_tables(p8):
    return [t.cpu().numpy() for t in p8[0].pdb.tables]


def puzzle_overshoot(L, max_nodes, res):
    """The header's bound on what the last launch of a puzzle search counts above what was left of max_nodes: (lanes that hold an
    item) x (nodes between two flushes of a lane), from the header's work-item rule and the counts of the launches before it."""
    per = res["nodes_per_threshold"]
    prev, left = (per[-2] if len(per) > 1 else 0), max_nodes - sum(per[:-1])
    depth = max(p for p in range(L.IDASTAR_MAX_PREFIX[L.ENV_NPUZZLE] + 1) if p == 0 or 4 * 3 ** (p - 1) <= 8 * prev)
    items = 4 * 3 ** (depth - 1) if depth else 1
    blocks = min(-(-items // 256), 8 * torch.cuda.get_device_properties(0).multi_processor_count, L.IDASTAR_MAX_LANES // 256)
    lanes = 256 * blocks
    assert left > 0
    return min(items, lanes) * min(L.IDASTAR_POLL_NODES, max(1, left // (2 * lanes)))


# ------------------------------------------------------------------------------------------------ puzzle8: the kernel against the singles
@pytest.mark.parametrize("reflect", [False, True])
def test_puzzle8_batch_equals_the_single_searches_and_the_host_twin(L, p8, p8_host_tables, prefix, reflect):
    """Nine roots at distances 0 .. 31.  Depth 7: 4 * 3^6 = 2916 items, 12 blocks a root, so the block -> root search has
    interior boundaries; depth -1: rounds in which roots own one block each; roots leave the batch round by round."""
    search = p8[int(reflect)]
    roots = cpu.p8_roots()
    for depth in cpu.DEPTHS:
        prefix(depth)
        got = search.solve_batch(roots, BIG)
        twin = L.idastar_host_batch(3, roots, ref.P8_PARTITION, p8_host_tables, BIG, reflect=reflect)
        assert len(got) == len(roots) == len(twin)
        for root, distance, res, host in zip(roots, cpu.DISTANCES, got, twin):
            cpu.same_search(res, search.solve(root, BIG), root)
            cpu.same_search(res, host, root)
            assert res["solved"] and len(res["moves"]) == distance, (depth, distance, res)


def test_no_state_leaks_between_roots_or_calls(p8, prefix):
    search = p8[0]
    root = ref.p8_states_at(26, 1, seed=13)[0]
    want = search.solve(root, BIG)
    for depth in (-1, 7):
        prefix(depth)
        got = search.solve_batch(np.stack([root, root, root]), BIG)
        for res in got:
            cpu.same_search(res, want, root)
            assert cpu.completed(res) == cpu.completed(got[0])
        one = search.solve_batch(root[None], BIG)
        assert len(one) == 1
        cpu.same_search(one[0], want, root)


def test_one_roots_budget_does_not_end_anothers_search(L, p8):
    search = p8[0]
    shallow, deep = (0, 1, 2, 3, 10, 20), 31
    roots = cpu.p8_roots(shallow + (deep,))
    free = [search.solve(r, BIG) for r in roots]
    # A shallow root's last count varies with the schedule, up to that threshold's whole tree.  The recursive search of
    # tests/test_idastar_cpu.py runs every threshold through the root's distance in full (it does not stop at the goal): the sum
    # of its counts is above whatever the kernel can count for that root.  The deep root runs out inside its completed
    # thresholds, whose counts are the tree's.
    whole = [sum(ref.reference_idastar_puzzle(3, r, ref.P8_PARTITION, ref.p8_tables(), d + 1)[1]) for r, d in zip(roots, shallow)]
    max_nodes = max(whole) + 1
    assert all(res["nodes_generated"] <= w for res, w in zip(free, whole))
    assert max_nodes < sum(cpu.completed(free[-1])), "the deep root must run out before its last threshold"
    got = search.solve_batch(roots, max_nodes)
    for root, res, want in zip(roots[:-1], got[:-1], free[:-1]):
        cpu.same_search(res, want, root)
        assert res["solved"]
    last = got[-1]
    assert last["status"] == "budget exhausted" and not last["solved"] and last["moves"] == [] and last["path_cost"] == float("inf")
    cpu.same_search(last, search.solve(roots[-1], max_nodes), roots[-1])
    over = puzzle_overshoot(L, max_nodes, last)
    print("budget %d: overshoot %d, bound %d" % (max_nodes, last["nodes_generated"] - max_nodes, over))
    assert max_nodes <= last["nodes_generated"] <= max_nodes + over, (last, over)
    assert over <= max(max_nodes // 2, L.IDASTAR_MAX_LANES) and over <= L.IDASTAR_OVERSHOOT


# ------------------------------------------------------------------------------------------------ shipped instances
@pytest.mark.parametrize("reflect", [False, True])
def test_puzzle15_twelve_shortest_shipped_states_as_one_batch(golden, p15, reflect):
    search = p15[int(reflect)]
    lens = golden["puzzle15_test_opt_len"]
    order = np.argsort(lens, kind="stable")[:12]
    roots = golden["puzzle15_test_states"][order]
    a, b = search.solve_batch(roots, BIG), search.solve_batch(roots, BIG)
    for i, root, first, second in zip(order, roots, a, b):
        print("puzzle15 state %d: length %d, nodes %d, thresholds %s" % (i, len(first["moves"]), first["nodes_generated"], first["thresholds"]))
        assert first["solved"] and len(first["moves"]) == int(lens[i])
        cpu.same_search(first, search.solve(root, BIG), root, dim=4)
        cpu.same_search(second, first, root, dim=4)  # two runs agree on everything but the last counts


def test_puzzle24_suffix_roots_as_one_batch(golden, L):
    """The <5> instances: six four-tile groups on roots 20, 30 and 40 moves from the goal of shipped state 0; and, reflected, four
    of the groups (a lane keeps two running indices per pattern, eight in all) on roots 10 and 14 moves from it."""
    from deepcubea_amd.search_methods.idastar import IDAStar
    from deepcubea_amd.utils.pattern_db import PatternDatabase
    six = PatternDatabase("puzzle24", P24_FOURS).build()
    four = PatternDatabase("puzzle24", P24_FOURS[:4], reflect=True)
    four.tables, four.sweeps = six.tables[:4], six.sweeps[:4]
    full, moves, n = golden["puzzle24_test_states"][0], golden["puzzle24_test_opt_moves"][0], int(golden["puzzle24_test_opt_len"][0])
    for pdb, ks in ((six, (20, 30, 40)), (four, (10, 14))):
        search = IDAStar("puzzle24", pdb)
        roots = np.stack([ref.replay_puzzle(5, full, moves[:n - k]) for k in ks])
        got = search.solve_batch(roots, BIG)
        for k, root, res in zip(ks, roots, got):
            print("puzzle24 %s, %d from the goal: nodes %d, thresholds %s" % (pdb.spec, k, res["nodes_generated"], res["thresholds"]))
            assert res["solved"] and len(res["moves"]) == k
            cpu.same_search(res, search.solve(root, BIG), root, dim=5)


# ------------------------------------------------------------------------------------------------ refusal, CLI
def test_a_bad_root_refuses_the_whole_batch_on_the_device_path(L, p8):
    search = p8[0]
    odd, i, word = cpu.bad_roots()[0]
    assert i == 1
    stream = L.stream_ptr()
    rc, msg, out = cpu.raw_batch("dca_idastar_npuzzle_batch", roots=odd, tables=[L.ptr(t) for t in search.pdb.tables], extra=(stream,))
    assert rc == -1 and "roots[1]: " in msg and word in msg and "dca_idastar_npuzzle_batch" in msg and cpu.untouched(out), msg
    with pytest.raises(L.DcaError, match=r"roots\[1\]: .*parity"):
        search.solve_batch(odd, BIG)
    good = cpu.p8_roots((10, 12, 14))
    rc, _, out = cpu.raw_batch("dca_idastar_npuzzle_batch", roots=good, tables=[L.ptr(t) for t in search.pdb.tables], extra=(stream,))
    assert rc == 0 and out["status"].tolist() == [0, 0, 0] and out["length"].tolist() == [10, 12, 14]  # the next valid call works
    assert [len(r["moves"]) for r in search.solve_batch(good, BIG)] == [10, 12, 14]
    with pytest.raises(ValueError, match="uint8 device tensor"):  # a host address must never reach the kernel's gathers
        L.idastar_npuzzle_batch(3, good, ref.P8_PARTITION, [t.cpu() for t in search.pdb.tables], BIG)


def test_cli_batch_reruns_a_refused_group_state_by_state(tmp_path, L):
    """Six states, a wrong-parity one among the first four, --batch 4: a group of four that the library refuses and the CLI runs
    again singly, then a group of two.  The same file with --batch 1 gives the same solved flags and lengths."""
    from deepcubea_amd.environments.n_puzzle import NPuzzleState
    from deepcubea_amd.search_methods import idastar
    from deepcubea_amd.utils import data_utils
    roots = [ref.p8_states_at(d, 1, seed=5)[0] for d in (12, 31, 7, 20, 3)]
    odd = roots[0].copy()
    a, b = [i for i in range(9) if odd[i] != 0][:2]
    odd[a], odd[b] = odd[b], odd[a]
    roots.insert(2, odd)
    spath = str(tmp_path / "states.pkl")
    data_utils.dump_pickle({"states": [NPuzzleState(r.copy()) for r in roots]}, spath)
    runs = {}
    for batch in (4, 1):
        rdir = str(tmp_path / ("out%d" % batch))
        try:
            idastar.main(["--states", spath, "--env", "puzzle8", "--model_dir", "pdb:4-4", "--results_dir", rdir, "--batch", str(batch)])
        finally:
            sys.stdout = sys.__stdout__
        runs[batch] = (data_utils.load_pickle(os.path.join(rdir, "results.pkl")), data_utils.load_pickle(os.path.join(rdir, "idastar.pkl")))
    (res, extra), (res1, extra1) = runs[4], runs[1]
    assert sorted(res.keys()) == sorted(res1.keys()) == ["num_nodes_generated", "paths", "solutions", "states", "times"]
    assert sorted(extra.keys()) == sorted(extra1.keys())
    assert extra["solved"] == extra1["solved"] == [True, True, False, True, True, True]
    assert [len(s) for s in res["solutions"]] == [len(s) for s in res1["solutions"]] == [12, 31, 0, 7, 20, 3]
    assert extra["status"][2].startswith("refused (") and "parity" in extra["status"][2] and res["num_nodes_generated"][2] == 0
    assert extra["thresholds"] == extra1["thresholds"] and len(res["times"]) == 6
    assert res["times"][0] == res["times"][3] and res["times"][4] == res["times"][5]  # a group's wall seconds over its size
    for root, soln, ok in zip(roots, res["solutions"], extra["solved"]):
        assert not ok or np.array_equal(ref.replay_puzzle(3, root, soln), ref.puzzle_goal(3))
