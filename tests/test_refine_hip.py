"""GPU: bounded batches of cube3 roots (dca_idastar_cube3_batch, IDAStar.solve_bounded) and the window refiner on them.  One
launch of ida_cube3_batch_kernel<D> runs the next threshold of every root still searching; root r's results are those of the
single search of that root alone, so every comparison is an equality: against the host twin and against dca_idastar_cube3*
root by root."""
import numpy as np
import pytest
import torch

from tests import test_idastar_cpu as ref
from tests import test_refine_cpu as cpu

pytestmark = pytest.mark.gpu


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
def tables(L):
    return [torch.tensor(t, device="cuda") for t in cpu.sym.tables_of(cpu.IDA_SET)]


def device_batch(L, tables, roots, mode, max_length=None, max_nodes=cpu.BIG):
    n, dual = cpu.MODES[mode]
    return L.idastar_cube3_batch(roots, cpu.IDA_SET, tables, max_nodes, max_length=max_length, sym=n, dual=dual)


def device_single(L, tables, root, mode, max_nodes=cpu.BIG):
    n, dual = cpu.MODES[mode]
    return L.idastar_cube3(root, cpu.IDA_SET, tables, max_nodes, sym=n, dual=dual)


@pytest.mark.parametrize("mode", list(cpu.MODES))
def test_kernel_equals_the_host_twin_root_by_root(L, tables, prefix, mode):
    """The CPU tests' six roots.  Depth 3: 1728 items, 7 blocks a root, so the block -> root search has interior boundaries;
    depth -1 and 0: one block a root; depth 2: 144 items in one block.  Free, and with the bound two below each distance."""
    roots, distances = cpu.batch_roots()
    bounds = [max(k - 2, 0) for k in distances]
    for depth in cpu.DEPTHS:
        prefix(depth)
        for bound in (None, bounds):
            got, want = device_batch(L, tables, roots, mode, bound), cpu.batch(roots, mode, max_length=bound)
            for root, res, twin in zip(roots, got, want):
                cpu.same_search(res, twin, root)
            if bound is not None:
                assert [r["status"] for r in got] == ["bounded"] * 4 + ["solved", "bounded"], (depth, got)
                assert all(T <= b for r, b in zip(got, bounds) for T in r["thresholds"])


@pytest.mark.parametrize("mode", ["plain", "sym+dual"])
def test_64_roots_in_one_call_equal_64_single_calls(L, tables, mode):
    rng = np.random.default_rng(64)
    perm = L.cube3_perm_table()
    roots = []
    for r in range(64):
        cur = cpu.GOAL
        for a in rng.integers(0, 12, size=6 + r % 3):
            cur = cur[perm[a]]
        roots.append(cur)
    roots = np.stack(roots)
    got = device_batch(L, tables, roots, mode)
    assert len(got) == 64
    for r, (root, res) in enumerate(zip(roots, got)):
        cpu.same_search(res, device_single(L, tables, root, mode), root)
        assert res["solved"] and len(res["moves"]) <= 6 + r % 3 and (6 + r % 3 - len(res["moves"])) % 2 == 0  # a walk's parity


class DeviceSearch:
    """IDAStar.solve_bounded on IDA_SET's device tables (the class itself builds a shipped preset, which a test need not)."""

    def __init__(self, L, tables):
        self.L, self.tables = L, tables

    def solve_bounded(self, roots, max_length, max_nodes=None):
        return device_batch(self.L, self.tables, roots, "sym+dual", max_length, cpu.BIG if max_nodes is None else max_nodes)


@pytest.mark.parametrize("name", ["a a^1", "4-cycle", "three quarter turns"])
def test_refine_takes_the_padding_out_on_the_device(L, tables, name):
    """The padding stands behind the first move, so the first window holds all of it and is replaced by an optimal six or four
    moves, whichever of the equally short solutions a lane finds first: the result has ten moves."""
    from deepcubea_amd.search_methods import refine
    root, _ = cpu.optimal_suffix()
    padded = cpu.padded_paths(1)[name]
    moves, stats = refine.refine_moves(DeviceSearch(L, tables), padded, 8)
    assert (ref.replay_cube3(root, moves) == cpu.GOAL).all() and len(moves) == 10 == stats["length_out"], (moves, stats)
    assert stats["length_in"] == len(padded) and stats["unfinished"] == 0 and stats["passes"] >= 2
    cpu.assert_short_windows_optimal(moves)


def test_solve_bounded_goes_through_the_class(L, tables):
    from deepcubea_amd.search_methods.idastar import IDAStar
    from deepcubea_amd.utils.cube3_pdb import Cube3PatternDatabase
    pdb = Cube3PatternDatabase("c0,c1,c2/e8,e9,e10,e11+sym:4+dual").build()  # IDA_SET, built on the device
    assert pdb.sym == 4 and pdb.dual
    search = IDAStar("cube3", pdb)
    roots, distances = cpu.batch_roots()
    got = search.solve_bounded(roots, [k for k in distances])
    for root, k, res in zip(roots, distances, got):
        assert res["solved"] and len(res["moves"]) == k and (ref.replay_cube3(root, res["moves"]) == cpu.GOAL).all()
        want = search.solve(root)
        assert res["thresholds"] == want["thresholds"] and cpu.completed(res) == cpu.completed(want)
    assert [r["status"] for r in search.solve_bounded(roots[:4], 4)] == ["bounded"] * 4
