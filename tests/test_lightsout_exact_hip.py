"""GPU: the exact LightsOut heuristic (csrc/dca_lightsout_exact.hip) — eval and solve against the host's GF(2) product built
from the oracle's move rule, over sizes, layouts and arbitrary bytes; on the reference's 500 shipped test states against its
recorded solution lengths; as the closure of the engine and of the command line.  Integer work: every comparison is exact."""
import ctypes as C
import os
import sys

import numpy as np
import pytest
import torch

from tests.test_lightsout_exact_cpu import bits, host_solve, press_matrix

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GRID_CAP_ROWS = (1 << 14) * 256  # the launcher's grid cap (kPdbMaxEvalBlocks) times its block size


@pytest.fixture(scope="module")
def L():
    from deepcubea_amd import _lib
    _lib.require_gpu()
    return _lib


@pytest.fixture(scope="module")
def M(L):
    return L.lightsout_exact_matrix()


@pytest.fixture(scope="module")
def A():
    return press_matrix().astype(np.int64)


@pytest.fixture(scope="module")
def shipped():
    return np.load(os.path.join(ROOT, "tests", "golden", "lightsout_test.npz"))


@pytest.fixture(scope="module")
def cases(A):
    """press sets x (none, the 49 single cells, all cells, 4096 seeded random masks) and the states A x they make"""
    rng = np.random.default_rng(49)
    x = np.concatenate([np.zeros((1, 49), np.uint8), np.eye(49, dtype=np.uint8), np.ones((1, 49), np.uint8),
                        rng.integers(0, 2, (4096, 49), dtype=np.uint8)])
    states = (x.astype(np.int64) @ A.T % 2).astype(np.uint8)
    return x, states


def dev(a):
    return torch.from_numpy(np.ascontiguousarray(a)).cuda()


def mask_bits(t: torch.Tensor) -> np.ndarray:
    return bits(t.cpu().numpy().view(np.uint64))


def test_eval_and_solve_against_the_host_through_x(L, cases):
    x, states = cases
    want_h = x.sum(1).astype(np.float32)
    assert np.array_equal(L.lightsout_exact_eval(dev(states)).cpu().numpy(), want_h)
    assert np.array_equal(mask_bits(L.lightsout_exact_solve(dev(states))), x)
    order = np.random.default_rng(7).permutation(len(x))
    for n in (0, 1, 63, 64, 65, 255, 256, 257):  # across the wavefront and workgroup edges
        pick = order[:n]
        S = dev(states[pick].reshape(n, 49))
        h, p = L.lightsout_exact_eval(S), L.lightsout_exact_solve(S)
        assert h.shape == (n,) and h.dtype == torch.float32 and p.shape == (n,) and p.dtype == torch.int64
        assert np.array_equal(h.cpu().numpy(), want_h[pick]), n
        assert np.array_equal(mask_bits(p), x[pick].reshape(n, 49)), n


def test_layouts_poisoned_gaps_and_sentinels(L, cases):
    x, states = cases
    n = 257
    x, states = x[:n], states[:n]
    want_h = x.sum(1).astype(np.float32)

    def check(view, what):
        assert view.shape == (n, 49) and view.stride(1) == 1
        out = torch.full((n + 8,), -1.0, dtype=torch.float32, device="cuda")
        presses = torch.full((n + 8,), -1, dtype=torch.int64, device="cuda")
        L.lightsout_exact_eval(view, out=out)
        L.lightsout_exact_solve(view, out=presses)
        assert np.array_equal(out[:n].cpu().numpy(), want_h), what
        assert np.array_equal(mask_bits(presses[:n]), x), what
        assert bool((out[n:] == -1.0).all()) and bool((presses[n:] == -1).all()), what  # nothing past row n - 1

    for ld in (49, 52, 64, 100):
        buf = torch.full((n, ld), 0xFF, dtype=torch.uint8, device="cuda")  # the bytes between the rows must not matter
        buf[:, :49].copy_(dev(states))
        assert buf.data_ptr() % 4 == 0
        check(buf[:, :49], "ld %d" % ld)
        flat = torch.full((n * ld + 1,), 0xFF, dtype=torch.uint8, device="cuda")  # the same rows one byte off every grid
        rows = flat[1:].view(n, ld)[:, :49]
        rows.copy_(dev(states))
        assert rows.data_ptr() % 2 == 1
        check(rows, "ld %d, base + 1" % ld)
    wide = torch.full((n, 128), 0xFF, dtype=torch.uint8, device="cuda")
    for first in (16, 17):  # a strided view of a wider tensor: word loads (16) and byte loads (17)
        wide.fill_(0xFF)
        wide[:, first:first + 49].copy_(dev(states))
        check(wide[:, first:first + 49], "columns %d.. of a 128-byte row" % first)


def test_any_bytes_count_as_their_bit_0(L, M):
    rng = np.random.default_rng(255)
    junk = np.concatenate([rng.integers(0, 256, (1000, 49), dtype=np.uint8), np.full((2, 49), 0xFF, np.uint8),
                           np.full((2, 49), 0xFE, np.uint8)])
    x = host_solve(M, junk)
    for rows in (junk, junk & 1):
        assert np.array_equal(L.lightsout_exact_eval(dev(rows)).cpu().numpy(), x.sum(1).astype(np.float32))
        assert np.array_equal(mask_bits(L.lightsout_exact_solve(dev(rows))), x)
    assert not x[-1].any() and x[-3].sum() == host_solve(M, np.ones((1, 49), np.uint8)).sum()


def test_grid_stride_loop_second_trip(L, M):
    """The launcher caps its grid at 2^14 blocks of 256 threads: past 4 194 304 rows a thread takes a second row."""
    n = GRID_CAP_ROWS + 321
    gen = torch.Generator(device="cuda").manual_seed(5)
    S = torch.randint(0, 2, (n, 49), dtype=torch.uint8, device="cuda", generator=gen)
    h, p = L.lightsout_exact_eval(S), L.lightsout_exact_solve(S)
    pick = np.unique(np.concatenate([np.random.default_rng(3).integers(0, n, 2000), [0, GRID_CAP_ROWS - 1, GRID_CAP_ROWS,
                                                                                       GRID_CAP_ROWS + 1, n - 1]]))
    idx = torch.from_numpy(pick).cuda()
    x = host_solve(M, S[idx].cpu().numpy())
    assert np.array_equal(h[idx].cpu().numpy(), x.sum(1).astype(np.float32))
    assert np.array_equal(mask_bits(p[idx]), x)
    assert bool((torch.bitwise_right_shift(p, 49) == 0).all()) and float(h.max()) <= 49 and float(h.min()) >= 0


def test_shipped_states_have_their_recorded_lengths_and_solve_reaches_the_goal(L, shipped):
    e, d = L.env_ids("lightsout7")[:2]
    S = dev(shipped["states"])
    assert np.array_equal(L.lightsout_exact_eval(S).cpu().numpy(), shipped["soln_len"].astype(np.float32))  # all 500
    presses = L.lightsout_exact_solve(S)
    cur = S.clone()
    for a in range(49):
        rows = torch.nonzero((presses >> a) & 1).flatten()
        if rows.numel():
            cur[rows] = L.next_state(e, d, cur[rows].contiguous(), a)
    assert bool(L.is_solved(e, d, cur).bool().all())
    from deepcubea_amd.utils.lightsout_exact import LightsOutExact
    lists = LightsOutExact("lightsout7").solve(S[:20])
    off, flat = shipped["solution_offsets"], shipped["solutions"]
    assert lists == [sorted(flat[off[i]:off[i + 1]].tolist()) for i in range(20)]


def test_every_press_moves_the_distance_by_exactly_one(L):
    e, d = L.env_ids("lightsout7")[:2]
    S = dev(np.random.default_rng(12).integers(0, 2, (256, 49), dtype=np.uint8))
    h = L.lightsout_exact_eval(S).cpu().numpy()
    children = L.expand_fused(e, d, S)["children"]
    assert children.shape == (256, 49, 49)
    hc = L.lightsout_exact_eval(children.view(-1, 49)).cpu().numpy().reshape(256, 49)
    assert np.array_equal(np.abs(hc - h[:, None]), np.ones((256, 49), np.float32))
    assert np.array_equal((hc == h[:, None] - 1).sum(1), h.astype(np.int64))  # the h cells of the solution, and no other


@pytest.mark.parametrize("sem", ["py", "cpp"])
@pytest.mark.parametrize("B", [1, 1000])
def test_engine_with_the_closure_returns_the_optimal_solution(L, shipped, B, sem):
    """train.sh:68's weight 0.2: below weight 1 this heuristic still gives an optimal solution.  B = 1 steps the
    all-children path, B = 1000 the packed dedup-first path the command line uses."""
    from deepcubea_amd.search_methods.engine import BwasEngine
    from deepcubea_amd.utils.lightsout_exact import LightsOutExact
    from oracle import c_oracle as co
    exact = LightsOutExact("lightsout7")
    fn = exact.heuristic_fn_dev()
    lens = shipped["soln_len"]
    order = np.argsort(lens, kind="stable")
    eng = BwasEngine("lightsout7", 0.2, B, max_nodes=(1 << 16) if B == 1 else 36 * 49000 + (1 << 16),
                     semantics=L.SEM_PY if sem == "py" else L.SEM_CPP, packed=B == 1000)
    for i in (order[0], order[len(order) // 2], order[-1]):  # the smallest, the median and the largest recorded length
        root = shipped["states"][i]
        res = eng.solve(root, fn, max_iters=200)
        assert res["solved"], (i, res)
        assert res["path_cost"] == float(lens[i]) and len(res["moves"]) == int(lens[i]), (i, res["path_cost"], lens[i])
        s = root[None].copy()
        for a in res["moves"]:
            s = co.next_state("lightsout7", s, a)
        assert co.is_solved("lightsout7", s)[0]
        assert sorted(res["moves"]) == exact.solve(dev(root[None]))[0]
    eng.close()


def test_astar_cli_exact_model(tmp_path, L, shipped):
    from deepcubea_amd.environments.lights_out import LOState
    from deepcubea_amd.search_methods import astar
    from deepcubea_amd.utils import data_utils
    from oracle import c_oracle as co
    states, lens = shipped["states"], shipped["soln_len"]
    order = np.argsort(lens, kind="stable")
    pick = [0, int(order[0]), int(order[len(order) // 2]), int(order[-1])]
    spath = str(tmp_path / "states.pkl")
    data_utils.dump_pickle({"states": [LOState(states[i].copy()) for i in pick]}, spath)
    rdir = str(tmp_path / "exact")
    try:
        astar.main(["--states", spath, "--env", "lightsout7", "--model_dir", "exact:gf2", "--weight", "0.2", "--batch_size", "1000",
                    "--results_dir", rdir, "--max_nodes", str(36 * 49000 + (1 << 16))])
    finally:
        sys.stdout = sys.__stdout__
    res = data_utils.load_pickle(os.path.join(rdir, "results.pkl"))
    assert sorted(res.keys()) == ["num_nodes_generated", "paths", "solutions", "states", "times"]  # astar.py:382-397
    assert [len(s) for s in res["solutions"]] == [int(lens[i]) for i in pick]
    for i, soln, path in zip(pick, res["solutions"], res["paths"]):
        s = states[i][None].copy()
        for a in soln:
            s = co.next_state("lightsout7", s, a)
        assert co.is_solved("lightsout7", s)[0] and len(path) == len(soln) + 1 and not np.asarray(path[-1].tiles).any()
    assert "exact heuristic gf2 for lightsout7" in open(os.path.join(rdir, "output.txt")).read()
    for env, model in (("cube3", "exact:gf2"), ("lightsout7", "exact:foo")):
        try:
            with pytest.raises(ValueError):
                astar.main(["--states", spath, "--env", env, "--model_dir", model, "--weight", "0.2", "--results_dir", str(tmp_path / "bad")])
        finally:
            sys.stdout = sys.__stdout__


def test_refusals_through_the_c_abi_launch_nothing(L, cases):
    x, states = cases
    lib, n = L.lib(), 64
    S = dev(states[:n])
    out = torch.full((n,), -1.0, dtype=torch.float32, device="cuda")
    presses = torch.full((n,), -1, dtype=torch.int64, device="cuda")
    s = L.stream_ptr()
    sp, op, pp = S.data_ptr(), out.data_ptr(), presses.data_ptr()
    refused = {"dim 5": ((5, sp, n, 49), b"dim"), "dim 0": ((0, sp, n, 49), b"dim"), "ld 48": ((7, sp, n, 48), b"ld = 48"),
               "n -1": ((7, sp, -1, 49), b"n = -1"), "n 2^31": ((7, sp, 1 << 31, 49), b"n = 2147483648"),
               "null states": ((7, None, n, 49), b"states")}
    for what, (args, word) in refused.items():
        assert lib.dca_lightsout_exact_eval(args[0], args[1], args[2], args[3], op, s) == -1, what  # DCA_E_BADARG
        msg = lib.dca_last_error()
        assert msg.startswith(b"bad argument: dca_lightsout_exact_eval: ") and word in msg.split(b": ", 2)[2], (what, msg)
        assert lib.dca_lightsout_exact_solve(args[0], args[1], args[2], args[3], pp, s) == -1, what
        msg = lib.dca_last_error()
        assert msg.startswith(b"bad argument: dca_lightsout_exact_solve: ") and word in msg.split(b": ", 2)[2], (what, msg)
    assert lib.dca_lightsout_exact_eval(7, sp, n, 49, None, s) == -1 and b"out" in lib.dca_last_error()
    assert lib.dca_lightsout_exact_solve(7, sp, n, 49, None, s) == -1 and b"presses" in lib.dca_last_error()
    assert lib.dca_lightsout_exact_eval(7, None, 0, 49, None, s) == 0 and lib.dca_lightsout_exact_solve(7, None, 0, 49, None, s) == 0
    torch.cuda.synchronize()
    assert bool((out == -1.0).all()) and bool((presses == -1).all()), "a refused call launches nothing"
    assert lib.dca_lightsout_exact_eval(7, sp, n, 49, op, s) == 0 and lib.dca_lightsout_exact_solve(7, sp, n, 49, pp, s) == 0
    torch.cuda.synchronize()
    assert np.array_equal(out.cpu().numpy(), x[:n].sum(1).astype(np.float32)) and np.array_equal(mask_bits(presses), x[:n])
