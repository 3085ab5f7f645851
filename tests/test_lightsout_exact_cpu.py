"""CPU: the exact LightsOut heuristic's host side (include/dca.h "exact LightsOut heuristic") — the constants the kernels use
(dca_lightsout_exact_matrix) against the move rule and against the reference's recorded run on its 500 shipped test states
(tests/golden/lightsout_test.npz), the spec handling of `--model_dir exact:gf2`, the ground-truth tool's statistics and the
refusals that need no device.  Integer work: every comparison is exact."""
import ctypes as C
import os
import sys
from types import SimpleNamespace

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.fixture(scope="module")
def M():
    from deepcubea_amd import _lib
    return _lib.lightsout_exact_matrix()


@pytest.fixture(scope="module")
def shipped():
    return np.load(os.path.join(ROOT, "tests", "golden", "lightsout_test.npz"))


def bits(rows: np.ndarray) -> np.ndarray:
    """uint64 masks -> uint8 [n, 49], bit i of a mask in column i"""
    return ((np.asarray(rows, np.uint64)[:, None] >> np.arange(49, dtype=np.uint64)) & np.uint64(1)).astype(np.uint8)


def host_solve(M: np.ndarray, states: np.ndarray) -> np.ndarray:
    """x = M s mod 2 per row -> uint8 [n, 49] (bit 0 of every byte is the cell)"""
    return ((np.asarray(states, np.int64) & 1) @ bits(M).astype(np.int64).T % 2).astype(np.uint8)


def press_matrix() -> np.ndarray:
    """A[i][a] = 1 where pressing a flips cell i, from the oracle's next_state on the goal (column a = the state one press makes)"""
    from oracle import c_oracle as co
    goal = np.zeros((1, 49), np.uint8)
    return np.stack([co.next_state("lightsout7", goal, a)[0] for a in range(49)], axis=1)


def test_matrix_is_the_inverse_of_the_press_matrix(M):
    from deepcubea_amd.environments.lights_out import LightsOut
    A = press_matrix()
    mm = LightsOut(7).move_matrix  # the Python environment's move table says the same
    A2 = np.zeros((49, 49), np.uint8)
    for a in range(49):
        A2[np.unique(mm[a]), a] = 1
    assert np.array_equal(A, A2) and np.array_equal(A, A.T) and A.sum() == 49 + 4 * 42
    assert M.dtype == np.uint64 and M.shape == (49,) and not (M >> np.uint64(49)).any()
    Mb = bits(M).astype(np.int64)
    assert np.array_equal(Mb @ A.astype(np.int64) % 2, np.eye(49, dtype=np.int64))
    assert np.array_equal(A.astype(np.int64) @ Mb % 2, np.eye(49, dtype=np.int64))
    assert np.array_equal(Mb, Mb.T)
    ones = Mb.sum(1)
    assert ones.min() == 14 and ones.max() == 23


def test_host_distance_equals_every_recorded_solution_length(M, shipped):
    states, lens = shipped["states"], shipped["soln_len"]
    assert states.shape == (500, 49) and states.dtype == np.uint8 and lens.shape == (500,) and lens.dtype == np.int16
    h = host_solve(M, states).sum(1)
    assert np.array_equal(h, lens.astype(np.int64))  # all 500
    assert (int(lens.min()), int(lens.max()), round(float(lens.mean()), 2)) == (13, 35, 24.26)
    assert np.array_equal(host_solve(M, states | 0xFE), host_solve(M, states))  # a cell is bit 0 of its byte


def test_recorded_solutions_are_the_press_sets(M, shipped):
    """An optimal solution presses no cell twice, and the press set of a state is unique: the recorded moves ARE the host solve."""
    x = host_solve(M, shipped["states"])
    flat, off = shipped["solutions"], shipped["solution_offsets"]
    assert off[0] == 0 and off[-1] == len(flat) and np.array_equal(np.diff(off), shipped["soln_len"])
    A = press_matrix().astype(np.int64)
    for i in range(500):
        moves = flat[off[i]:off[i + 1]].astype(np.int64)
        assert len(set(moves.tolist())) == len(moves), i
        assert np.array_equal(np.sort(moves), np.flatnonzero(x[i])), i
        assert np.array_equal(A @ x[i].astype(np.int64) % 2, shipped["states"][i]), i  # pressing the set from the goal makes the state


def test_spec_handling_needs_no_device(monkeypatch):
    import torch
    from deepcubea_amd.search_methods import astar
    from deepcubea_amd.utils.lightsout_exact import LightsOutExact, parse_exact_spec

    def touched(*a, **k):
        raise AssertionError("torch.cuda touched before the spec was refused")
    for name in ("is_available", "device_count", "current_device", "init"):
        monkeypatch.setattr(torch.cuda, name, touched)
    p = astar.build_parser()
    args = p.parse_args(["--states", "s.pkl", "--env", "lightsout7", "--model_dir", "exact:gf2", "--results_dir", "r",
                         "--weight", "0.2", "--batch_size", "1000"])
    assert args.model_dir == "exact:gf2" and astar._is_exact(args) and not astar._is_pdb(args)
    assert parse_exact_spec("lightsout7", "gf2") == "gf2" and LightsOutExact("lightsout7").spec == "gf2"
    for env in ("puzzle15", "cube3", "lightsout5", "puzzle8", "cube4"):
        with pytest.raises(ValueError):
            LightsOutExact(env)
        with pytest.raises(ValueError):
            astar._load_heuristic(SimpleNamespace(model_dir="exact:gf2", env=env), None)
    for model in ("exact:foo", "exact:", "exact:gf3", "exact:auto"):
        with pytest.raises(ValueError):
            astar._load_heuristic(SimpleNamespace(model_dir=model, env="lightsout7"), None)
    with pytest.raises(ValueError, match="one-hot"):
        LightsOutExact("lightsout7").heuristic_fn_dev()(None, True)
    env = SimpleNamespace(get_num_moves=lambda: 49)
    auto = SimpleNamespace(instances_per_gpu="auto", model_dir="exact:gf2", batch_size=1000, env="lightsout7", max_nodes="auto")
    assert astar.auto_instances(auto, env, 500, None) == 1  # integer values: one instance, as for pdb:
    help_text = " ".join({a.dest: a for a in p._actions}["model_dir"].help.split())
    assert "exact:gf2" in help_text and "--weight 0.2 --batch_size 1000" in help_text and "2^h" in help_text
    assert "pdb:SPEC" in help_text


def test_truth_tool_statistics_on_hand_made_arrays():
    sys.path.insert(0, os.path.join(ROOT, "tools"))
    try:
        import lightsout7_truth as tool
    finally:
        sys.path.pop(0)
    h = np.array([0.25, 2.0, 2.5, 5.0, 4.0, 3.4])
    hs = np.array([0, 2, 2, 5, 5, 2])
    rows, summary = tool.error_by_distance(h, hs)
    assert [r[:2] for r in rows] == [(0, 1), (2, 3), (5, 2)]
    want = [(0.25, 0.25, 0.25), ((0.0 + 0.5 + 1.4) / 3, 1.4, (2.0 + 2.5 + 3.4) / 3), (0.5, 1.0, 4.5)]
    for r, w in zip(rows, want):
        assert np.allclose(r[2:], w, rtol=0, atol=1e-12)
    # round(h) == h*: 0.25 -> 0 yes, 2.0 yes, 2.5 -> 2 (half to even) yes, 5.0 yes, 4.0 no, 3.4 -> 3 no
    assert np.allclose(summary, ((0.25 + 0.0 + 0.5 + 0.0 + 1.0 + 1.4) / 6, 1.4, 4 / 6), rtol=0, atol=1e-12)
    back = tool.distance_by_back_steps(np.array([0, 1, 1, 3, 1, 3]), np.array([0, 1, 3, 3, 3, 3]))
    assert back == [(0, 1, 0, 0.0, 0, 1.0), (1, 1, 1, 1.0, 1, 1.0), (3, 4, 1, 2.0, 3, 0.5)]
    for bad in ((np.zeros(3), np.zeros(2)), (np.zeros(0), np.zeros(0))):
        with pytest.raises(ValueError):
            tool.error_by_distance(*bad)
    with pytest.raises(ValueError):
        tool.distance_by_back_steps(np.zeros(3), np.zeros(2))


def test_matrix_refusals_through_the_c_abi():
    from deepcubea_amd import _lib
    lib = _lib.lib()
    rows = np.full(64, 0x5A5A5A5A5A5A5A5A, np.uint64)
    p = rows.ctypes.data_as(C.c_void_p)
    for what, (dim, ptr, word) in {"dim 5": (5, p, b"dim"), "dim 4": (4, p, b"dim"), "dim 0": (0, p, b"dim"), "dim 8": (8, p, b"dim"),
                                   "a null pointer": (7, None, b"rows")}.items():
        assert lib.dca_lightsout_exact_matrix(dim, ptr) == -1, what  # DCA_E_BADARG
        msg = lib.dca_last_error()
        assert msg.startswith(b"bad argument: dca_lightsout_exact_matrix") and word in msg, (what, msg)
    assert (rows == 0x5A5A5A5A5A5A5A5A).all()
    assert lib.dca_lightsout_exact_matrix(7, p) == 0
    assert np.array_equal(rows[:49], _lib.lightsout_exact_matrix()) and (rows[49:] == 0x5A5A5A5A5A5A5A5A).all()
