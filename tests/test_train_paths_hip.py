"""GPU tests of what `_lib.linear_train` does in each of its 2 x 3 modes (gemm x wgrad): which C entry points it calls and in
which order, what its autograd node keeps for the backward pass, and that its four results are BIT FOR BIT the ones the public
wrappers give when the test composes the same step from them (absmax_bits, split/cast_planes_scaled, split/cast_rows_scaled,
f16x3_gemm / f16_gemm, wgrad_f16, dy.sum(0)).  The kernels themselves are held against host arithmetic elsewhere
(test_train_operands_hip.py, test_train_gemm_hip.py, test_wgrad_*.py); this file pins the path through them.

Shapes: (256, 64, 64) is the smallest linear_train sends to the kernels and needs no padding; (257, 68, 72) pads both K
dimensions (68 and 72) to 128 and has a row count off every tile."""
import functools

import pytest
import torch

pytestmark = pytest.mark.gpu

SHAPES = [(256, 64, 64), (257, 68, 72)]  # (m, k, n)
MODES = [("f16x3", "library"), ("f16x3", "f16x3"), ("f16x3", "f16"), ("f16", "library"), ("f16", "f16"), ("f16", "f16x3")]  # (gemm, wgrad)
CASES = ["both", "no_dx", "no_dw"]  # gradients wanted: input and weight / weight alone (layer 1's case) / input alone

NAMES = {"A": "dca_absmax_bits", "P2": "dca_split_planes_scaled", "P1": "dca_cast_planes_scaled", "R2": "dca_split_rows_scaled",
         "R1": "dca_cast_rows_scaled", "G3": "dca_f16x3_gemm", "G1": "dca_f16_gemm", "W3": ("dca_wgrad_f16", 3), "W1": ("dca_wgrad_f16", 1)}
# entry points that launch kernels, in call order: the forward, then the backward of each gradient case
LAUNCHES = {
    ("f16x3", "library"): {"fwd": "A P2 R2 G3", "both": "A P2 R2 G3", "no_dx": "", "no_dw": "A P2 R2 G3"},
    ("f16x3", "f16x3"): {"fwd": "A P2 R2 G3", "both": "A P2 R2 G3 W3", "no_dx": "A P2 W3", "no_dw": "A P2 R2 G3"},
    ("f16x3", "f16"): {"fwd": "A P2 R2 G3", "both": "A P2 R2 G3 W1", "no_dx": "A P2 W1", "no_dw": "A P2 R2 G3"},
    ("f16", "library"): {"fwd": "A P1 R1 G1", "both": "A P1 R1 G1", "no_dx": "", "no_dw": "A P1 R1 G1"},
    ("f16", "f16"): {"fwd": "A P1 R1 G1", "both": "A P1 R1 G1 W1", "no_dx": "A P1 W1", "no_dw": "A P1 R1 G1"},
    ("f16", "f16x3"): {"fwd": "A P2 R1 G1", "both": "A P2 R1 G1 W3", "no_dx": "A P2 W3", "no_dw": "A P2 R1 G1"},
}
# planes of x the node keeps where wgrad is not "library" (there it keeps x itself)
SAVED_PLANES = {("f16x3", "f16x3"): 2, ("f16x3", "f16"): 2, ("f16", "f16"): 1, ("f16", "f16x3"): 2}


def _pad64(k: int) -> int:
    return (k + 63) // 64 * 64


def _spread(m: int, n: int, seed: int, binades: float = 20.0) -> torch.Tensor:
    g = torch.Generator().manual_seed(seed)
    return torch.randn(m, n, generator=g) * torch.exp2(-binades * torch.rand(m, n, generator=g)) * 3.0e-3


@functools.lru_cache(maxsize=None)
def _data(shape):
    m, k, n = shape
    return (_spread(m, k, 11 * m + k).cuda(), _spread(n, k, 13 * n + k).cuda() * 50.0, _spread(1, n, 17 * n)[0].cuda().contiguous(),
            _spread(m, n, 19 * m + n).cuda())


class _Spy:
    """Stands in for the library object: every symbol looked up on it is noted (dca_wgrad_f16 with its `products`), then called."""

    def __init__(self, real, calls):
        self._real, self._calls = real, calls

    def __getattr__(self, name):
        fn = getattr(self._real, name)

        def call(*a):
            self._calls.append((name, a[11]) if name == "dca_wgrad_f16" else name)
            return fn(*a)

        return call


@functools.lru_cache(maxsize=None)
def _run(mode, shape, case):
    """One forward and one backward of linear_train with the library spied on -> what was called, saved and computed."""
    from deepcubea_amd import _lib
    _lib.require_gpu()
    gemm, wgrad = mode
    m, k, n = shape
    x0, w0, b0, dy = _data(shape)
    lin = torch.nn.Linear(k, n).cuda()
    with torch.no_grad():
        lin.weight.copy_(w0)
        lin.bias.copy_(b0)
    lin.weight.requires_grad_(case != "no_dw")
    x = x0.clone().requires_grad_(case != "no_dx")
    real_lib, calls = _lib.lib, []
    spy = _Spy(real_lib(), calls)
    _lib.lib = lambda: spy
    try:
        y = _lib.linear_train(x, lin, wgrad=wgrad, gemm=gemm)
        n_fwd = len(calls)
        saved = [(t.dtype, tuple(t.shape)) for t in y.grad_fn.saved_tensors]
        y.backward(dy)
        torch.cuda.synchronize()
    finally:
        _lib.lib = real_lib
    calls = [c for c in calls[:n_fwd] if c != "dca_wgrad_workspace_bytes"], [c for c in calls[n_fwd:] if c != "dca_wgrad_workspace_bytes"]
    return {"fwd": calls[0], "bwd": calls[1], "saved": saved, "y": y.detach(), "dx": x.grad, "dw": lin.weight.grad, "db": lin.bias.grad}


def _expected(text):
    return [NAMES[a] for a in text.split()]


@pytest.mark.parametrize("shape", SHAPES)
@pytest.mark.parametrize("mode", MODES)
def test_each_mode_calls_these_entry_points_in_this_order(mode, shape):
    for case in CASES:
        r = _run(mode, shape, case)
        assert r["fwd"] == _expected(LAUNCHES[mode]["fwd"]), (case, "forward")
        assert r["bwd"] == _expected(LAUNCHES[mode][case]), (case, "backward")
        assert (r["dx"] is None) == (case == "no_dx") and (r["dw"] is None) == (case == "no_dw") and r["db"] is not None


@pytest.mark.parametrize("shape", SHAPES)
@pytest.mark.parametrize("mode", MODES)
def test_each_mode_keeps_these_tensors_for_the_backward_pass(mode, shape):
    m, k, n = shape
    saved = _run(mode, shape, "both")["saved"]
    if mode[1] == "library":
        assert saved == [(torch.float32, (m, k)), (torch.float32, (n, k))]
    else:
        assert saved == [(torch.float16, (SAVED_PLANES[mode], m, _pad64(k))), (torch.int32, (1,)), (torch.float32, (n, k))]


@pytest.mark.parametrize("shape", SHAPES)
@pytest.mark.parametrize("mode", MODES)
def test_each_mode_equals_the_public_wrappers_composed_bit_for_bit(mode, shape):
    from deepcubea_amd import _lib
    gemm, wgrad = mode
    m, k, n = shape
    x, w, b, dy = _data(shape)
    two = gemm == "f16x3" or wgrad == "f16x3"
    planes = _lib.split_planes_scaled if two else _lib.cast_planes_scaled

    def gemm_of(ap, amax, wt, bias):
        if gemm == "f16x3":
            wp, cs = _lib.split_rows_scaled(wt, amax, k_pad=ap.shape[2])
            return _lib.f16x3_gemm(ap, wp[0], wp[1], cs, 1.0, bias, None, False, False, True)[1]
        wh, cs = _lib.cast_rows_scaled(wt, amax, k_pad=ap.shape[2])
        return _lib.f16_gemm(ap[0], wh[0], cs, 1.0, bias)

    amax_x = _lib.absmax_bits(x)
    xp = planes(x, amax_x, n_pad=_pad64(k))
    assert tuple(xp.shape) == (2 if two else 1, m, _pad64(k))
    want_y = gemm_of(xp, amax_x, w, b)
    amax_dy = _lib.absmax_bits(dy)
    dyp = planes(dy, amax_dy, n_pad=_pad64(n))
    want_dx = gemm_of(dyp, amax_dy, w.t().contiguous(), None)
    want_db = dy.sum(0)

    r = _run(mode, shape, "both")
    assert torch.equal(r["y"], want_y), "y"
    assert torch.equal(r["dx"], want_dx), "dx"
    assert torch.equal(r["db"], want_db), "db"
    if wgrad == "library":
        want_dw = dy.t().mm(x)
        if not torch.equal(want_dw, dy.t().mm(x)):
            print("dW not compared: two evaluations of dy.t().mm(x) differ in their bits on this device")
            return
    else:
        want_dw = _lib.wgrad_f16(dyp, xp, n, k, amax_dy, amax_x, 3 if wgrad == "f16x3" else 1)
    assert torch.equal(r["dw"], want_dw), "dW"
    for case in ("no_dx", "no_dw"):  # a gradient that is not wanted does not change the ones that are
        q = _run(mode, shape, case)
        assert torch.equal(q["y"], want_y) and torch.equal(q["db"], want_db)
        assert q["dx"] is None or torch.equal(q["dx"], want_dx)
        assert q["dw"] is None or torch.equal(q["dw"], want_dw)
