"""GPU tests of the training step's NON-parity GEMM mode (`--train_gemm f16`): the one-product kernel dca_f16_gemm on the scaled high
fp16 planes, the high-plane-only operand kernels dca_cast_planes_scaled / dca_cast_rows_scaled, `_lib.linear_train(..., gemm="f16")`
and the whole step.

Outputs are NaN-filled before every call; what a kernel must not write has to keep the fill.  Integer operands make every partial
sum an integer below 2^24, so the fp32 result is exact in any order and a difference is a wiring error."""
import ctypes as C
import importlib.util
import math
import os
import random

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
U16 = 2.0 ** -11  # unit roundoff of an fp16 high plane: the cast kernels convert with (_Float16)v, round to nearest even
NAN16 = 0x7E00


def _parity_tool():
    """tools/train_gemm_parity.py: the functions that produced profiles/train_gemm_parity.txt are the ones asserted on here."""
    spec = importlib.util.spec_from_file_location("train_gemm_parity", os.path.join(ROOT, "tools", "train_gemm_parity.py"))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod


def _pad64(v):
    return (v + 63) // 64 * 64


def _nan(shape, dtype=torch.float32):
    return torch.full(shape, float("nan"), dtype=dtype, device="cuda")


def _p(t, off=0):
    return C.c_void_p(0 if t is None else t.data_ptr() + off)


def _h16(t):
    return t.view(torch.int16).to(torch.int32) & 0xFFFF


# ------------------------------------------------------------------------------ 1. exact on integers
_M = (1, 15, 16, 17, 255, 256, 257, 513)
_N = (4, 60, 64, 68, 252, 256, 260)
_K = (64, 128, 192, 320)  # one, two, three and five 64-deep K-steps: both stage parities, the pipeline's head and tail
INT_CASES = [(m, _N[(i + 3 * j) % 7], _K[(i + j) % 4]) for i, m in enumerate(_M) for j in (0, 1)]
INT_CASES.append((2305, 260, 64))  # ten M tiles: the tile map's second group of eight returns early for six of them


def _window(rows, width, ld, values):
    """An fp16 [rows + 2, ld] NaN buffer on the device with `values` [rows, width] in rows 1..rows+1, and the row window inside it."""
    buf = torch.full((rows + 2, ld), float("nan"), dtype=torch.float16)
    buf[1:rows + 1, :width] = values.to(torch.float16)
    buf = buf.cuda()
    return buf, buf[1:rows + 1]


def _gemm_raw(a_win, m, k, lda, w_win, n, ldw, cs, bias, alpha=1.0):
    """dca_f16_gemm through ctypes into the column window [4, 4 + n) of rows 1..m+1 of an fp32 [m + 2, n + 12] NaN buffer."""
    from deepcubea_amd import _lib
    ldo = n + 12
    buf = _nan((m + 2, ldo))
    rc = _lib.lib().dca_f16_gemm(_p(a_win), m, k, lda, _p(w_win), n, ldw, _p(cs), alpha, _p(bias), _p(buf, 4 * (ldo + 4)), ldo,
                                 _lib.stream_ptr())
    torch.cuda.synchronize()
    return rc, buf


def _only_window_written(buf, m, n):
    mask = torch.ones_like(buf, dtype=torch.bool)
    mask[1:m + 1, 4:4 + n] = False
    return bool(torch.isnan(buf[mask]).all()) and not bool(torch.isnan(buf[1:m + 1, 4:4 + n]).any())


def test_the_integer_cases_reach_every_size():
    assert {c[0] for c in INT_CASES} == set(_M) | {2305} and {c[1] for c in INT_CASES} == set(_N) and {c[2] for c in INT_CASES} == set(_K)
    assert all(sum(1 for c in INT_CASES if c[0] == m) == 2 for m in _M)


@pytest.mark.parametrize("m,n,k", INT_CASES)
def test_integer_operands_are_exact_and_only_the_window_is_written(m, n, k):
    """a_h, w_h integers in [-8, 8], bias integers, col_scale powers of two in 2^-3..2^3, alpha = 1: the result equals int64 host
    arithmetic bit for bit (|sum| <= 64 k <= 20480, times 8, plus the bias: far below 2^24, so every fp32 operation is exact
    whatever the order inside the MFMA).  lda = k + 8, ldw = k + 16 with NaN in the extra columns; a and w are row windows inside
    NaN-filled buffers; the output is a window at column 4 of a NaN-filled [m + 2, n + 12] matrix.  Also with col_scale = NULL and
    with bias = NULL."""
    from deepcubea_amd import _lib
    _lib.require_gpu()
    gen = torch.Generator().manual_seed(100000 * m + 1000 * n + k)
    a = torch.randint(-8, 9, (m, k), generator=gen)
    w = torch.randint(-8, 9, (n, k), generator=gen)
    bias = torch.randint(-100, 101, (n,), generator=gen)
    ce = torch.randint(-3, 4, (n,), generator=gen)
    _, a_win = _window(m, k, k + 8, a)
    _, w_win = _window(n, k, k + 16, w)
    cs_d, bias_d = torch.exp2(ce.float()).cuda(), bias.float().cuda()
    prod = (a @ w.t()).double()
    assert float(prod.abs().max()) * 8 + 100 < 2 ** 24
    for cs, b in ((cs_d, bias_d), (None, bias_d), (cs_d, None), (None, None)):
        want = prod * (torch.exp2(ce.double())[None, :] if cs is not None else 1.0) + (bias.double()[None, :] if b is not None else 0.0)
        rc, buf = _gemm_raw(a_win, m, k, k + 8, w_win, n, k + 16, cs, b)
        assert rc == 0, _lib.lib().dca_last_error()
        assert _only_window_written(buf, m, n), (cs is None, b is None)
        got = buf[1:m + 1, 4:4 + n].cpu()
        assert torch.equal(got, want.float()) and torch.equal(got.double(), want), (cs is None, b is None)


# ------------------------------------------------------------------------------ 2. launch-to-launch determinism
def test_two_launches_give_the_same_bits():
    from deepcubea_amd import _lib
    _lib.require_gpu()
    m, n, k = 1000, 324, 256
    g = torch.Generator().manual_seed(7)
    a = (torch.randn(m, k, generator=g) * 300).to(torch.float16).cuda()
    w = (torch.randn(n, k, generator=g) * 300).to(torch.float16).cuda()
    cs = torch.exp2(torch.randint(-20, -10, (n,), generator=g).float()).cuda()
    bias = torch.randn(n, generator=g).cuda()
    first = _lib.f16_gemm(a, w, cs, 1.0, bias, out=_nan((m, n)))
    second = _lib.f16_gemm(a, w, cs, 1.0, bias, out=_nan((m, n)))
    torch.cuda.synchronize()
    assert bool(torch.isfinite(first).all()) and torch.equal(first.view(torch.int32), second.view(torch.int32))
    ref = (a.double() @ w.double().t()) * cs.double()[None, :] + bias.double()[None, :]
    assert float((first.double() - ref).abs().max()) <= 1e-4 * float(ref.abs().max())  # (and they are the product, not noise)


# ------------------------------------------------------------------------------ 3. derived bound on real data
def _spread(shape, gen, top, spread=9.9):
    """Random signs, magnitudes top * 2^-(spread * U[0, 1)): within 2^-spread of the largest, so every element of the scaled high
    plane is a NORMAL fp16 number (the largest element goes to [2^14, 2^15), the smallest stays above 2^4)."""
    sign = torch.randint(0, 2, shape, generator=gen).float() * 2.0 - 1.0
    return sign * top * torch.exp2(-spread * torch.rand(shape, generator=gen))


def _f16_bound(a, w, bias, k_pad):
    """Elementwise bound of the one-product GEMM against float64 for operands whose scaled high planes are all NORMAL fp16 numbers:
    each operand is rounded once to 11 bits (u = 2^-11; the power-of-two scales are exact), products of fp16 numbers are exact in
    fp32, then k_pad fp32 additions in any order, the scale, the bias add and the store:
    |y - y64| <= (2u + u^2 + (k_pad + 4) 2^-24) (|a| |w|^T + |b|)."""
    mag = a.double().abs() @ w.double().abs().t()
    if bias is not None:
        mag = mag + bias.double().abs()[None, :]
    return (2.0 * U16 + U16 ** 2 + (k_pad + 4) * 2.0 ** -24) * mag


@pytest.mark.parametrize("m,n,k", [(300, 132, 68), (777, 256, 512), (1000, 324, 200)])
def test_real_data_through_the_cast_kernels_stays_inside_the_derived_bound(m, n, k):
    """x [m, k] within 2^-9.9 of its largest element, W [n, k] the same per ROW (rows at different magnitudes), operands through
    cast_planes_scaled / cast_rows_scaled: |y - y64| <= (2u + u^2 + (k_pad + 4) 2^-24) (|x| |W|^T + |b|) elementwise."""
    from deepcubea_amd import _lib
    _lib.require_gpu()
    g = torch.Generator().manual_seed(13 * m + n)
    x = _spread((m, k), g, 3.0).cuda()
    w = (_spread((n, k), g, 1.0) * torch.exp2(torch.randint(-12, 5, (n, 1), generator=g).float())).cuda()
    bias = torch.randn(n, generator=g).cuda()
    kp = _pad64(k)
    amax = _lib.absmax_bits(x)
    xh = _lib.cast_planes_scaled(x, amax, n_pad=kp)
    wh, cs = _lib.cast_rows_scaled(w, amax, k_pad=kp)
    assert float(xh[0, :, :k].float().abs().min()) >= 16.0 and float(wh[0, :, :k].float().abs().min()) >= 16.0  # normal, by far
    y = _lib.f16_gemm(xh[0], wh[0], cs, 1.0, bias, out=_nan((m, n)))
    err = (y.double() - (x.double() @ w.double().t() + bias.double()[None, :])).abs()
    bound = _f16_bound(x, w, bias, kp)
    print("TRAIN_GEMM f16 (%d, %d, %d): worst err / bound %.3g" % (m, n, k, float((err / bound).max())))
    assert bool(torch.isfinite(y).all()) and bool((err <= bound).all()), float((err / bound).max())


# ------------------------------------------------------------------------------ 4. refusals
def test_every_refusal_returns_badarg_and_leaves_the_output_alone():
    from deepcubea_amd import _lib
    _lib.require_gpu()
    L = _lib.lib()
    m, n, k = 40, 8, 128
    a = torch.ones((m, 136), dtype=torch.float16, device="cuda")
    w = torch.ones((n, 136), dtype=torch.float16, device="cuda")
    out = _nan((m, 16))

    def call(ah=_p(a), m=m, k=k, lda=136, wh=_p(w), n=n, ldw=136, xo=_p(out), ldo=16):
        return L.dca_f16_gemm(ah, m, k, lda, wh, n, ldw, None, 1.0, None, xo, ldo, _lib.stream_ptr())

    cases = (dict(k=96), dict(k=32), dict(k=0), dict(lda=120), dict(lda=132), dict(ldw=120), dict(ldw=132), dict(ldo=4), dict(ldo=10),
             dict(n=0), dict(m=-1), dict(ah=None), dict(wh=None), dict(xo=None), dict(ah=_p(a, 8)), dict(wh=_p(w, 2)), dict(xo=_p(out, 4)),
             dict(xo=_p(out, 8)))
    for kw in cases:
        assert call(**kw) == -1, kw
        assert L.dca_last_error().decode().startswith("bad argument: "), kw
    torch.cuda.synchronize()
    assert bool(torch.isnan(out).all())
    assert call(m=0) == 0  # no rows: nothing to do, nothing written
    torch.cuda.synchronize()
    assert bool(torch.isnan(out).all())
    assert call() == 0, L.dca_last_error()  # the same call with nothing wrong goes through
    torch.cuda.synchronize()
    assert bool((out[:, :n] == float(k)).all()) and bool(torch.isnan(out[:, n:]).all())
    with pytest.raises(_lib.DcaError, match="bad argument"):  # and the wrapper turns a refusal into DcaError
        _lib.f16_gemm(a[:, :96], w[:, :96], None, 1.0, None)


# ------------------------------------------------------------------------------ 5. the cast kernels
def _word(value):
    return torch.tensor([int(np.float32(value).view(np.uint32))], dtype=torch.int64).to(torch.int32).cuda()


def _amax_cases(x):
    from deepcubea_amd import _lib
    return {"own": _lib.absmax_bits(x), "zero": _word(0.0), "inf": _word(float("inf")), "denormal": _word(1e-40), "none": None}


@pytest.mark.parametrize("m,n,n_pad", [(1, 4, 64), (37, 68, 128), (300, 132, 192)])
def test_cast_planes_scaled_is_the_high_plane_of_the_split_bit_for_bit(m, n, n_pad):
    """out_h == plane 0 of split_planes_scaled for the same amax word (its own |max|, 0, inf, a denormal — the last three stand for
    scale 1 — and NULL); pad columns zero; the 8 columns past n_pad keep the fill.  The source is a column window of a wider
    NaN matrix."""
    from deepcubea_amd import _lib
    _lib.require_gpu()
    g = torch.Generator().manual_seed(m + n)
    wide = _nan((m, n + 8))
    wide[:, 4:4 + n] = (torch.randn(m, n, generator=g) * torch.exp2(-14.0 * torch.rand(m, n, generator=g))).cuda()
    x = wide[:, 4:4 + n]
    for name, amax in _amax_cases(x.contiguous()).items():
        both = _lib.split_planes_scaled(x, amax, n_pad=n_pad, ldo=n_pad + 8, out=_nan((2, m, n_pad + 8), torch.float16))
        one = _lib.cast_planes_scaled(x, amax, n_pad=n_pad, ldo=n_pad + 8, out=_nan((1, m, n_pad + 8), torch.float16))
        torch.cuda.synchronize()
        assert torch.equal(_h16(one[0]), _h16(both[0])), name
        assert bool((_h16(one[0, :, n:n_pad]) == 0).all()) and bool((_h16(one[0, :, n_pad:]) == NAN16).all()), name
        assert bool(torch.isfinite(one[0, :, :n_pad]).all()), name
        if name in ("zero", "inf", "denormal", "none"):  # scale 1: the plain conversion
            assert torch.equal(_h16(one[0, :, :n]), _h16(x.to(torch.float16))), name


@pytest.mark.parametrize("n,k,k_pad", [(4, 64, 64), (132, 260, 320), (1000, 324, 384)])
def test_cast_rows_scaled_is_the_high_plane_and_the_col_scale_of_the_split_bit_for_bit(n, k, k_pad):
    """out_h and col_scale == split_rows_scaled's for the same other-operand word; rows at different magnitudes, one row all zero
    (its own |max| word is 0: scale 1); pad columns zero; the 8 columns past k_pad keep the fill."""
    from deepcubea_amd import _lib
    _lib.require_gpu()
    g = torch.Generator().manual_seed(n + k)
    wide = _nan((n, k + 8))
    w = torch.randn(n, k, generator=g) * torch.exp2(torch.randint(-30, 10, (n, 1), generator=g).float())
    w[n // 2] = 0.0
    wide[:, 4:4 + k] = w.cuda()
    view = wide[:, 4:4 + k]
    for name, other in _amax_cases(view.contiguous()).items():
        both, cs2 = _lib.split_rows_scaled(view, other, k_pad=k_pad, ldo=k_pad + 8, out=_nan((2, n, k_pad + 8), torch.float16),
                                           col_scale=_nan((n,)))
        one, cs1 = _lib.cast_rows_scaled(view, other, k_pad=k_pad, ldo=k_pad + 8, out=_nan((1, n, k_pad + 8), torch.float16),
                                         col_scale=_nan((n,)))
        torch.cuda.synchronize()
        assert torch.equal(_h16(one[0]), _h16(both[0])), name
        assert torch.equal(cs1.view(torch.int32), cs2.view(torch.int32)) and bool(torch.isfinite(cs1).all()), name
        assert bool((_h16(one[0, :, k:k_pad]) == 0).all()) and bool((_h16(one[0, :, k_pad:]) == NAN16).all()), name
        assert bool((_h16(one[0, n // 2, :k_pad]) == 0).all()), name
        if name in ("zero", "inf", "denormal", "none"):
            assert float(cs1[n // 2]) == 1.0, name  # both scales 1


def test_cast_kernels_refuse_what_their_twins_refuse():
    """The DCA_ARG list of dca_split_planes_scaled / dca_split_rows_scaled (tests/test_train_operands_hip.py) without the low plane:
    -1, `bad argument: `, nothing written; the same calls with good arguments go through."""
    from deepcubea_amd import _lib
    _lib.require_gpu()
    L = _lib.lib()
    i64 = C.c_int64
    st = _lib.stream_ptr()
    x = torch.ones(16, 64, device="cuda")
    word = torch.full((1,), 0x3F800000, dtype=torch.int32, device="cuda")
    plane = _nan((16, 136), torch.float16)
    cs = torch.full((16,), -7.0, device="cuda")

    def planes_(xx=x, xoff=0, m=16, n=64, ld=64, h=plane, hoff=0, ldo=136, n_pad=128):
        return L.dca_cast_planes_scaled(_p(xx, xoff), i64(m), i64(n), i64(ld), _p(word), _p(h, hoff), i64(ldo), i64(n_pad), st)

    def rows_(ww=x, woff=0, n=16, k=64, ld=64, h=plane, hoff=0, ldo=136, k_pad=128, c=cs):
        return L.dca_cast_rows_scaled(_p(ww, woff), i64(n), i64(k), i64(ld), _p(h, hoff), i64(ldo), i64(k_pad), _p(c), _p(word), st)

    bad = [
        ("planes n % 4", lambda: planes_(n=62)), ("planes n < 4", lambda: planes_(n=0)), ("planes ld < n", lambda: planes_(ld=60)),
        ("planes ld % 4", lambda: planes_(n=60, ld=62)), ("planes m < 0", lambda: planes_(m=-1)),
        ("planes n_pad < n", lambda: planes_(n_pad=60)), ("planes n_pad % 4", lambda: planes_(n_pad=126)),
        ("planes ldo < n_pad", lambda: planes_(ldo=124)), ("planes ldo % 4", lambda: planes_(ldo=134)),
        ("planes misaligned x", lambda: planes_(xoff=4, m=15)), ("planes misaligned out", lambda: planes_(hoff=2, m=15)),
        ("planes null x", lambda: planes_(xx=None)), ("planes null out_h", lambda: planes_(h=None)),
        ("rows k % 4", lambda: rows_(k=62)), ("rows k < 4", lambda: rows_(k=0)), ("rows ld < k", lambda: rows_(ld=60)),
        ("rows ld % 4", lambda: rows_(k=60, ld=62)), ("rows n < 0", lambda: rows_(n=-1)), ("rows n >= 2^31", lambda: rows_(n=2 ** 31)),
        ("rows k_pad < k", lambda: rows_(k_pad=60)), ("rows k_pad % 4", lambda: rows_(k_pad=126)),
        ("rows ldo < k_pad", lambda: rows_(ldo=124)), ("rows ldo % 4", lambda: rows_(ldo=134)),
        ("rows misaligned w", lambda: rows_(woff=4, n=15)), ("rows misaligned out", lambda: rows_(hoff=2, n=15)),
        ("rows null w", lambda: rows_(ww=None)), ("rows null out_h", lambda: rows_(h=None)), ("rows null col_scale", lambda: rows_(c=None)),
    ]
    for what, call in bad:
        assert call() == -1, what
        assert L.dca_last_error().decode().startswith("bad argument: "), what
    torch.cuda.synchronize()
    assert bool((_h16(plane) == NAN16).all()) and torch.equal(cs.cpu(), torch.full((16,), -7.0))
    assert planes_(m=0) == 0 and rows_(n=0) == 0  # nothing to do
    torch.cuda.synchronize()
    assert bool((_h16(plane) == NAN16).all()) and torch.equal(cs.cpu(), torch.full((16,), -7.0))
    assert planes_() == 0 and rows_() == 0
    torch.cuda.synchronize()
    assert float(plane[0, 0]) == 2.0 ** 14 and float(plane[0, 64]) == 0.0 and float(cs[0]) == 2.0 ** -28


# ------------------------------------------------------------------------------ 6. linear_train(..., gemm="f16")
@pytest.mark.parametrize("m,n,k", [(300, 132, 68), (1000, 324, 200)])
def test_linear_train_f16_y_and_dx_inside_the_bound_and_the_rest_untouched(m, n, k):
    """x, W and dy each within 2^-9.9 of their largest element (normal high planes in both contractions): y inside the bound of
    test_real_data_through_the_cast_kernels_stays_inside_the_derived_bound, dx inside the same bound with the contraction over n and
    no bias term.  With wgrad = "library", dW and db are bit-equal to the default mode's for the same x and dy; gemm = "f16x3" passed
    explicitly is bit-equal to passing nothing."""
    from deepcubea_amd import _lib
    _lib.require_gpu()
    g = torch.Generator().manual_seed(m + n + k)
    lin = torch.nn.Linear(k, n)
    with torch.no_grad():
        lin.weight.copy_(_spread((n, k), g, 0.5))
        lin.bias.copy_(torch.randn(n, generator=g))
    lin = lin.cuda()
    x, dy = _spread((m, k), g, 3.0).cuda(), _spread((m, n), g, 1e-4).cuda()

    def run(**kw):
        lin.zero_grad()
        leaf = x.clone().requires_grad_(True)
        y = _lib.linear_train(leaf, lin, "library", **kw)
        y.backward(dy)
        return y.detach(), leaf.grad, lin.weight.grad.clone(), lin.bias.grad.clone()

    ours, base, named = run(gemm="f16"), run(), run(gemm="f16x3")
    for a, b in zip(named, base):
        assert torch.equal(a.view(torch.int32), b.view(torch.int32))
    assert torch.equal(ours[2].view(torch.int32), base[2].view(torch.int32)), "dW"
    assert torch.equal(ours[3].view(torch.int32), base[3].view(torch.int32)), "db"
    w64 = lin.weight.detach().double()
    err_y = (ours[0].double() - (x.double() @ w64.t() + lin.bias.detach().double()[None, :])).abs()
    bound_y = _f16_bound(x, lin.weight.detach(), lin.bias.detach(), _pad64(k))
    err_dx = (ours[1].double() - dy.double() @ w64).abs()
    bound_dx = _f16_bound(dy, lin.weight.detach().t(), None, _pad64(n))
    print("TRAIN_GEMM linear_train (%d, %d, %d): worst err / bound y %.3g dx %.3g"
          % (m, n, k, float((err_y / bound_y).max()), float((err_dx / bound_dx).max())))
    assert bool(torch.isfinite(ours[0]).all()) and bool(torch.isfinite(ours[1]).all())
    assert bool((err_y <= bound_y).all()), float((err_y / bound_y).max())
    assert bool((err_dx <= bound_dx).all()), float((err_dx / bound_dx).max())
    assert not torch.equal(ours[0], base[0]), "the mode is a different arithmetic"


# ------------------------------------------------------------------------------ 7. whole step, derived part
@pytest.fixture(scope="module")
def tool():
    return _parity_tool()


@pytest.fixture(scope="module")
def small_step_data(tool):
    from deepcubea_amd import _lib
    _lib.require_gpu()
    x, y = tool.small_data()
    return x, y, tool.small_net(11).state_dict()


@pytest.fixture(scope="module")
def reference_steps(tool, small_step_data):
    """The float64 step and the default step at network seed 11: computed once, shared, never changed."""
    x, y, sd = small_step_data
    return tool.step(x, y, sd, "float64"), tool.step(x, y, sd, "f16x3", "library")


@pytest.mark.parametrize("wgrad", ["library", "f16x3", "f16"])
def test_whole_step_f16_every_linear_forward_inside_the_bound_of_its_own_operands(tool, small_step_data, wgrad, monkeypatch):
    """train_gemm = "f16" with each wgrad mode: every gradient finite; each of the six Linears' y against float64 of THAT layer's own
    x, W and b (caught where linear_train hands them over, by a spy that forwards `gemm` as well).  The bound is the one-product
    bound plus what real activations and weights add: an element below 2^-10 of its tensor's (x) or row's (W) largest lands in the
    subnormal range of the scaled high plane, where rounding is off by at most d = 2^-25 / 2^e absolutely instead of 2^-11
    relatively (exact zeros — ReLU's — stay exact).  With |hi(v) - v| <= u |v| + d a product differs by at most
    (2u + u^2) |x||w| + (1 + u)(d_x |w| + d_w |x|) + d_x d_w, summed over k."""
    from deepcubea_amd import _lib
    caught, real = [], _lib.linear_train

    def spy(x, lin, wgrad="library", gemm="f16x3"):
        y = real(x, lin, wgrad, gemm=gemm)
        caught.append({"lin": lin, "x": x.detach(), "y": y.detach(), "gemm": gemm, "wgrad": wgrad})
        return y

    monkeypatch.setattr(_lib, "linear_train", spy)
    x, y, sd = small_step_data
    _, grads, net = tool.step(x, y, sd, "f16", wgrad)
    assert len(caught) == 6 and all(rec["gemm"] == "f16" and rec["wgrad"] == wgrad for rec in caught)
    assert all(bool(torch.isfinite(g).all()) for g in grads.values())

    def slack(amax):  # d = half a subnormal spacing of fp16 (2^-25) in units of the unscaled values whose largest is amax
        return 2.0 ** -25 / torch.exp2(14.0 - torch.floor(torch.log2(amax)))

    for rec in caught:
        lin, xl = rec["lin"], rec["x"].double()
        w, b = lin.weight.detach().double(), lin.bias.detach().double()
        k = w.shape[1]
        d_x = float(slack(xl.abs().max()))
        d_w = slack(w.abs().amax(1))  # [n]
        bound = (_f16_bound(xl, w, b, _pad64(k)) + (1.0 + U16) * (d_x * w.abs().sum(1)[None, :] + d_w[None, :] * xl.abs().sum(1)[:, None])
                 + k * d_x * d_w[None, :])
        err = (rec["y"].double() - (xl @ w.t() + b[None, :])).abs()
        worst = float((err / bound.clamp_min(1e-300)).max())
        print("TRAIN_GEMM STEP f16 / wgrad %s %s: worst err / bound %.3g" % (wgrad, tuple(w.shape), worst))
        assert bool((err <= bound).all()), (tuple(w.shape), worst)


def test_default_mode_still_takes_a_spy_with_the_old_signature(tool, small_step_data, reference_steps, monkeypatch):
    from deepcubea_amd import _lib
    calls, real = [], _lib.linear_train

    def spy(x, lin, wgrad="library"):
        calls.append(wgrad)
        return real(x, lin, wgrad)

    monkeypatch.setattr(_lib, "linear_train", spy)
    x, y, sd = small_step_data
    loss, grads, _ = tool.step(x, y, sd, "f16x3", "library")
    assert calls == ["library"] * 6
    assert loss == reference_steps[1][0] and all(bool(torch.isfinite(g).all()) for g in grads.values())


# ------------------------------------------------------------------------------ 8. whole step, measured part
# profiles/train_gemm_parity.txt, "worst of 3 seeds" rows: (|loss - loss64| / |loss64|, worst max|g - g64| / max|g64|)
MEASURED_STEP = {
    "library": (7.515e-06, 1.358e-01),
    "f16": (7.515e-06, 1.358e-01),
}


@pytest.mark.parametrize("wgrad", ["library", "f16"])
def test_whole_step_f16_against_float64_stays_within_four_times_the_measured_distance(tool, small_step_data, reference_steps, wgrad):
    """The loss and every parameter's gradient of the f16 step against the same step in float64 — the reference's arithmetic at
    double precision.  No tolerance can be derived through ten BatchNorms, so the distance was MEASURED on the MI355X for network
    seeds 11, 12, 13 (profiles/train_gemm_parity.txt, written by tools/train_gemm_parity.py, which also lists the default f16x3
    step as the yardstick); the seed-11 values asserted here stay within 4x the worst of the three — the factor covers the
    seed-to-seed variation of a rounding-error maximum.  Parameters with an analytically zero gradient (Linear biases in front of
    a BatchNorm) are held to 4x the default step's noise."""
    x, y, _ = small_step_data
    mt = tool.step_metrics(x, y, 11, "f16", wgrad, reference_steps[0], reference_steps[1])
    worst_loss, worst_grad = MEASURED_STEP[wgrad]
    print("TRAIN_GEMM PARITY f16 / wgrad %s: loss %.3e (measured worst %.3e)  grad %.3e at %s (measured worst %.3e)  noise %.3g"
          % (wgrad, mt["loss"], worst_loss, mt["grad"], mt["which"], worst_grad, mt["noise"]))
    assert mt["finite"]
    assert mt["loss"] <= 4.0 * worst_loss, (mt["loss"], worst_loss)
    assert all(v <= 4.0 * worst_grad for v in mt["per"].values()), (mt["which"], mt["grad"], worst_grad)
    assert mt["noise"] <= 4.0, mt["noise"]


# ------------------------------------------------------------------------------ 9. train_nnet
def test_train_nnet_three_iterations_in_each_pair_of_modes(tool, small_step_data):
    from deepcubea_amd.utils import nnet_utils
    x, y, sd = small_step_data
    for gemm in ("f16x3", "f16"):
        for wgrad in ("library", "f16x3", "f16"):
            net = tool.small_net()
            net.load_state_dict(sd)
            net = net.cuda().set_train_gemm(gemm).set_wgrad(wgrad)
            np.random.seed(3)
            random.seed(3)
            last = nnet_utils.train_nnet(net, x, y.view(-1, 1), torch.device("cuda"), 256, 3, 0, 1e-3, 0.9999993, display=False)
            assert math.isfinite(last) and int(net.bn1.num_batches_tracked) == 3, (gemm, wgrad)
            assert all(bool(torch.isfinite(p).all()) for p in net.parameters()), (gemm, wgrad)


MEASURED_RUN_RATIO = 1.0090  # profiles/train_gemm_parity.txt, "worst ratio of 5 seeds"


def test_sixty_adam_steps_end_no_further_from_the_default_run_than_measured(tool, small_step_data):
    """60 Adam steps of batch 256 on the 512 states from identical weights, batches and seeds in f16x3 and f16 mode: the final
    loss of the f16 run over the f16x3 run's is at most 2x the worst ratio measured over batch seeds 1-5 on the MI355X
    (profiles/train_gemm_parity.txt).  Two fp32 runs already drift apart at the rounding level, so the ratio is
    measured against the default mode and never against a constant invented here."""
    x, y, sd = small_step_data
    ratio, ours, base = tool.short_run_ratio(x, y, sd, 3)
    print("TRAIN_GEMM RUN seed 3: f16 %.6f f16x3 %.6f ratio %.4f (measured worst %.4f)" % (ours, base, ratio, MEASURED_RUN_RATIO))
    assert math.isfinite(ours) and math.isfinite(base)
    assert ratio <= 2.0 * MEASURED_RUN_RATIO, (ratio, MEASURED_RUN_RATIO)


# ------------------------------------------------------------------------------ 10. with --l1_train embed
@pytest.mark.parametrize("wgrad", ["library", "f16"])
def test_embed_layer_1_is_not_touched(wgrad, monkeypatch):
    """puzzle15 with l1_train = "embed" and train_gemm = "f16": linear_train sees the nine other Linears only, fc1's forward is
    bit-equal to the default GEMM mode's, and fc1's gradient is the scatter's own: bit-equal to dca_l1_embed_wgrad run again on
    the gradient that arrived at fc1's output.  (Bit-equality of fc1's gradient BETWEEN the two GEMM modes cannot hold and is not
    asked: the gradient that arrives at fc1 has come back through fc2's and the blocks' input-gradient GEMMs, which are what the
    mode changes.  What the mode must leave alone is fc1's own arithmetic, and that is what is compared.)"""
    from deepcubea_amd import _lib
    from deepcubea_amd.utils import env_utils
    from deepcubea_amd.utils.synthetic_weights import load_synthetic_weights
    _lib.require_gpu()
    env_id, dim = _lib.env_ids("puzzle15")[:2]
    states, nb, _ = _lib.generate_states(env_id, dim, 512, 0, 30, 5, 0)
    x, y = _lib.nnet_input(env_id, dim, states), nb.float().contiguous()
    seen, arrived, pre1, real, real_embed, real_scatter = [], [], [], _lib.linear_train, _lib.l1_embed_train, _lib.l1_embed_wgrad

    def spy(t, lin, wgrad="library", gemm="f16x3"):
        seen.append((tuple(lin.weight.shape), gemm))
        return real(t, lin, wgrad, gemm=gemm)

    def embed_spy(states_nnet, lin, depth):
        out = real_embed(states_nnet, lin, depth)
        pre1.append(out.detach().clone())
        return out

    def scatter_spy(states_nnet, dy, depth, want_bias=True):
        arrived.append(dy.detach().clone())
        return real_scatter(states_nnet, dy, depth, want_bias=want_bias)

    monkeypatch.setattr(_lib, "linear_train", spy)
    monkeypatch.setattr(_lib, "l1_embed_train", embed_spy)
    monkeypatch.setattr(_lib, "l1_embed_wgrad", scatter_spy)

    def step(gemm):
        del seen[:]
        net = env_utils.get_environment("puzzle15").get_nnet_model()
        load_synthetic_weights(net, 2024)
        net = net.cuda().train().set_l1_train("embed").set_wgrad(wgrad).set_train_gemm(gemm)
        torch.nn.functional.mse_loss(net(x)[:, 0], y).backward()
        return net, list(seen)

    base, seen_base = step("f16x3")
    ours, seen_ours = step("f16")
    shapes = sorted([(1000, 5000)] + [(1000, 1000)] * 8)
    assert sorted(s for s, _ in seen_base) == shapes and all(g == "f16x3" for _, g in seen_base)
    assert sorted(s for s, _ in seen_ours) == shapes and all(g == "f16" for _, g in seen_ours)
    assert len(pre1) == 2 and torch.equal(pre1[0], pre1[1]), "fc1's forward does not know the mode"
    assert len(arrived) == 2
    for net, dy in zip((base, ours), arrived):
        dw, db = real_scatter(x, dy, net.one_hot_depth)
        assert torch.equal(net.fc1.weight.grad, dw) and torch.equal(net.fc1.bias.grad, db)
    assert all(bool(torch.isfinite(p.grad).all()) for p in ours.parameters())
    print("TRAIN_GEMM EMBED wgrad %s: fc1 gradient between the GEMM modes: max |diff| %.3g of max %.3g"
          % (wgrad, float((ours.fc1.weight.grad - base.fc1.weight.grad).abs().max()), float(base.fc1.weight.grad.abs().max())))
