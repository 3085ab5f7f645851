"""GPU tests of the training step's weight gradient on dca_wgrad_f16 (`--wgrad f16x3 | f16`; csrc/dca_wgrad.hip): dW = dy^T . x
from the fp16 planes, fragments read with the transposing LDS read, rows cut into wgrad_splits(m, n, k) slices.

Outputs and workspaces are NaN-filled before every call; what the kernel must not write has to keep the fill.  Integer planes make
every partial sum an integer below 2^24, so the fp32 result is exact in any order and a difference is a wiring error."""
import ctypes as C
import math
import random
import re

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu
NOISE = re.compile(r"(fc1|fc2|blocks\.\d\.[02])\.bias")  # a Linear bias in front of a BatchNorm: analytically zero gradient
U16 = 2.0 ** -11  # unit roundoff of an fp16 high plane: k_split_planes_scaled converts with (_Float16)v, round to nearest even


def _pad64(v):
    return (v + 63) // 64 * 64


def _nan(shape, dtype=torch.float32):
    return torch.full(shape, float("nan"), dtype=dtype, device="cuda")


def _p(t, off=0):
    return C.c_void_p(0 if t is None else t.data_ptr() + off)


def _int_planes(m, width, extra, hi_lim, lo_lim, gen):
    """(planes [2, m, ld] fp16 on the device, high int64 [m, width], low int64 [m, width]): integers in the live columns, zeros up
    to pad64(width) — the kernel reads those — and NaN in the `extra` columns beyond, which it must never read."""
    ld = _pad64(width) + extra
    hi = torch.randint(-hi_lim, hi_lim + 1, (m, width), generator=gen)
    lo = torch.randint(-lo_lim, lo_lim + 1, (m, width), generator=gen)
    planes = torch.zeros((2, m, ld), dtype=torch.float16)
    planes[:, :, _pad64(width):] = float("nan")
    planes[0, :, :width] = hi.to(torch.float16)
    planes[1, :, :width] = lo.to(torch.float16)
    return planes.cuda(), hi, lo


def _word(value):
    """A device word holding the bits of fp32 `value` (an amax word), and the exponent e of the scale 2^e it stands for."""
    bits = int(np.float32(value).view(np.uint32))
    ex = ((bits >> 23) & 0xFF) - 127
    e = 0 if (ex < -100 or ex > 100) else 14 - ex
    return torch.tensor([bits], dtype=torch.int64).to(torch.int32).cuda(), e


def _raw_call(dyp, xp, m, n, k, products, amax_dy=None, amax_x=None, dw_cols=12, dw_off=4, ws_slack=0, low=True):
    """dca_wgrad_f16 through ctypes on NaN-filled output and workspace -> (rc, dW window [n, k], whole dW buffer, workspace)."""
    from deepcubea_amd import _lib
    buf = _nan((n, k + dw_cols))
    need = _lib.wgrad_workspace_bytes(m, n, k)
    ws = _nan((need // 4 + ws_slack,)) if need else None
    rc = _lib.lib().dca_wgrad_f16(_p(dyp[0]), _p(dyp[1]) if low else None, dyp.shape[2], _p(xp[0]), _p(xp[1]) if low else None,
                                  xp.shape[2], m, n, k, _p(amax_dy), _p(amax_x), products, _p(buf, 4 * dw_off), buf.shape[1],
                                  _p(ws), need, _lib.stream_ptr())
    torch.cuda.synchronize()
    return rc, buf[:, dw_off:dw_off + k], buf, ws


def _only_window_written(buf, k, dw_off=4):
    mask = torch.ones_like(buf, dtype=torch.bool)
    mask[:, dw_off:dw_off + k] = False
    return bool(torch.isnan(buf[mask]).all()) and not bool(torch.isnan(buf[:, dw_off:dw_off + k]).any())


def _row_counts(n, k):
    """Batch sizes for one (n, k): the fixed list, both sides of one K-tile (31 / 32 / 33) and — from wgrad_splits itself — both
    sides of the first row count that takes two slices and of the first that takes three, plus ragged last slices."""
    from deepcubea_amd import _lib
    ms = {1, 7, 31, 32, 33, 64, 100, 257}
    two = next(m for m in range(1, 4097) if _lib.wgrad_splits(m, n, k) == 2)
    three = next(m for m in range(two, 4097) if _lib.wgrad_splits(m, n, k) >= 3)
    ms |= {two - 1, two, two + 37, three - 1, three, three + 75, 1000}
    return sorted(ms)


# ------------------------------------------------------------------------------ 1. exact on integers, 2. the scale
@pytest.mark.parametrize("n,k", [(4, 4), (64, 64), (68, 132), (128, 128), (132, 260), (260, 68)])
def test_integer_planes_are_exact_in_both_modes_and_the_scale_is_a_power_of_two(n, k):
    """High planes integers in [-8, 8], low planes in [-3, 3], amax NULL: products = 3 must equal dyh.xh + dyh.xl + dyl.xh (no lo.lo
    term) and products = 1 dyh.xh, computed in int64 on the host, bit for bit.  Every partial sum is an integer below
    112 m <= 458 752 < 2^24 (m <= 4096): summation order cannot show.  Row strides exceed the widths (NaN beyond pad64), dW is a
    column window at a 16-byte offset of a wider NaN-filled matrix.  With both amax words set the result is the unscaled one times
    2^-(e_dy + e_x), bit for bit."""
    from deepcubea_amd import _lib
    _lib.require_gpu()
    gen = torch.Generator().manual_seed(1000 * n + k)
    seen = set()
    for m in _row_counts(n, k):
        S = _lib.wgrad_splits(m, n, k)
        seen.add(min(S, 3))
        dyp, dyh, dyl = _int_planes(m, n, 8, 8, 3, gen)
        xp, xh, xl = _int_planes(m, k, 16, 8, 3, gen)
        want = {3: dyh.t() @ xh + dyh.t() @ xl + dyl.t() @ xh, 1: dyh.t() @ xh}
        assert int(want[3].abs().max()) < 2 ** 24
        for products in (3, 1):
            rc, dw, buf, ws = _raw_call(dyp, xp, m, n, k, products)
            assert rc == 0, _lib.lib().dca_last_error()
            assert _only_window_written(buf, k), (m, products)
            assert torch.equal(dw.cpu().double(), want[products].double()), (m, S, products)
            assert (ws is None) == (S == 1)
            if ws is not None:  # the partial tiles: S slabs [n][k], every element written
                assert not bool(torch.isnan(ws).any())
        if m in (33, 257, 1000):
            (w_dy, e_dy), (w_x, e_x) = _word(3.0e-5), _word(700.0)
            assert (e_dy, e_x) == (30, 5)
            rc, dw, buf, _ = _raw_call(dyp, xp, m, n, k, 3, w_dy, w_x)
            assert rc == 0 and _only_window_written(buf, k)
            assert torch.equal(dw.cpu().double(), want[3].double() * 2.0 ** -(e_dy + e_x)), m
            (w_zero, e_zero) = _word(0.0)  # an amax word of zero stands for scale 1 (pow2_scale_of)
            rc, dw, _, _ = _raw_call(dyp, xp, m, n, k, 1, w_zero, w_x, low=False)
            assert rc == 0 and e_zero == 0 and torch.equal(dw.cpu().double(), want[1].double() * 2.0 ** -e_x), m
    assert seen == {1, 2, 3}, "one slice, two slices and three or more all occur"


# ------------------------------------------------------------------------------ 3. launch-to-launch determinism
def _random_case(m, n, k, seed, spread=None):
    """fp32 dy [m, n] (rows over 20 binades) and x = 2 relu(randn) [m, k] on the device — the recipe of
    test_linear_train_is_fp32_accurate_forward_and_backward — or, with `spread`, both within 2^-spread of their largest element."""
    g = torch.Generator().manual_seed(seed)
    if spread is None:
        x = torch.relu(torch.randn(m, k, generator=g)) * 2.0
        dy = torch.randn(m, n, generator=g) * 1e-7
        dy *= torch.exp2(-20.0 * torch.rand(m, 1, generator=g))
    else:
        sign = lambda shape: torch.randint(0, 2, shape, generator=g).float() * 2.0 - 1.0
        x = sign((m, k)) * 3.0 * torch.exp2(-spread * torch.rand(m, k, generator=g))
        dy = sign((m, n)) * 1e-4 * torch.exp2(-spread * torch.rand(m, n, generator=g))
    return dy.cuda(), x.cuda()


def _planes_of(v):
    from deepcubea_amd import _lib
    amax = _lib.absmax_bits(v)
    return _lib.split_planes_scaled(v, amax, n_pad=_pad64(v.shape[1])), amax


@pytest.mark.parametrize("m", [200, 1000])
def test_two_launches_give_the_same_bits(m):
    from deepcubea_amd import _lib
    _lib.require_gpu()
    n, k = 132, 260
    assert (_lib.wgrad_splits(m, n, k) == 1) == (m == 200)
    dy, x = _random_case(m, n, k, 5)
    (dyp, a_dy), (xp, a_x) = _planes_of(dy), _planes_of(x)
    for products in (3, 1):
        first = _lib.wgrad_f16(dyp, xp, n, k, a_dy, a_x, products, out=_nan((n, k)))
        second = _lib.wgrad_f16(dyp, xp, n, k, a_dy, a_x, products, out=_nan((n, k)))
        assert bool(torch.isfinite(first).all()) and torch.equal(first.view(torch.int32), second.view(torch.int32))


# ------------------------------------------------------------------------------ 4. random data, products = 3, through linear_train
@pytest.mark.parametrize("m,n,k", [(300, 132, 68), (777, 256, 512), (1000, 324, 200)])
def test_f16x3_mode_is_fp32_accurate_and_leaves_y_dx_db_alone(m, n, k):
    """linear_train(..., wgrad="f16x3") on the data of test_linear_train_is_fp32_accurate_forward_and_backward (rows of dy over 20
    binades, x = 2 relu(randn)): dW as close to float64 as the library's fp32 product on the same data, by that test's criterion
    e_ours <= max(4 e_lib, 2e-7 max|dW64|); y, dx and db bit-equal to "library" mode's."""
    from deepcubea_amd import _lib
    _lib.require_gpu()
    g = torch.Generator().manual_seed(m + k + n)
    lin = torch.nn.Linear(k, n)
    with torch.no_grad():
        lin.weight.copy_(torch.randn(n, k, generator=g) / k ** 0.5)
        lin.weight[::7] *= 1e-3
        lin.bias.copy_(torch.randn(n, generator=g))
    lin = lin.cuda()
    dy, x = _random_case(m, n, k, m + k + n + 1)
    dw64 = dy.double().t() @ x.double()

    def run(fn):
        lin.zero_grad()
        leaf = x.clone().requires_grad_(True)
        y = fn(leaf)
        y.backward(dy)
        return y.detach(), leaf.grad, lin.weight.grad.clone(), lin.bias.grad.clone()

    ours = run(lambda t: _lib.linear_train(t, lin, wgrad="f16x3"))
    base = run(lambda t: _lib.linear_train(t, lin, wgrad="library"))
    lib32 = run(lambda t: torch.nn.functional.linear(t, lin.weight, lin.bias))
    for name, a, b in zip(("y", "dx", "dw", "db"), ours, base):
        if name != "dw":
            assert torch.equal(a.view(torch.int32), b.view(torch.int32)), name
    e_ours, e_lib = float((ours[2].double() - dw64).abs().max()), float((lib32[2].double() - dw64).abs().max())
    scale = float(dw64.abs().max())
    print("WGRAD f16x3 (%d, %d, %d): e_ours %.3g e_lib %.3g max|dW64| %.3g" % (m, n, k, e_ours, e_lib, scale))
    assert bool(torch.isfinite(ours[2]).all())
    assert e_ours <= max(4.0 * e_lib, 2e-7 * scale), (e_ours, e_lib, scale)


# ------------------------------------------------------------------------------ 5. random data, products = 1
def _f16_bound(dy, x, m):
    """Elementwise bound of the one-product mode against float64, for data whose scaled high planes are all NORMAL fp16 numbers:
    each operand carries one rounding to nearest of relative size u = 2^-11 (k_split_planes_scaled: (_Float16)(v * 2^e), the
    power-of-two scale is exact), so a product is off by at most (2 u + u^2) |dy| |x|; the fp32 accumulation of m terms in any
    order, the fold of the slices and the final scaling add at most (m + 2) 2^-24 of sum |dy| |x|."""
    return (2.0 * U16 + U16 ** 2 + (m + 2) * 2.0 ** -24) * (dy.double().abs().t() @ x.double().abs())


@pytest.mark.parametrize("m,n,k", [(300, 132, 68), (1000, 324, 200)])
def test_f16_mode_stays_inside_its_derived_bound(m, n, k):
    """products = 1 on data within 2^-9.9 of its largest element (inside the 2^10 the scaled high plane holds as normal numbers:
    the largest element goes to [2^14, 2^15), the smallest stays above 2^4): |dW - dW64| <= (2 * 2^-11 + 2^-22 + (m + 2) 2^-24)
    (|dy|^T |x|) elementwise."""
    from deepcubea_amd import _lib
    _lib.require_gpu()
    dy, x = _random_case(m, n, k, 11 * m + n, spread=9.9)
    (dyp, a_dy), (xp, a_x) = _planes_of(dy), _planes_of(x)
    assert float(dyp[0, :, :n].float().abs().min()) >= 16.0 and float(xp[0, :, :k].float().abs().min()) >= 16.0  # normal, by far
    dw = _lib.wgrad_f16(dyp[:1].contiguous(), xp[:1].contiguous(), n, k, a_dy, a_x, 1, out=_nan((n, k)))
    err = (dw.double() - dy.double().t() @ x.double()).abs()
    bound = _f16_bound(dy, x, m)
    print("WGRAD f16 (%d, %d, %d): worst err / bound %.3g" % (m, n, k, float((err / bound).max())))
    assert bool(torch.isfinite(dw).all()) and bool((err <= bound).all()), float((err / bound).max())


# ------------------------------------------------------------------------------ 6. refusals
def test_every_refusal_raises_and_leaves_the_output_alone():
    from deepcubea_amd import _lib
    _lib.require_gpu()
    L = _lib.lib()
    m, n, k = 600, 8, 8  # three slices: a workspace is needed
    assert _lib.wgrad_splits(m, n, k) == 3
    need = _lib.wgrad_workspace_bytes(m, n, k)
    dyp = torch.zeros((2, m, 72), dtype=torch.float16, device="cuda")
    xp = torch.zeros((2, m, 72), dtype=torch.float16, device="cuda")
    dw, ws = _nan((n, 16)), _nan((need // 4 + 4,))

    def call(dyh=_p(dyp[0]), dyl=_p(dyp[1]), ld_dy=72, xh=_p(xp[0]), xl=_p(xp[1]), ld_x=72, m=m, n=n, k=k, products=3, out=_p(dw),
             ld_dw=16, wsp=_p(ws), wsb=need):
        rc = L.dca_wgrad_f16(dyh, dyl, ld_dy, xh, xl, ld_x, m, n, k, None, None, products, out, ld_dw, wsp, wsb, _lib.stream_ptr())
        _lib.check(rc, "dca_wgrad_f16")

    cases = (dict(products=2), dict(products=0), dict(n=6), dict(k=10), dict(n=0), dict(k=-4), dict(m=0), dict(m=-5),
             dict(ld_dy=56), dict(ld_x=56), dict(n=68), dict(k=68), dict(ld_dy=68), dict(ld_x=76), dict(ld_dw=4),
             dict(dyh=None), dict(xh=None), dict(out=None), dict(dyl=None), dict(xl=None),
             dict(dyh=_p(dyp[0], 8)), dict(dyl=_p(dyp[1], 2)), dict(xh=_p(xp[0], 4)), dict(xl=_p(xp[1], 8)), dict(out=_p(dw, 2)),
             dict(wsp=None), dict(wsb=need - 4), dict(wsb=0), dict(wsp=_p(ws, 2)))
    for kw in cases:
        with pytest.raises(_lib.DcaError):
            call(**kw)
        torch.cuda.synchronize()
        assert bool(torch.isnan(dw).all()) and bool(torch.isnan(ws).all()), kw
    call()  # the same call with nothing wrong goes through (planes of zeros: dW = 0)
    torch.cuda.synchronize()
    assert bool((dw[:, :k] == 0).all()) and bool(torch.isnan(dw[:, k:]).all())
    call(products=1, dyl=None, xl=None)  # the one-product mode takes no low planes


# ------------------------------------------------------------------------------ 7. one whole step against float64
def _small_net():
    from deepcubea_amd.utils.pytorch_models import ResnetModel
    torch.manual_seed(11)
    return ResnetModel(16, 16, 256, 128, 2, 1, True)  # puzzle15's input, h1 256, residual width 128, 2 blocks


def _rel(a, ref):
    return float((a - ref).abs().max()) / max(float(ref.abs().max()), 1e-300)


@pytest.fixture(scope="module")
def small_step_data():
    from deepcubea_amd import _lib
    _lib.require_gpu()
    env_id, dim = _lib.env_ids("puzzle15")[:2]
    states, nb, _ = _lib.generate_states(env_id, dim, 512, 0, 30, 5, 0)
    return _lib.nnet_input(env_id, dim, states), nb.float().contiguous(), _small_net().state_dict()


def _step(data, mode, spy=None):
    """One forward + backward of the small network from the shared weights -> (loss, {param: grad float64 on the host})."""
    x, y, sd = data
    net = _small_net()
    net.load_state_dict(sd)
    net = net.cuda().train()
    if mode == "float64":
        net = net.double()
        onehot = torch.nn.functional.one_hot(x.long(), 16).view(x.shape[0], -1).double()
        loss = torch.nn.functional.mse_loss(net.trunk(onehot)[:, 0], y.double())
    else:
        net.set_wgrad(mode)
        loss = torch.nn.functional.mse_loss(net(x)[:, 0], y)
    loss.backward()
    return float(loss.detach().double()), {k: p.grad.double().cpu() for k, p in net.named_parameters()}, net


def test_whole_step_f16x3_is_as_close_to_float64_as_the_library_step(small_step_data):
    """ResnetModel(16, 16, 256, 128, 2 blocks), batch 512: every parameter gradient of the f16x3 step is as close to float64 as the
    "library" step's (factor 4; floor 2e-7 of the tensor's largest element; analytically-zero gradients within 4x the library
    step's noise) — the rule of tests/test_train_step_hip.py with the library step as the yardstick.  Everything but the Linears'
    weight gradients is bit-equal between the modes: the gradients that flow back do not pass through dW."""
    l64, g64, _ = _step(small_step_data, "float64")
    l_lib, g_lib, _ = _step(small_step_data, "library")
    l_o, g_o, _ = _step(small_step_data, "f16x3")
    assert l_o == l_lib, "the forward pass is the same"
    failures = []
    for key in g64:
        is_w = re.fullmatch(r"(fc1|fc2|blocks\.\d\.[02])\.weight", key) is not None
        if not is_w:
            assert torch.equal(g_o[key], g_lib[key]), key
        if NOISE.fullmatch(key):
            if not float(g_o[key].abs().max()) <= 4.0 * float(g_lib[key].abs().max()):
                failures.append(("zero-gradient " + key, float(g_o[key].abs().max()), float(g_lib[key].abs().max())))
            continue
        e_o, e_l = _rel(g_o[key], g64[key]), _rel(g_lib[key], g64[key])
        if is_w:
            print("WGRAD STEP %s: f16x3 %.3g library %.3g (relative to max|g64|)" % (key, e_o, e_l))
        assert bool(torch.isfinite(g_o[key]).all()), key
        if not e_o <= max(4.0 * e_l, 2e-7):
            failures.append(("grad " + key, e_o, e_l))
    assert not failures, failures


def test_whole_step_f16_every_linear_inside_the_bound_of_its_own_operands(small_step_data, monkeypatch):
    """"f16" mode: every gradient finite; each Linear's weight.grad against float64 of THAT layer's own dy and x (caught where
    linear_train hands them over).  The bound is the one-product bound of test_f16_mode_stays_inside_its_derived_bound plus what
    real activations add: an element below 2^-10 of its tensor's largest lands in the subnormal range of the scaled high plane,
    where rounding to nearest is off by at most d = 2^-25 / 2^e absolutely instead of 2^-11 relatively (exact zeros — ReLU's —
    stay exact).  With |hi(v) - v| <= u |v| + d the products differ by at most (2u + u^2) |dy||x| + (1 + u)(d_dy |x| + d_x |dy|)
    + d_dy d_x, summed over the batch."""
    from deepcubea_amd import _lib
    caught, real = [], _lib.linear_train

    def spy(x, lin, wgrad="library"):
        y = real(x, lin, wgrad)
        rec = {"lin": lin, "x": x.detach()}
        y.register_hook(lambda g, rec=rec: rec.__setitem__("dy", g.detach().clone()))
        caught.append(rec)
        return y

    monkeypatch.setattr(_lib, "linear_train", spy)
    _, grads, net = _step(small_step_data, "f16")
    assert len(caught) == 6 and all(bool(torch.isfinite(g).all()) for g in grads.values())

    def absolute_slack(v):  # d = half a subnormal spacing of fp16 (2^-25) in units of the unscaled tensor
        ex = math.floor(math.log2(float(v.abs().max())))
        return 2.0 ** -25 / 2.0 ** (14 - ex)

    for rec in caught:
        lin, x, dy = rec["lin"], rec["x"].double(), rec["dy"].double()
        m = x.shape[0]
        d_dy, d_x = absolute_slack(dy), absolute_slack(x)
        bound = (_f16_bound(dy, x, m) + (1.0 + U16) * (d_dy * x.abs().sum(0)[None, :] + d_x * dy.abs().sum(0)[:, None])
                 + m * d_dy * d_x)
        err = (lin.weight.grad.double() - dy.t() @ x).abs()
        worst = float((err / bound.clamp_min(1e-300)).max())
        print("WGRAD STEP f16 %s: worst err / bound %.3g" % (tuple(lin.weight.shape), worst))
        assert bool((err <= bound).all()), (tuple(lin.weight.shape), worst)


# ------------------------------------------------------------------------------ 8. train_nnet, 9. with --l1_train embed
def test_train_nnet_three_iterations_in_each_mode(small_step_data, monkeypatch):
    """Three Adam iterations per mode from the same weights and batches: all losses finite, and the FIRST loss bit-equal to
    "library" mode's — the forward pass is the same arithmetic until the first update."""
    from deepcubea_amd.utils import nnet_utils
    x, y, sd = small_step_data
    losses = {}

    class Recording(torch.nn.MSELoss):
        def forward(self, a, b):
            out = super().forward(a, b)
            losses[mode].append(out.detach().clone())
            return out

    monkeypatch.setattr(nnet_utils.nn, "MSELoss", Recording)
    for mode in ("library", "f16x3", "f16"):
        losses[mode] = []
        net = _small_net()
        net.load_state_dict(sd)
        net = net.cuda().set_wgrad(mode)
        np.random.seed(3)
        random.seed(3)
        last = nnet_utils.train_nnet(net, x, y.view(-1, 1), torch.device("cuda"), 256, 3, 0, 1e-3, 0.9999993, display=False)
        vals = [float(v) for v in losses[mode]]
        assert len(vals) == 3 and all(math.isfinite(v) for v in vals) and vals[-1] == last
        assert int(net.bn1.num_batches_tracked) == 3
    for mode in ("f16x3", "f16"):
        assert torch.equal(losses[mode][0], losses["library"][0]), mode


@pytest.mark.parametrize("mode", ["f16x3", "f16"])
def test_embed_layer_1_is_not_touched(mode, monkeypatch):
    """puzzle15 with l1_train = "embed": one step runs, fc1's gradient is the scatter's own — bit-equal to the embed step in
    "library" mode — and the new kernel sees the nine other Linears only."""
    from deepcubea_amd import _lib
    from deepcubea_amd.utils import env_utils
    from deepcubea_amd.utils.synthetic_weights import load_synthetic_weights
    _lib.require_gpu()
    env_id, dim = _lib.env_ids("puzzle15")[:2]
    states, nb, _ = _lib.generate_states(env_id, dim, 512, 0, 30, 5, 0)
    x, y = _lib.nnet_input(env_id, dim, states), nb.float().contiguous()
    shapes, real = [], _lib.wgrad_f16

    def counting(dyp, xp, n, k, *a, **kw):
        shapes.append((n, k))
        return real(dyp, xp, n, k, *a, **kw)

    monkeypatch.setattr(_lib, "wgrad_f16", counting)

    def step(wgrad):
        net = env_utils.get_environment("puzzle15").get_nnet_model()
        load_synthetic_weights(net, 2024)
        net = net.cuda().train().set_l1_train("embed").set_wgrad(wgrad)
        torch.nn.functional.mse_loss(net(x)[:, 0], y).backward()
        return net

    base = step("library")
    assert shapes == []
    ours = step(mode)
    assert sorted(shapes) == sorted([(1000, 5000)] + [(1000, 1000)] * 8)
    assert torch.equal(ours.fc1.weight.grad, base.fc1.weight.grad) and torch.equal(ours.fc1.bias.grad, base.fc1.bias.grad)
    assert all(bool(torch.isfinite(p.grad).all()) for p in ours.parameters())
