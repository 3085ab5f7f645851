"""GPU tests of the training step's dense layers where they run on the hand-written kernels: `_lib.linear_train`'s dispatch rule and
autograd contract, one whole forward + backward of the production networks against float64, and a run recorded from the reference
(tests/golden/train_nnet_b256.npz) whose every trunk Linear goes through dca_f16x3_gemm.

The accuracy criterion is the project's own (test_linear_train_is_fp32_accurate_forward_and_backward): a result is fp32-accurate
when it is as close to float64 as torch's fp32 kernels are, a factor 4 allowed, with a floor of 2e-7 of the largest element."""
import json
import os
import random
import re

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NOISE = re.compile(r"(fc1|fc2|blocks\.\d\.[02])\.bias")  # a Linear bias in front of a BatchNorm: analytically zero gradient


def _takes_kernel(m: int, k: int, n: int) -> bool:
    """The dispatch rule of _lib.linear_train, written down a second time on purpose."""
    return m >= 256 and k >= 64 and k % 4 == 0 and n % 4 == 0


@pytest.fixture
def gemm_calls(monkeypatch):
    """Counts the launches of dca_f16x3_gemm that go through _lib.f16x3_gemm."""
    from deepcubea_amd import _lib
    calls = []
    real = _lib.f16x3_gemm

    def counting(*a, **kw):
        calls.append(tuple(a[0].shape))
        return real(*a, **kw)

    monkeypatch.setattr(_lib, "f16x3_gemm", counting)
    return calls


@pytest.fixture
def library_gemms(monkeypatch):
    """Switches linear_train to the library's GEMMs for one test (restored afterwards)."""
    from deepcubea_amd import _lib

    def switch(on: bool):
        monkeypatch.setattr(_lib, "TRAIN_F16X3", not on)

    return switch


def _assert_fp32_accurate(names, ours, lib32, want):
    for name, o, l, w_ in zip(names, ours, lib32, want):
        if w_ is None:
            assert o is None, name
            continue
        e_ours, e_lib = float((o - w_).abs().max()), float((l - w_).abs().max())
        scale = float(w_.abs().max())
        assert bool(torch.isfinite(o).all()), name
        assert e_ours <= max(4.0 * e_lib, 2e-7 * scale), (name, e_ours, e_lib, scale)


def _lin(k: int, n: int, seed: int, bias: bool = True) -> torch.nn.Linear:
    g = torch.Generator().manual_seed(seed)
    lin = torch.nn.Linear(k, n, bias=bias)
    with torch.no_grad():
        lin.weight.copy_(torch.randn(n, k, generator=g) / k ** 0.5)
        lin.weight[::7] *= 1e-3  # rows of very different magnitude: the per-row scales
        if bias:
            lin.bias.copy_(torch.randn(n, generator=g))
    return lin


def _three_ways(lin, x, dy, x_grad=True, make_x=None, consume=None):
    """forward + backward of `lin` on x with upstream gradient dy: (linear_train, F.linear fp32, float64), each a list
    [y, dx, dw, db] of float64 CPU tensors (None where there is no gradient).  make_x(x_dev) -> the tensor handed to the layer
    (a view, say) and consume(y, dy) -> the scalar to call backward on let the caller choose the call form."""
    from deepcubea_amd import _lib
    ref = torch.nn.Linear(lin.in_features, lin.out_features, bias=lin.bias is not None).double()
    ref.load_state_dict({kk: v.double() for kk, v in lin.state_dict().items()})
    for p, q in zip(ref.parameters(), lin.parameters()):
        p.requires_grad_(q.requires_grad)
    make_x = make_x or (lambda t: t)
    consume = consume or (lambda y, d: (y * d).sum())

    def run(mod, fn, x0, d):
        mod.zero_grad()
        leaf = x0.clone().requires_grad_(x_grad)
        y = fn(make_x(leaf))
        consume(y, d).backward()
        outs = [y.detach(), leaf.grad, mod.weight.grad, mod.bias.grad if mod.bias is not None else None]
        return [None if t is None else t.double().cpu() for t in outs]

    want = run(ref, ref, x.double(), dy.double())
    lin = lin.cuda()
    ours = run(lin, lambda t: _lib.linear_train(t, lin), x.cuda(), dy.cuda())
    lib32 = run(lin, lambda t: torch.nn.functional.linear(t, lin.weight, lin.bias), x.cuda(), dy.cuda())
    return ours, lib32, want


NAMES = ("y", "dx", "dw", "db")


# ------------------------------------------------------------------------------ 2. dispatch
@pytest.mark.parametrize("n", [1, 4, 6, 1000])
@pytest.mark.parametrize("k", [60, 64, 68, 625, 2401])
@pytest.mark.parametrize("m", [255, 256, 257])
def test_dispatch_table_on_both_sides_of_every_threshold(m, k, n, gemm_calls, library_gemms):
    """Which path a layer takes (m >= 256, in_features >= 64, both widths % 4 == 0), how many launches that costs (forward +
    input gradient when x needs one, forward alone when it does not), fp32 accuracy either way, and nothing on the kernel once
    TRAIN_F16X3 is off."""
    from deepcubea_amd import _lib
    _lib.require_gpu()
    g = torch.Generator().manual_seed(1000 * m + 10 * k + n)
    lin = _lin(k, n, m + k + n)
    x = torch.relu(torch.randn(m, k, generator=g)) * 2.0
    dy = torch.randn(m, n, generator=g) * 1e-3
    kernel = _takes_kernel(m, k, n)
    kp = (k + 63) // 64 * 64
    ours, lib32, want = _three_ways(lin, x, dy)
    assert gemm_calls == ([(2, m, kp), (2, m, (n + 63) // 64 * 64)] if kernel else [])
    _assert_fp32_accurate(NAMES, ours, lib32, want)
    del gemm_calls[:]
    ours, lib32, want = _three_ways(lin, x, dy, x_grad=False)
    assert ours[1] is None and gemm_calls == ([(2, m, kp)] if kernel else [])
    _assert_fp32_accurate(NAMES, ours, lib32, want)
    del gemm_calls[:]
    library_gemms(True)
    ours, lib32, want = _three_ways(lin, x, dy)
    assert gemm_calls == []
    _assert_fp32_accurate(NAMES, ours, lib32, want)


@pytest.mark.parametrize("env_name", ["cube3", "puzzle15", "puzzle24", "puzzle35", "puzzle48", "lightsout7"])
def test_which_linears_of_the_registered_networks_take_the_kernel(env_name, gemm_calls):
    """Every Linear of env.get_nnet_model() at batch 10 000: the 5000- and 1000-wide trunk layers take dca_f16x3_gemm, the
    1-wide output layer does not, and of the input layers those with 324 (cube3), 256 (puzzle15) and 1296 (puzzle35) columns do
    while 625 (puzzle24) and 2401 (puzzle48) — not multiples of 4 — stay on the library.  A change of the rule shows up here."""
    from deepcubea_amd import _lib
    from deepcubea_amd.utils import env_utils
    _lib.require_gpu()
    net = env_utils.get_environment(env_name).get_nnet_model()
    in_dim = {"cube3": 324, "puzzle15": 256, "puzzle24": 625, "puzzle35": 1296, "puzzle48": 2401, "lightsout7": 294}[env_name]
    lins = [(name, mod) for name, mod in net.named_modules() if isinstance(mod, torch.nn.Linear)]
    assert [name for name, _ in lins][-3:] == ["fc1", "fc2", "fc_out"] and len(lins) == 11
    table = {}
    for name, lin in lins:
        x = torch.randn(10000, lin.in_features, device="cuda")
        del gemm_calls[:]
        with torch.no_grad():
            y = _lib.linear_train(x, lin.cuda())
        assert tuple(y.shape) == (10000, lin.out_features)
        table[name] = len(gemm_calls)
        assert table[name] == int(_takes_kernel(10000, lin.in_features, lin.out_features)), name
        lin.cpu()
    assert net.fc1.in_features == in_dim
    want = {name: 1 for name, _ in lins}
    want["fc_out"] = 0
    if in_dim in (625, 2401):
        want["fc1"] = 0
    if env_name == "lightsout7":  # 49 lights x 6: 294 = 2 * 147 columns, not a multiple of 4
        want["fc1"] = 0
    assert table == want


# ------------------------------------------------------------------------------ 2. call forms
M, K, N = 517, 324, 136  # ragged rows, K padded 324 -> 384 inside the planes, N padded 136 -> 192 in the input-gradient GEMM


def _data(seed=3, m=M, k=K, n=N):
    g = torch.Generator().manual_seed(seed)
    x = torch.relu(torch.randn(m, k, generator=g)) * 2.0
    dy = torch.randn(m, n, generator=g) * 1e-5 * torch.exp2(-12.0 * torch.rand(m, 1, generator=g))
    return x, dy


def test_x_without_requires_grad_gives_no_dx_and_takes_no_absmax_of_dy(gemm_calls, monkeypatch):
    from deepcubea_amd import _lib
    _lib.require_gpu()
    absmax = []
    real = _lib.absmax_bits
    monkeypatch.setattr(_lib, "absmax_bits", lambda *a, **kw: (absmax.append(1), real(*a, **kw))[1])
    x, dy = _data()
    ours, lib32, want = _three_ways(_lin(K, N, 1), x, dy, x_grad=False)
    assert ours[1] is None and len(gemm_calls) == 1 and len(absmax) == 1  # (the forward's own max|x|; none for dy)
    _assert_fp32_accurate(NAMES, ours, lib32, want)
    del absmax[:], gemm_calls[:]
    ours, lib32, want = _three_ways(_lin(K, N, 1), x, dy, x_grad=True)
    assert len(gemm_calls) == 2 and len(absmax) == 2
    _assert_fp32_accurate(NAMES, ours, lib32, want)


def test_frozen_weight_and_no_bias(gemm_calls):
    from deepcubea_amd import _lib
    _lib.require_gpu()
    x, dy = _data(4)
    lin = _lin(K, N, 2)
    lin.weight.requires_grad_(False)
    ours, lib32, want = _three_ways(lin, x, dy)
    assert ours[2] is None and ours[3] is not None and len(gemm_calls) == 2
    _assert_fp32_accurate(NAMES, ours, lib32, want)
    del gemm_calls[:]
    lin = _lin(K, N, 2, bias=False)
    ours, lib32, want = _three_ways(lin, x, dy)
    assert ours[3] is None and ours[2] is not None and len(gemm_calls) == 2
    _assert_fp32_accurate(NAMES, ours, lib32, want)
    del gemm_calls[:]
    lin = _lin(K, N, 2)
    lin.bias.requires_grad_(False)
    ours, lib32, want = _three_ways(lin, x, dy)
    assert ours[3] is None and len(gemm_calls) == 2
    _assert_fp32_accurate(NAMES, ours, lib32, want)


@pytest.mark.parametrize("form", ["column_slice", "transposed"])
def test_non_contiguous_x(form, gemm_calls):
    from deepcubea_amd import _lib
    _lib.require_gpu()
    g = torch.Generator().manual_seed(8)
    _, dy = _data(5)
    if form == "column_slice":  # x = columns 8 .. 8 + K of a wider tensor whose other columns are large
        x = torch.randn(M, K + 24, generator=g) * 2.0
        x[:, :8] = 1.0e6
        x[:, 8 + K:] = -1.0e6
        make_x = lambda t: t[:, 8:8 + K]  # noqa: E731
    else:
        x = torch.randn(K, M, generator=g) * 2.0
        make_x = lambda t: t.t()  # noqa: E731
    ours, lib32, want = _three_ways(_lin(K, N, 6), x, dy, make_x=make_x)
    assert len(gemm_calls) == 2
    _assert_fp32_accurate(NAMES, ours, lib32, want)
    if form == "column_slice":
        assert float(ours[1][:, :8].abs().max()) == 0.0 and float(ours[1][:, 8 + K:].abs().max()) == 0.0


@pytest.mark.parametrize("form", ["sum_stride0", "transposed_consumer"])
def test_non_contiguous_dy(form, gemm_calls):
    """y.sum().backward() hands backward an expanded (stride-0) gradient; a consumer that transposes y hands it a transposed one."""
    from deepcubea_amd import _lib
    _lib.require_gpu()
    x, dy = _data(7)
    if form == "sum_stride0":
        consume = lambda y, d: y.sum() * 3.0e-4  # noqa: E731
    else:
        consume = lambda y, d: (y.t() * d.t().contiguous()).sum()  # noqa: E731
    ours, lib32, want = _three_ways(_lin(K, N, 9), x, dy, consume=consume)
    assert len(gemm_calls) == 2
    _assert_fp32_accurate(NAMES, ours, lib32, want)


# ------------------------------------------------------------------------------ 2. exact cases
def test_exact_cases_zero_gradient_zero_input_zero_weight_rows():
    from deepcubea_amd import _lib
    _lib.require_gpu()
    x, dy = _data(11)
    lin = _lin(K, N, 12).cuda()
    xd = x.cuda().requires_grad_(True)
    y = _lib.linear_train(xd, lin)
    y.backward(torch.zeros_like(y))  # dy == 0: max|dy| has bits 0, the scale stays 1
    assert bool(torch.isfinite(xd.grad).all()) and float(xd.grad.abs().max()) == 0.0
    assert float(lin.weight.grad.abs().max()) == 0.0
    # x == 0: y is the broadcast bias, bit for bit
    y0 = _lib.linear_train(torch.zeros(M, K, device="cuda"), lin).detach()
    assert torch.equal(y0.view(torch.int32), lin.bias.detach()[None].expand(M, N).contiguous().view(torch.int32))
    # all-zero weight rows: those output columns are their bias, bit for bit; the others are as accurate as ever
    with torch.no_grad():
        lin.weight[[0, 5, N - 1]] = 0.0
    y1 = _lib.linear_train(x.cuda(), lin).detach()
    for c in (0, 5, N - 1):
        assert torch.equal(y1[:, c].view(torch.int32), lin.bias.detach()[c].expand(M).contiguous().view(torch.int32))
    want = torch.nn.functional.linear(x.double(), lin.weight.detach().double().cpu(), lin.bias.detach().double().cpu())
    y32 = torch.nn.functional.linear(x.cuda(), lin.weight, lin.bias).detach()
    _assert_fp32_accurate(("y",), [y1.double().cpu()], [y32.double().cpu()], [want])


def test_post_relu_input_with_ninety_percent_exact_zeros(gemm_calls):
    from deepcubea_amd import _lib
    _lib.require_gpu()
    g = torch.Generator().manual_seed(113)  # (not _data's own seed: the mask would follow the signs)
    x, dy = _data(13)
    x = x * (torch.rand(M, K, generator=g) < 0.2)  # relu left half; a fifth of that survives
    assert float((x == 0).float().mean()) >= 0.88
    ours, lib32, want = _three_ways(_lin(K, N, 14), x, dy)
    assert len(gemm_calls) == 2
    _assert_fp32_accurate(NAMES, ours, lib32, want)


# ------------------------------------------------------------------------------ 2. power-of-two invariance
@pytest.mark.parametrize("p", [-60, -7, 9, 40])
def test_power_of_two_invariance_bit_for_bit(p):
    """The scales are exponent shifts taken from the operand itself, so multiplying an operand by 2^p changes nothing but the
    exponent that comes back through col_scale: with no bias, linear_train(x * 2^p) == linear_train(x) * 2^p bit for bit; the
    same for dx under dy * 2^p, and for one weight row scaled by 2^p with its output column (the other columns do not move)."""
    from deepcubea_amd import _lib
    _lib.require_gpu()
    x, dy = _data(21)
    lin = _lin(K, N, 22, bias=False).cuda()
    f = 2.0 ** p

    def run(xx, dd, layer):
        leaf = xx.cuda().requires_grad_(True)
        y = _lib.linear_train(leaf, layer)
        y.backward(dd.cuda())
        return y.detach(), leaf.grad

    def same(a, b):
        return torch.equal(a.contiguous().view(torch.int32), b.contiguous().view(torch.int32))

    y0, dx0 = run(x, dy, lin)
    assert float(y0.abs().max()) > 0 and float(dx0.abs().max()) > 0
    y1, _ = run(x * f, dy, lin)
    assert same(y1, y0 * f)
    _, dx1 = run(x, dy * f, lin)
    assert same(dx1, dx0 * f)
    lin2 = _lin(K, N, 22, bias=False)
    with torch.no_grad():
        lin2.weight[7] *= f
        lin2.weight[N - 1] *= f
    y2, _ = run(x, dy, lin2.cuda())
    want = y0.clone()
    want[:, 7] *= f
    want[:, N - 1] *= f
    assert same(y2, want)


@pytest.mark.parametrize("mag", [1e-30, 1e30 / 8])
def test_range_limit_inputs_between_2_pow_minus_100_and_2_pow_101(mag, gemm_calls):
    """An operand whose |max| lies in [2^-100, 2^101) is scaled into fp16 range and comes out finite and fp32-accurate: here
    activations and gradients at 1e-30 and at 1.25e29.  Beyond that range the scale is left at 1 BY DESIGN (pow2_scale_of: zero,
    denormal, inf and NaN take the same exit), the planes then flush or overflow, and nothing is promised about the result."""
    from deepcubea_amd import _lib
    _lib.require_gpu()
    g = torch.Generator().manual_seed(31)
    x = torch.randn(M, K, generator=g) * mag
    assert 2.0 ** -100 <= float(x.abs().max()) < 2.0 ** 101
    dy = torch.randn(M, N, generator=g) * 1e-3
    ours, lib32, want = _three_ways(_lin(K, N, 32, bias=False), x, dy)  # (no bias: an O(1) bias would hide y in the criterion)
    assert len(gemm_calls) == 2
    _assert_fp32_accurate(NAMES, ours, lib32, want)
    del gemm_calls[:]
    x2, _ = _data(33)
    dy2 = torch.randn(M, N, generator=g) * mag  # the gradient at the edge of the range, the activations O(1)
    ours, lib32, want = _three_ways(_lin(K, N, 32), x2, dy2)
    assert len(gemm_calls) == 2
    _assert_fp32_accurate(NAMES, ours, lib32, want)


# ------------------------------------------------------------------------------ 3. one whole step against float64
def _plain_trunk(net, x):
    """The network's forward in training mode written out with its own nn.Linear / nn.BatchNorm1d modules: torch's fp32 kernels,
    nothing of this project's on the path (the yardstick; ResnetModel.trunk would take _trunk_train_dev here)."""
    relu = torch.relu
    x = relu(net.bn1(net.fc1(x)))
    x = relu(net.bn2(net.fc2(x)))
    for blk in net.blocks:
        h = relu(blk[1](blk[0](x)))
        x = relu(blk[3](blk[2](h)) + x)
    return net.fc_out(x)


def _one_step(env_name, mode, states, y):
    """One forward + backward from the synthetic weights of seed 2024 -> (loss, {param: grad}, {running stat: value}), float64 CPU."""
    from deepcubea_amd.utils import env_utils
    from deepcubea_amd.utils.synthetic_weights import load_synthetic_weights
    net = env_utils.get_environment(env_name).get_nnet_model()
    load_synthetic_weights(net, 2024)
    net = net.cuda().train()
    onehot = torch.nn.functional.one_hot(states.long(), net.one_hot_depth).view(states.shape[0], -1)
    if mode == "float64":
        net = net.double()
        out = net.trunk(onehot.double())[:, 0]
        loss = torch.nn.functional.mse_loss(out, y.double())
    elif mode == "torch32":
        out = _plain_trunk(net, onehot.float())[:, 0]
        loss = torch.nn.functional.mse_loss(out, y)
    else:
        out = net(states)[:, 0]
        loss = torch.nn.functional.mse_loss(out, y)
    loss.backward()
    grads = {k: p.grad.double().cpu() for k, p in net.named_parameters()}
    stats = {k: v.double().cpu() for k, v in net.state_dict().items() if "running_" in k}
    assert all(int(v) == 8 for k, v in net.state_dict().items() if "num_batches_tracked" in k)
    return float(loss.double()), grads, stats


def _rel(a, ref):
    return float((a - ref).abs().max()) / max(float(ref.abs().max()), 1e-300)


@pytest.mark.parametrize("env_name,batch", [("cube3", 10000), ("puzzle15", 1003)])
def test_whole_step_at_the_production_geometry_against_float64(env_name, batch, gemm_calls, library_gemms):
    """One forward + backward of env.get_nnet_model() (5000 / 1000 / 4 blocks) from identical weights, four ways: float64, plain
    torch fp32 (the yardstick), the device path as shipped, the device path with the library's GEMMs (BatchNorm kernels alone).
    cube3 at batch 10 000 is the training step of the README's headline run; puzzle15 at batch 1003 is a ragged batch with a
    256-wide input.  Loss, every parameter gradient and every running statistic of the two device paths are as close to float64
    as torch's fp32 step is (factor 4; floors: 2^-22 of the loss, 2e-7 of a tensor's largest element).

    Measured on the MI355X (profiles/train_step_parity.txt): see that file for the ratios ours / torch32, worst and median."""
    from deepcubea_amd import _lib
    _lib.require_gpu()
    env_id, dim = _lib.env_ids(env_name)[:2]
    states, nb, _ = _lib.generate_states(env_id, dim, batch, 0, 30, 5, 0)
    x = _lib.nnet_input(env_id, dim, states)
    y = nb.float().contiguous()
    l64, g64, s64 = _one_step(env_name, "float64", x, y)
    l32, g32, s32 = _one_step(env_name, "torch32", x, y)
    assert gemm_calls == []
    shipped = _one_step(env_name, "device", x, y)
    # 10 trunk Linears, forward + input gradient, less the input gradient of fc1 (its input needs none); puzzle15's too: 256 columns
    assert len(gemm_calls) == 19
    again = _one_step(env_name, "device", x, y)
    assert again[0] == shipped[0], "the same step twice gives a bit-identical loss"
    del gemm_calls[:]
    library_gemms(True)
    bn_only = _one_step(env_name, "device", x, y)
    assert gemm_calls == []
    failures = []
    report = {"env": env_name, "batch": batch, "loss_float64": l64, "loss_torch32_err": abs(l32 - l64)}
    for label, (lo, go, so) in (("shipped", shipped), ("library_gemms", bn_only)):
        loss_bound = max(4.0 * abs(l32 - l64), 2.0 ** -22 * abs(l64))
        if not abs(lo - l64) <= loss_bound:
            failures.append((label, "loss", abs(lo - l64), loss_bound))
        ratios = {}
        for k in g64:
            if NOISE.fullmatch(k):  # analytically zero: bounded by torch32's own rounding noise there
                ours_abs, t32_abs = float(go[k].abs().max()), float(g32[k].abs().max())
                ratios["zero:" + k] = ours_abs / max(t32_abs, 1e-300)
                if not ours_abs <= 4.0 * t32_abs:
                    failures.append((label, "zero-gradient " + k, ours_abs, 4.0 * t32_abs))
                continue
            e_o, e_t = _rel(go[k], g64[k]), _rel(g32[k], g64[k])
            ratios[k] = e_o / max(e_t, 1e-300)
            if not e_o <= max(4.0 * e_t, 2e-7):
                failures.append((label, "grad " + k, e_o, e_t))
        for k in s64:
            e_o, e_t = _rel(so[k], s64[k]), _rel(s32[k], s64[k])
            ratios["stat:" + k] = e_o / max(e_t, 1e-300)
            if not e_o <= max(4.0 * e_t, 2e-7):
                failures.append((label, "stat " + k, e_o, e_t))
        for kind, keys in (("grad", [k for k in ratios if ":" not in k]), ("zero_grad", [k for k in ratios if k.startswith("zero:")]),
                           ("stat", [k for k in ratios if k.startswith("stat:")])):
            vals = sorted((ratios[k], k) for k in keys)
            report["%s_%s_ratio_ours_over_torch32" % (label, kind)] = {
                "worst": [round(vals[-1][0], 3), vals[-1][1]], "median": round(vals[len(vals) // 2][0], 3)}
        report[label + "_loss_err"] = abs(lo - l64)
        errs = sorted(_rel(go[k], g64[k]) for k in g64 if not NOISE.fullmatch(k))
        report[label + "_grad_err_vs_float64"] = {"worst": errs[-1], "median": errs[len(errs) // 2]}
    errs = sorted(_rel(g32[k], g64[k]) for k in g64 if not NOISE.fullmatch(k))
    report["torch32_grad_err_vs_float64"] = {"worst": errs[-1], "median": errs[len(errs) // 2]}
    print("PARITY " + json.dumps(report))
    assert not failures, failures


# ------------------------------------------------------------------------------ 4. a recorded run that reaches the kernels
def test_train_nnet_at_batch_256_matches_reference_run_on_the_kernels(gemm_calls):
    """tests/golden/train_nnet_b256.npz: the reference's own train_nnet on ResnetModel(54, 6, 64, 64, 2, 1, True), 1024 examples
    in batches of 256, six iterations from iteration 2, lr 1e-3 with the default decay.  Same tolerances and exclusions as
    test_train_nnet_on_device_matches_reference_run — and every trunk Linear on dca_f16x3_gemm: 6 Linears x (forward + input
    gradient) less fc1's input gradient = 11 launches per step; fc_out (1 wide) is on the library."""
    from deepcubea_amd import _lib
    from deepcubea_amd.utils import nnet_utils
    from deepcubea_amd.utils.pytorch_models import ResnetModel
    _lib.require_gpu()
    g = np.load(os.path.join(ROOT, "tests", "golden", "train_nnet_b256.npz"))
    tag = "b256"
    net = ResnetModel(54, 6, 64, 64, 2, 1, True)
    net.load_state_dict({k.split(":", 2)[2]: torch.tensor(g[k]) for k in g.files if k.startswith(tag + ":init:")})
    net = net.cuda()
    bs, itrs, itr0, lr, lr_d = g[tag + ":args"]
    assert int(bs) == 256 and int(itrs) == 6
    np.random.seed(7)
    random.seed(7)
    x = torch.from_numpy(g[tag + ":x"]).cuda()
    y = torch.from_numpy(g[tag + ":y"].astype(np.float32)).cuda()
    last = nnet_utils.train_nnet(net, x, y, torch.device("cuda"), int(bs), int(itrs), int(itr0), float(lr), float(lr_d),
                                 display=False)
    assert len(gemm_calls) == 11 * 6
    assert sorted(set(gemm_calls)) == [(2, 256, 64), (2, 256, 384)]  # k = 64, and fc1's 324 padded to 384
    want_loss = float(g[tag + ":last_loss"])
    use = {"loss": abs(last - want_loss) / (1e-3 * max(1.0, abs(last))), "weights": 0.0}
    assert abs(last - want_loss) < 1e-3 * max(1.0, abs(last))
    bad = []
    for k, v in net.state_dict().items():
        if "num_batches_tracked" in k:
            assert int(v) == int(g["%s:final:%s" % (tag, k)])
            continue
        if re.fullmatch(r"(fc1|fc2|blocks\.\d\.[02])\.bias", k) or "running_mean" in k:
            continue  # noise by construction (see test_train_nnet_on_device_matches_reference_run)
        want = g["%s:final:%s" % (tag, k)]
        frac = float(np.max(np.abs(v.cpu().numpy() - want) / (2e-4 + 2e-3 * np.abs(want))))
        use["weights"] = max(use["weights"], frac)
        if not np.allclose(v.cpu().numpy(), want, rtol=2e-3, atol=2e-4):
            bad.append(k)
    print("PARITY " + json.dumps({"fixture": "train_nnet_b256", "last_loss": last, "fraction_of_tolerance_used": use}))
    assert not bad, bad
