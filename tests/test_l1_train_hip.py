"""GPU tests of the training step's layer 1 from the uint8 rows (`--l1_train embed`): the scatter kernel dca_l1_embed_wgrad
(csrc/dca_embed_train.hip) bit for bit against a host loop that follows the summation order include/dca.h states, against float64
with the bound of a sequential sum, its refusals; `_lib.l1_embed_train` (forward dca_l1_embed, backward the scatter); the model's
"embed" mode against float64 by the rule of test_train_step_hip.py (as close to float64 as torch's fp32 step is, factor 4; floors
2^-22 of the loss and 2e-7 of a tensor's largest element); and `train_nnet` in that mode.

Shapes are the smallest at which each mechanism can go wrong: both sides of the chunk (32 / 64 rows) and slice (S rows) boundaries,
one to three slices, whole and partial column tiles of every tile width (64, 32, 16)."""
import ctypes as C
import math
import random
import re

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu
GEOMETRIES = [(54, 6), (16, 16), (25, 25), (36, 36), (49, 49), (49, 6)]  # dca_l1_embed_supported(): cube3, puzzle15/24/35/48, lightsout7
NOISE = re.compile(r"(fc1|fc2|blocks\.\d\.[02])\.bias")  # a Linear bias in front of a BatchNorm: analytically zero gradient
U = 2.0 ** -24  # unit roundoff of fp32
SENTINEL = -777.25


def _p(t):
    return C.c_void_p(0 if t is None else t.data_ptr())


def _bits(t):
    return t.contiguous().view(torch.int32)


def _same(a, b):
    return torch.equal(_bits(a), _bits(b))


def _slice_rows(d, depth):
    from deepcubea_amd import _lib
    return _lib.l1_embed_wgrad_slice_rows(d, depth)


def _case(m, n, d, depth, seed, same_state=False):
    """uint8 states [m, d] (bytes < depth) and dy [m, n]: normal noise spread over 24 binades by a per-row power of two, so that
    the order of a sum shows in its bits."""
    rng = np.random.default_rng(seed)
    s = rng.integers(0, depth, size=(m, d), dtype=np.uint8)
    if same_state and m:
        s[:] = s[0]
    dy = (rng.standard_normal((m, n)) * 2.0 ** rng.integers(-12, 12, size=(m, 1))).astype(np.float32)
    return s, dy


def _host_model(s, dy, depth, S):
    """The contract's order on the host: per slice of S rows, `for r ascending: acc[cols(r)] += dy[r]` in fp32 from +0.0 (the
    columns of one row are distinct, so the vectorised add is exact), the slices then added in ascending order from +0.0."""
    m, d = s.shape
    n = dy.shape[1]
    S = S if S > 0 else max(m, 1)
    base = np.arange(d) * depth
    tot_w, tot_b = np.zeros((d * depth, n), np.float32), np.zeros(n, np.float32)
    for a in range(0, m, S):
        pw, pb = np.zeros((d * depth, n), np.float32), np.zeros(n, np.float32)
        for r in range(a, min(a + S, m)):
            pw[base + s[r]] += dy[r]
            pb += dy[r]
        tot_w += pw
        tot_b += pb
    return np.ascontiguousarray(tot_w.T), tot_b


def _launch(s, dy, depth, ld_dy=None, ldw=None, want_db=True, ws_bytes=None):
    """dca_l1_embed_wgrad through the raw C ABI on strided buffers filled with a sentinel -> (rc, dW buffer [n, ldw], db, dy buffer)."""
    from deepcubea_amd import _lib
    L = _lib.lib()
    m, d = s.shape
    n = dy.shape[1]
    K = d * depth
    ld_dy = n if ld_dy is None else ld_dy
    ldw = K if ldw is None else ldw
    s_dev = torch.zeros((max(m, 1), d), dtype=torch.uint8, device="cuda")  # (an empty tensor has no address)
    s_dev[:m] = torch.from_numpy(s).cuda()
    dy_buf = torch.full((max(m, 1), ld_dy), float("nan"), dtype=torch.float32, device="cuda")
    dy_buf[:m, :n] = torch.from_numpy(dy).cuda()
    dy_before = dy_buf.clone()
    dw_buf = torch.full((n, ldw), SENTINEL, dtype=torch.float32, device="cuda")
    db = torch.full((n,), SENTINEL, dtype=torch.float32, device="cuda") if want_db else None
    need = int(L.dca_l1_embed_wgrad_workspace_bytes(C.c_int64(m), d, depth, C.c_int64(n)))
    assert need >= 0
    ws_bytes = need if ws_bytes is None else ws_bytes
    ws = torch.empty(max(ws_bytes, 1), dtype=torch.uint8, device="cuda") if ws_bytes else None
    rc = L.dca_l1_embed_wgrad(_p(s_dev), C.c_int64(m), d, depth, _p(dy_buf), C.c_int64(ld_dy), C.c_int64(n), _p(dw_buf), C.c_int64(ldw),
                              _p(db), _p(ws), C.c_int64(ws_bytes), _lib.stream_ptr())
    torch.cuda.synchronize()
    assert _same(dy_buf, dy_before), "dy (slack included) is read-only"
    return rc, dw_buf, db


def _check_bits(s, dy, depth, strided=True):
    m, d = s.shape
    n, K = dy.shape[1], d * depth
    want_w, want_b = _host_model(s, dy, depth, _slice_rows(d, depth))
    rc, dw_buf, db = _launch(s, dy, depth, ld_dy=n + 4 if strided else None, ldw=K + 3 if strided else None)
    assert rc == 0
    assert _same(dw_buf[:, :K], torch.from_numpy(want_w).cuda()), (m, n, d, depth)
    assert _same(db, torch.from_numpy(want_b).cuda()), (m, n, d, depth)
    if strided:
        assert bool((dw_buf[:, K:] == SENTINEL).all()), "the slack of dW's rows keeps its sentinel"
    return dw_buf, db


# ------------------------------------------------------------------------------ 1. the kernel, bit for bit
@pytest.mark.parametrize("d,depth", GEOMETRIES)
def test_every_geometry_bit_for_bit_against_the_host_loop(d, depth):
    """m = 65, n = 68 (a partial last column tile at every tile width), strides ld_dy = n + 4 and ldw = K + 3."""
    s, dy = _case(65, 68, d, depth, seed=d * 100 + depth)
    _check_bits(s, dy, depth)


M_LABELS = ["1", "2", "63", "64", "65", "257", "S-1", "S", "S+1", "2*S+3"]


@pytest.mark.parametrize("m_label", M_LABELS)
@pytest.mark.parametrize("d,depth", [(16, 16), (49, 49)])
def test_row_and_column_grid_on_both_tile_widths(d, depth, m_label):
    """(16,16): 64-wide tiles; (49,49): 16-wide.  m on both sides of the chunk and slice boundaries, up to three slices; n in
    {4, 16, 60, 64, 68, 200}: 60, 68 and 200 leave a partial last tile.  The slice-relative sizes need S <= 2048 (the kernel's
    S is 1024 / 2048; a longer S would keep m <= 4100 instead)."""
    S = _slice_rows(d, depth)
    assert 0 < S <= 2048
    m = int(eval(m_label, {"S": S}))
    for n in (4, 16, 60, 64, 68, 200):
        s, dy = _case(m, n, d, depth, seed=m * 1000 + n)
        _check_bits(s, dy, depth)


def test_every_row_the_same_state_is_the_longest_chain_and_leaves_plus_zero():
    """All 300 rows select the same 16 columns: 300 dependent adds on one address; every other column is +0.0 by bit pattern."""
    d = depth = 16
    s, dy = _case(300, 64, d, depth, seed=5, same_state=True)
    dw_buf, _ = _check_bits(s, dy, depth)
    hit = np.zeros(d * depth, bool)
    hit[np.arange(d) * depth + s[0]] = True
    untouched = _bits(dw_buf[:, :d * depth])[:, torch.from_numpy(~hit).cuda()]
    assert untouched.numel() == 64 * (256 - 16) and bool((untouched == 0).all())


def test_two_launches_give_identical_bits_and_db_may_be_null():
    d = depth = 49
    S = _slice_rows(d, depth)
    s, dy = _case(S + 70, 40, d, depth, seed=9)
    rc1, w1, b1 = _launch(s, dy, depth)
    rc2, w2, b2 = _launch(s, dy, depth)
    rc3, w3, b3 = _launch(s, dy, depth, want_db=False)
    assert rc1 == 0 and rc2 == 0 and rc3 == 0 and b3 is None
    assert _same(w1, w2) and _same(b1, b2) and _same(w1, w3)


def test_state_matrix_off_the_16_byte_grid_and_zero_rows():
    """A row slice of a larger byte matrix starts at any address (the kernel then reads it byte by byte); m == 0 writes zeros."""
    from deepcubea_amd import _lib
    d = depth = 25
    s, dy = _case(200, 36, d, depth, seed=11)
    buf = torch.zeros(200 * d + 1, dtype=torch.uint8, device="cuda")
    buf[1:] = torch.from_numpy(s).cuda().flatten()
    s_dev = buf[1:].view(200, d)
    assert s_dev.data_ptr() % 2 == 1
    dw = torch.full((36, d * depth), SENTINEL, dtype=torch.float32, device="cuda")
    db = torch.full((36,), SENTINEL, dtype=torch.float32, device="cuda")
    dy_dev = torch.from_numpy(dy).cuda()
    rc = _lib.lib().dca_l1_embed_wgrad(_p(s_dev), C.c_int64(200), d, depth, _p(dy_dev), C.c_int64(36), C.c_int64(36), _p(dw),
                                       C.c_int64(d * depth), _p(db), _p(None), C.c_int64(0), _lib.stream_ptr())
    assert rc == 0
    want_w, want_b = _host_model(s, dy, depth, _slice_rows(d, depth))
    assert _same(dw, torch.from_numpy(want_w).cuda()) and _same(db, torch.from_numpy(want_b).cuda())
    rc, dw0, db0 = _launch(s[:0], dy[:0], depth, ldw=d * depth + 3)
    assert rc == 0 and bool((_bits(dw0[:, :d * depth]) == 0).all()) and bool((_bits(db0) == 0).all())
    assert bool((dw0[:, d * depth:] == SENTINEL).all())


# ------------------------------------------------------------------------------ 2. the kernel against float64
def _seq_sum_bound(count, slices, sum_abs):
    """|fl(sum) - sum| of a sequential fp32 sum of `count` addends in `slices` partial sums: (count + slices) roundings at most
    touch a term, each relative 2^-24 (Higham, Accuracy and Stability, eq. 4.4, first order; 1 % for the higher orders)."""
    return 1.01 * (count + slices) * U * sum_abs


def test_against_float64_within_the_bound_of_a_sequential_sum():
    d = depth = 49
    m, n = 257, 64
    s, dy = _case(m, n, d, depth, seed=21)
    rc, dw, db = _launch(s, dy, depth)
    assert rc == 0
    slices = math.ceil(m / _slice_rows(d, depth))
    onehot = np.zeros((m, d * depth), np.float64)
    onehot[np.arange(m)[:, None], np.arange(d) * depth + s] = 1.0
    dy64 = dy.astype(np.float64)
    want, sum_abs, count = dy64.T @ onehot, np.abs(dy64).T @ onehot, onehot.sum(0)[None, :]
    err = np.abs(dw.cpu().numpy().astype(np.float64) - want)
    assert np.all(err <= _seq_sum_bound(count, slices, sum_abs)), float(np.max(err / np.maximum(_seq_sum_bound(count, slices, sum_abs), 1e-300)))
    err_b = np.abs(db.cpu().numpy().astype(np.float64) - dy64.sum(0))
    assert np.all(err_b <= _seq_sum_bound(m, slices, np.abs(dy64).sum(0)))


# ------------------------------------------------------------------------------ 3. refusals
def test_every_refusal_returns_badarg_with_a_message_and_launches_nothing():
    from deepcubea_amd import _lib
    L = _lib.lib()
    d = depth = 16
    K = d * depth
    S = _slice_rows(d, depth)
    m, n = S + 1, 8
    s = torch.zeros((m, d), dtype=torch.uint8, device="cuda")
    dy = torch.ones((m, n + 8), dtype=torch.float32, device="cuda")
    dw = torch.full((n, K + 4), SENTINEL, dtype=torch.float32, device="cuda")
    db = torch.full((n,), SENTINEL, dtype=torch.float32, device="cuda")
    need = int(L.dca_l1_embed_wgrad_workspace_bytes(C.c_int64(m), d, depth, C.c_int64(n)))
    assert need == 2 * (n * K + n) * 4
    ws = torch.empty(need, dtype=torch.uint8, device="cuda")
    good = dict(s=_p(s), m=m, d=d, depth=depth, dy=_p(dy), ld_dy=n + 8, n=n, dw=_p(dw), ldw=K + 4, db=_p(db), ws=_p(ws), wsb=need)

    def call(**kw):
        a = dict(good, **kw)
        return L.dca_l1_embed_wgrad(a["s"], C.c_int64(a["m"]), a["d"], a["depth"], a["dy"], C.c_int64(a["ld_dy"]), C.c_int64(a["n"]),
                                    a["dw"], C.c_int64(a["ldw"]), a["db"], a["ws"], C.c_int64(a["wsb"]), _lib.stream_ptr())

    bad = {
        "unsupported geometry": dict(d=5, depth=5),
        "n % 4 != 0": dict(n=6),
        "m < 0": dict(m=-1),
        "null states": dict(s=_p(None)),
        "null dy": dict(dy=_p(None)),
        "null dW": dict(dw=_p(None)),
        "misaligned dy": dict(dy=C.c_void_p(dy.data_ptr() + 4)),
        "ld_dy % 4 != 0": dict(ld_dy=n + 2),
        "ldw < K": dict(ldw=K - 1),
        "ld_dy < n": dict(ld_dy=n - 4),
        "workspace too small": dict(wsb=need - 1),
        "workspace missing": dict(ws=_p(None)),
    }
    for what, kw in bad.items():
        assert call(**kw) == -1, what
        assert len(L.dca_last_error()) > 0, what
    torch.cuda.synchronize()
    assert bool((dw == SENTINEL).all()) and bool((db == SENTINEL).all()), "a refused call launches nothing"
    assert int(L.dca_l1_embed_wgrad_slice_rows(5, 5)) == -1 and len(L.dca_last_error()) > 0
    assert int(L.dca_l1_embed_wgrad_workspace_bytes(C.c_int64(-1), d, depth, C.c_int64(n))) == -1
    assert call() == 0  # and the same arguments, all good, run
    torch.cuda.synchronize()
    assert bool((dw[:, :K] != SENTINEL).all()) and bool((dw[:, K:] == SENTINEL).all())


# ------------------------------------------------------------------------------ 4. the autograd function
def _lin(k, n, seed, bias=True):
    g = torch.Generator().manual_seed(seed)
    lin = torch.nn.Linear(k, n, bias=bias)
    with torch.no_grad():
        lin.weight.copy_(torch.randn(n, k, generator=g) / 4.0)
        if bias:
            lin.bias.copy_(torch.randn(n, generator=g))
    return lin


@pytest.fixture
def wgrad_calls(monkeypatch):
    """Counts the calls of _lib.l1_embed_wgrad."""
    from deepcubea_amd import _lib
    calls = []
    real = _lib.l1_embed_wgrad

    def counting(*a, **kw):
        calls.append(kw.get("want_bias", True))
        return real(*a, **kw)

    monkeypatch.setattr(_lib, "l1_embed_wgrad", counting)
    return calls


def test_autograd_function_forward_backward_bits_float64_and_skipped_work(wgrad_calls):
    from deepcubea_amd import _lib
    _lib.require_gpu()
    d = depth = 16
    m, n, K = 300, 128, 256
    s_np, dy_np = _case(m, n, d, depth, seed=31)
    s, dy = torch.from_numpy(s_np).cuda(), torch.from_numpy(dy_np).cuda()
    lin = _lin(K, n, 41).cuda()
    y = _lib.l1_embed_train(s, lin, depth)
    assert y.is_contiguous() and tuple(y.shape) == (m, n)
    y.backward(dy)
    assert wgrad_calls == [True]
    assert s.grad is None and not s.requires_grad  # the states get no gradient
    # bits: forward = the inference kernel on W^T, backward = the scatter kernel
    assert _same(y.detach(), _lib.l1_embed(s, depth, lin.weight.detach().t().contiguous(), lin.bias.detach(), relu=False))
    dw, db = _lib.l1_embed_wgrad(s, dy, depth)
    assert _same(lin.weight.grad, dw) and _same(lin.bias.grad, db)
    # float64 autograd of F.linear(one_hot): y is a sequential sum of bias + 16 weights, the gradients sums over the rows
    ref = torch.nn.Linear(K, n).double().cuda()
    ref.load_state_dict({k: v.double() for k, v in lin.state_dict().items()})
    onehot = torch.nn.functional.one_hot(s.long(), depth).view(m, K).double()
    y64 = ref(onehot)
    y64.backward(dy.double())
    abs_terms = onehot @ ref.weight.detach().abs().t() + ref.bias.detach().abs()
    assert bool(((y.detach().double() - y64.detach()).abs() <= _seq_sum_bound(d + 1, 1, abs_terms)).all())
    count, sum_abs = onehot.sum(0)[None, :], dy.double().abs().t() @ onehot
    assert bool(((lin.weight.grad.double() - ref.weight.grad).abs() <= _seq_sum_bound(count, 1, sum_abs)).all())
    assert bool(((lin.bias.grad.double() - ref.bias.grad).abs() <= _seq_sum_bound(m, 1, dy.double().abs().sum(0))).all())

    # a frozen weight: no scatter at all (the bias gradient alone is a column sum)
    del wgrad_calls[:]
    frozen = _lin(K, n, 41).cuda()
    frozen.weight.requires_grad_(False)
    _lib.l1_embed_train(s, frozen, depth).backward(dy)
    assert wgrad_calls == [] and frozen.weight.grad is None
    assert bool(((frozen.bias.grad.double() - ref.bias.grad).abs() <= _seq_sum_bound(m, 1, dy.double().abs().sum(0))).all())
    # no bias: the scatter skips db; no bias and a frozen weight: nothing to differentiate, no call
    nobias = _lin(K, n, 41, bias=False).cuda()
    y2 = _lib.l1_embed_train(s, nobias, depth)
    y2.backward(dy)
    assert wgrad_calls == [False] and _same(nobias.weight.grad, dw)
    del wgrad_calls[:]
    nobias.weight.requires_grad_(False)
    assert not _lib.l1_embed_train(s, nobias, depth).requires_grad and wgrad_calls == []


# ------------------------------------------------------------------------------ 5. the model
@pytest.fixture
def counters(monkeypatch, wgrad_calls):
    from deepcubea_amd import _lib
    from deepcubea_amd.utils.pytorch_models import ResnetModel
    counts = {"linear_f16x3": 0, "onehot": 0, "encode": 0, "wgrad": wgrad_calls}
    real_lin, real_onehot, real_encode = _lib._train_gemm, _lib.onehot, ResnetModel.encode

    def lin(*a, **kw):
        counts["linear_f16x3"] += 1
        return real_lin(*a, **kw)

    def onehot(*a, **kw):
        counts["onehot"] += 1
        return real_onehot(*a, **kw)

    def encode(self, x):
        counts["encode"] += 1
        return real_encode(self, x)

    monkeypatch.setattr(_lib, "_train_gemm", lin)  # (every forward and input-gradient GEMM of linear_train; the key keeps its name)
    monkeypatch.setattr(_lib, "onehot", onehot)
    monkeypatch.setattr(ResnetModel, "encode", encode)
    return counts


def _plain_trunk(net, x):
    """The network's forward in training mode on its own nn.Linear / nn.BatchNorm1d modules: torch's kernels only (the yardstick)."""
    relu = torch.relu
    x = relu(net.bn1(net.fc1(x)))
    x = relu(net.bn2(net.fc2(x)))
    for blk in net.blocks:
        h = relu(blk[1](blk[0](x)))
        x = relu(blk[3](blk[2](h)) + x)
    return net.fc_out(x)


def _fresh_net(env_name):
    from deepcubea_amd.utils import env_utils
    from deepcubea_amd.utils.synthetic_weights import load_synthetic_weights
    net = env_utils.get_environment(env_name).get_nnet_model()
    load_synthetic_weights(net, 2024)
    return net.cuda().train()


def _one_step(env_name, mode, states, y):
    """One forward + backward from the synthetic weights of seed 2024 -> (loss, {param: grad}, {running stat: value}, net)."""
    net = _fresh_net(env_name)
    onehot = torch.nn.functional.one_hot(states.long(), net.one_hot_depth).view(states.shape[0], -1)
    if mode == "float64":
        net = net.double()
        out = net.trunk(onehot.double())[:, 0]
        loss = torch.nn.functional.mse_loss(out, y.double())
    elif mode == "torch32":
        out = _plain_trunk(net, onehot.float())[:, 0]
        loss = torch.nn.functional.mse_loss(out, y)
    else:
        net.set_l1_train(mode)
        out = net(states)[:, 0]
        loss = torch.nn.functional.mse_loss(out, y)
    loss.backward()
    grads = {k: p.grad.double().cpu() for k, p in net.named_parameters()}
    stats = {k: v.double().cpu() for k, v in net.state_dict().items() if "running_" in k}
    return float(loss.detach().double()), grads, stats, net


def _rel(a, ref):
    return float((a - ref).abs().max()) / max(float(ref.abs().max()), 1e-300)


@pytest.mark.parametrize("env_name,batch,gemm_mode_launches", [("puzzle15", 1003, 19), ("puzzle24", 300, 18)])
def test_model_embed_mode_whole_step_against_float64_and_call_counts(env_name, batch, gemm_mode_launches, counters):
    """env.get_nnet_model() (5000 / 1000 / 4 blocks), one forward + backward in "embed" mode: loss, every gradient and every running
    statistic as close to float64 as plain torch fp32 is (factor 4; floors 2^-22 of the loss, 2e-7 of a tensor's largest element;
    analytically-zero gradients within 4x torch32's noise) — the rule of test_whole_step_at_the_production_geometry_against_float64.
    No one-hot matrix on the way (no encode / _lib.onehot call), 18 f16x3 Linears (19 less fc1's forward) and one scatter; "gemm"
    mode on the same object: 19 for puzzle15 (18 for puzzle24, whose 625 columns keep fc1 off the f16x3 kernel) and no scatter.
    Eval-mode output is bit-identical in both modes."""
    from deepcubea_amd import _lib
    _lib.require_gpu()
    env_id, dim = _lib.env_ids(env_name)[:2]
    states, nb, _ = _lib.generate_states(env_id, dim, batch, 0, 30, 5, 0)
    x = _lib.nnet_input(env_id, dim, states)
    y = nb.float().contiguous()
    l64, g64, s64, _ = _one_step(env_name, "float64", x, y)
    l32, g32, s32, _ = _one_step(env_name, "torch32", x, y)
    assert counters["linear_f16x3"] == 0 and counters["wgrad"] == []
    for k in ("onehot", "encode"):
        counters[k] = 0
    lo, go, so, net = _one_step(env_name, "embed", x, y)
    assert counters["onehot"] == 0 and counters["encode"] == 0, "no one-hot matrix in embed mode"
    assert counters["linear_f16x3"] == 18 and len(counters["wgrad"]) == 1
    assert int(net.bn1.num_batches_tracked) == int(_fresh_net(env_name).bn1.num_batches_tracked) + 1

    failures, figures = [], {}
    loss_bound = max(4.0 * abs(l32 - l64), 2.0 ** -22 * abs(l64))
    figures["loss"] = (abs(lo - l64), loss_bound)
    if not abs(lo - l64) <= loss_bound:
        failures.append(("loss", abs(lo - l64), loss_bound))
    for k in g64:
        if NOISE.fullmatch(k):
            ours_abs, t32_abs = float(go[k].abs().max()), float(g32[k].abs().max())
            figures["zero:" + k] = (ours_abs, t32_abs)
            if not ours_abs <= 4.0 * t32_abs:
                failures.append(("zero-gradient " + k, ours_abs, 4.0 * t32_abs))
            continue
        e_o, e_t = _rel(go[k], g64[k]), _rel(g32[k], g64[k])
        figures[k] = (e_o, e_t)
        if not e_o <= max(4.0 * e_t, 2e-7):
            failures.append(("grad " + k, e_o, e_t))
    for k in s64:
        e_o, e_t = _rel(so[k], s64[k]), _rel(s32[k], s64[k])
        figures["stat:" + k] = (e_o, e_t)
        if not e_o <= max(4.0 * e_t, 2e-7):
            failures.append(("stat " + k, e_o, e_t))
    print("L1TRAIN PARITY %s (ours, torch32 / bound) %s" % (env_name, {k: ("%.3g" % a, "%.3g" % b) for k, (a, b) in figures.items()
                                                                     if k in ("loss", "fc1.weight", "zero:fc1.bias", "bn1.weight", "bn1.bias")}))
    assert not failures, failures

    # the same object back in "gemm" mode: today's path, launch for launch
    counters["linear_f16x3"] = 0
    del counters["wgrad"][:]
    net.set_l1_train("gemm")
    net.zero_grad()
    torch.nn.functional.mse_loss(net(x)[:, 0], y).backward()
    assert counters["linear_f16x3"] == gemm_mode_launches and counters["wgrad"] == [] and counters["encode"] == 1
    # eval mode does not look at the switch
    net.eval()
    with torch.no_grad():
        out_gemm = net(x[:64])
        net.set_l1_train("embed")
        out_embed = net(x[:64])
    assert _same(out_gemm, out_embed)


# ------------------------------------------------------------------------------ 6. the driver's training loop
def test_train_nnet_three_iterations_in_embed_mode_twice_the_same_bits():
    from deepcubea_amd import _lib
    from deepcubea_amd.utils import env_utils, nnet_utils
    _lib.require_gpu()
    env_id, dim = _lib.env_ids("puzzle15")[:2]
    states, nb, _ = _lib.generate_states(env_id, dim, 768, 0, 30, 7, 0)
    x = _lib.nnet_input(env_id, dim, states)
    y = nb.float().view(-1, 1).contiguous()

    def run():
        torch.manual_seed(3)
        np.random.seed(3)
        random.seed(3)
        net = env_utils.get_environment("puzzle15").get_nnet_model().cuda()
        net.set_l1_train("embed")
        last = nnet_utils.train_nnet(net, x, y, torch.device("cuda"), 256, 3, 0, 1e-3, 0.9999993, display=False)
        return last, net

    last1, net1 = run()
    last2, net2 = run()
    assert math.isfinite(last1) and last1 == last2
    assert int(net1.bn1.num_batches_tracked) == 3
    for (k, a), (_, b) in zip(net1.state_dict().items(), net2.state_dict().items()):
        assert torch.equal(a, b), k
