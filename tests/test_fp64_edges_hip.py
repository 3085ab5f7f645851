"""The float64 mode's kernels (csrc/dca_gemm64.hip: dca_gemm64, dca_l1_embed64; csrc/dca_mlp.hip: dca_head_gemv on DCA_DT_F64
rows, dca_head_gemv64) away from the round shapes of the 5000/1000 network: ragged m / n / k, one to four K-tiles, row strides
larger than the width, every column tile of the embedding kernel, its one-state and odd last blocks, the wrap of a workgroup
onto a second row block, the output layer's grid-stride second trip, every DCA_ARG refusal, and a narrow network checked by
value against the module in float64 on the host.

Every output buffer is filled with NaN before the launch (views with padding included): after it no in-range element is NaN
and every padding element still holds the fill's bits.

The random-data bounds are derived, not measured.  A float64 sum of t terms, in any order, fused or not, is within
gamma_t = t u / (1 - t u) of the exact sum times the sum of the terms' magnitudes (u = 2^-53).  A dense layer's element is a
sum of k products, the bias and the skip (k + 2 terms), the output layer's a sum of k products, 6 butterfly levels and the
bias (<= k + 8 roundings); device and host are each within that of the exact value, so they are within twice that of each
other: 2 (k + 2) u (sum |a||w| + |bias| + |skip|), and 2 (k + 8) u (sum |x||w| + |b|)."""
import copy
import ctypes as C

import pytest
import torch

pytestmark = pytest.mark.gpu

U = 2.0 ** -53
NAN_BITS = 0x7FF8000000000000  # the quiet NaN torch.full(..., nan) writes
GEOMETRIES = [(54, 6), (16, 16), (25, 25), (36, 36), (49, 49), (49, 6)]  # cube3, puzzle15/24/35/48, lightsout7 (state_dim, depth)


def _L():
    from deepcubea_amd import _lib
    _lib.require_gpu()
    return _lib


def _nan(rows, cols, dtype=torch.float64):
    return torch.full((rows, cols), float("nan"), dtype=dtype, device="cuda")


def _padded(t: torch.Tensor, ld: int, col0: int = 0):
    """t [m, w] (cpu) -> (buffer [m, ld] on the device, NaN outside the window; its view [:, col0:col0 + w] holding t)."""
    buf = _nan(t.shape[0], ld, t.dtype)
    view = buf[:, col0:col0 + t.shape[1]]
    view.copy_(t)
    return buf, view


def _assert_written(buf: torch.Tensor, n: int, what):
    """buf [m, ld], the launch's output in columns [0, n): no NaN left there, the fill's bits untouched behind."""
    assert not bool(torch.isnan(buf[:, :n]).any()), ("an in-range element was not written", what)
    if buf.shape[1] > n:
        pad = buf[:, n:].contiguous()
        bits = pad.view(torch.int64) if pad.dtype == torch.float64 else pad.view(torch.int32)
        fill = NAN_BITS if pad.dtype == torch.float64 else 0x7FC00000
        assert bool((bits == fill).all()), ("a padding element was written", what)


# ------------------------------------------------------------------------------------------------------------- dca_gemm64
# every m, n and k of the lists at least once; K-tiles 1 (k <= 16), 2 (18..32), 3 (34) and 4 (62); m, n and k ragged together
GEMM_SHAPES = [(1, 1, 2), (3, 15, 4), (63, 16, 14), (64, 17, 16), (65, 63, 18), (127, 64, 30), (128, 65, 32), (129, 127, 34),
               (257, 128, 62), (3, 129, 2), (65, 192, 18), (129, 200, 34), (257, 200, 62)]


def _int_problem(m, n, k, seed):
    """Small integers as in test_gemm64_exact_on_integer_data: asymmetric w, distinct rows, every sum exact in float64."""
    g = torch.Generator().manual_seed(seed)
    a = torch.randint(-4, 5, (m, k), generator=g).double()
    a[:, 0] += torch.arange(m, dtype=torch.float64) % 7
    w = torch.randint(-4, 5, (n, k), generator=g).double()
    w[:, 0] += torch.arange(n, dtype=torch.float64)
    bias = torch.randint(-50, 51, (n,), generator=g).double()
    skip = torch.randint(-1000, 1001, (m, n), generator=g).double()
    return a, w, bias, skip


def _host_gemm(a, w):
    return torch.from_numpy(a.numpy() @ w.numpy().T)


# (name, bias, skip, relu, skip aliases out)
GEMM_FORMS = [("plain", False, False, False, False), ("bias_relu", True, False, True, False), ("bias_skip", True, True, False, False),
              ("inplace_skip_relu", False, True, True, True), ("skip_no_bias", False, True, False, False)]


def _gemm_forms(L, ad, wd, bias, skip, n, ldo, check, what):
    """The five forms of the layer on device operands (views or not), each into a NaN-filled buffer of row stride ldo (the
    skip in another buffer of that stride, or in the output's own); check(name, bias + skip, |bias| + |skip|, relu, got [m, n]
    on the host) judges each: the caller holds a . w^T."""
    m = ad.shape[0]
    bd = bias.cuda()
    for name, use_b, use_s, relu, inplace in GEMM_FORMS:
        buf = _nan(m, ldo)
        out = buf[:, :n]
        sk = None
        if use_s and inplace:
            out.copy_(skip)
            sk = out
        elif use_s:
            sk = _padded(skip, ldo)[1]
        got = L.gemm64(ad, wd, bd if use_b else None, sk, relu, out=out)
        assert got.data_ptr() == buf.data_ptr()
        _assert_written(buf, n, (what, name))
        extra = (bias if use_b else 0.0) + (skip if use_s else 0.0)
        mag = (bias.abs() if use_b else 0.0) + (skip.abs() if use_s else 0.0)
        check(name, extra, mag, relu, buf[:, :n].cpu())


@pytest.mark.parametrize("m,n,k", GEMM_SHAPES)
@torch.no_grad()
def test_gemm64_exact_at_ragged_shapes_and_strides(m, n, k):
    """Bit for bit against host float64 on integer data, every form of the layer: contiguous, then lda = k + 2 / ldw = k + 4 /
    ldo = n + 3, then `a` as a column window (lda = k + 6) that starts at column 2 of a wider matrix.  The operands' padding
    holds NaN: one padding element read into a sum poisons it."""
    L = _L()
    a, w, bias, skip = _int_problem(m, n, k, 1000 * m + 10 * n + k)
    prod = _host_gemm(a, w)

    def check(tag):
        def f(name, extra, mag, relu, got):
            want = prod + extra
            assert torch.equal(got, want.relu() if relu else want), (m, n, k, tag, name)
        return f

    _gemm_forms(L, a.cuda(), w.cuda(), bias, skip, n, n, check("contiguous"), "contiguous")
    wv = _padded(w, k + 4)[1]
    assert wv.stride(0) == k + 4
    av = _padded(a, k + 2)[1]
    _gemm_forms(L, av, wv, bias, skip, n, n + 3, check("lda k+2"), "lda k+2")
    av = _padded(a, k + 6, 2)[1]
    assert av.stride(0) == k + 6 and av.data_ptr() % 16 == 0 and av.data_ptr() != av.untyped_storage().data_ptr()
    _gemm_forms(L, av, wv, bias, skip, n, n + 3, check("window"), "window")


@torch.no_grad()
def test_gemm64_bits_do_not_depend_on_batch_stride_or_padding():
    """Random float64 data, bit for bit between launches: a row alone / inside a 257-row batch / under another lda; k = 18
    against the same data zero-padded to k = 32; n = 65 against the first 65 units of a 192-unit layer that extends it."""
    L = _L()
    g = torch.Generator().manual_seed(64)
    m, n, k = 257, 129, 62
    a = torch.randn((m, k), generator=g, dtype=torch.float64)
    w = torch.randn((n, k), generator=g, dtype=torch.float64).cuda()
    b = torch.randn((n,), generator=g, dtype=torch.float64).cuda()
    ad = a.cuda()
    full = L.gemm64(ad, w, b, None, False)
    assert torch.equal(L.gemm64(_padded(a, k + 6, 2)[1], w, b, None, False), full)
    for r in (0, 63, 64, 127, 128, 200):
        assert torch.equal(L.gemm64(ad[r:r + 1].contiguous(), w, b, None, False)[0], full[r]), r
        assert torch.equal(L.gemm64(_padded(a[r:r + 1], k + 2)[1], w, b, None, False)[0], full[r]), r
    # K tail: the kernel's zero fill against zeros that are really there
    m, n = 65, 63
    a18 = torch.randn((m, 18), generator=g, dtype=torch.float64)
    w18 = torch.randn((n, 18), generator=g, dtype=torch.float64)
    a32, w32 = torch.zeros((m, 32), dtype=torch.float64), torch.zeros((n, 32), dtype=torch.float64)
    a32[:, :18], w32[:, :18] = a18, w18
    assert torch.equal(L.gemm64(a18.cuda(), w18.cuda(), None, None, False), L.gemm64(a32.cuda(), w32.cuda(), None, None, False))
    # column tail: units 0..64 of a two-tile layer against the layer that ends there
    m, k = 129, 34
    a = torch.randn((m, k), generator=g, dtype=torch.float64).cuda()
    w192 = torch.randn((192, k), generator=g, dtype=torch.float64).cuda()
    b192 = torch.randn((192,), generator=g, dtype=torch.float64).cuda()
    wide = L.gemm64(a, w192, b192, None, True)
    assert torch.equal(L.gemm64(a, w192[:65].contiguous(), b192[:65].contiguous(), None, True), wide[:, :65])


@torch.no_grad()
def test_gemm64_random_data_within_the_derived_bound():
    """|got - want| <= 2 (k + 2) 2^-53 (sum |a||w| + |bias| + |skip|) per element against host float64 (module docstring);
    ReLU is 1-Lipschitz, so the bound holds behind it."""
    L = _L()
    worst = 0.0
    for m, n, k in [(3, 15, 4), (65, 63, 18), (128, 65, 32), (129, 127, 34), (257, 128, 62), (257, 200, 62)]:
        g = torch.Generator().manual_seed(7 * m + n + k)
        a = torch.randn((m, k), generator=g, dtype=torch.float64)
        w = torch.randn((n, k), generator=g, dtype=torch.float64)
        bias = torch.randn((n,), generator=g, dtype=torch.float64)
        skip = torch.randn((m, n), generator=g, dtype=torch.float64)
        prod, mag = _host_gemm(a, w), _host_gemm(a.abs(), w.abs())

        def check(name, extra, extra_mag, relu, got):
            nonlocal worst
            want = prod + extra
            want = want.relu() if relu else want
            bound = 2 * (k + 2) * U * (mag + extra_mag)
            err = (got - want).abs()
            worst = max(worst, float((err / bound).max()))
            assert bool((err <= bound).all()), (m, n, k, name, float((err / bound).max()))

        _gemm_forms(L, _padded(a, k + 2)[1], _padded(w, k + 4)[1], bias, skip, n, n + 3, check, (m, n, k))
    print("RATIO gemm64 random data: worst error / bound = %.4f" % worst)


# --------------------------------------------------------------------------------------------------------- dca_l1_embed64
E64_LDS_MAX = 160 * 1024


def _embed_tile(d, depth, n_pad):
    """(NT, rows staged per step) as dca_l1_embed64 chooses them: the widest of 64 / 32 / 16 that divides n_pad and leaves
    room for >= 256 staged rows next to the table slice, else 8; at most 1024 rows."""
    dp = (d + 7) & ~7

    def rows(nt, least):
        r = (E64_LDS_MAX - (d * depth * nt * 8 + nt * 8)) // dp
        return min(r, 1024) if r >= least else 0

    for nt in (64, 32, 16):
        if n_pad % nt == 0 and rows(nt, 256) > 0:
            return nt, rows(nt, 256)
    return 8, rows(8, 1)


# (state_dim, depth, n_pad, NT, rows)
EMBED_CASES = [(54, 6, 32, 32, 1024), (54, 6, 48, 16, 1024), (54, 6, 40, 8, 1024),
               (16, 16, 64, 64, 1024), (16, 16, 32, 32, 1024), (16, 16, 16, 16, 1024), (16, 16, 8, 8, 1024),
               (25, 25, 64, 16, 1024), (25, 25, 24, 8, 1024),
               (36, 36, 64, 8, 1024),
               (49, 49, 64, 8, 180),
               (49, 6, 64, 32, 1024), (49, 6, 48, 16, 1024), (49, 6, 8, 8, 1024)]


def _host_embed(x, depth, wt, b, relu):
    want = b.expand(x.shape[0], -1).clone()
    for p in range(x.shape[1]):
        want += wt[p * depth + x[:, p].long()]
    return want.relu() if relu else want


@pytest.mark.parametrize("d,depth,n_pad,nt,rows", EMBED_CASES)
@torch.no_grad()
def test_l1_embed64_every_tile_and_block_tail(d, depth, n_pad, nt, rows):
    """Bit for bit against the host sum (bias first, positions ascending) at every column tile the dispatch can choose:

        geometry   n_pad             tile NT
        (54, 6)    32 / 48 / 40      32 / 16 / 8
        (16, 16)   64 / 32 / 16 / 8  64 / 32 / 16 / 8
        (25, 25)   64 / 24           16 / 8        (NT 64 and 32 do not leave 256 rows)
        (36, 36)   64                8
        (49, 49)   64                8, staging 180 rows
        (49, 6)    64 / 48 / 8       32 / 16 / 8

    (the tile computed from the 160 KB of LDS as the dispatch computes it), with one state (half = 1, no second state), two,
    an odd block, a full block +- 1 and two blocks + 1."""
    L = _L()
    assert _embed_tile(d, depth, n_pad) == (nt, rows)
    g = torch.Generator().manual_seed(d * 1000 + depth * 10 + n_pad)
    ms = (1, 2, 3, 1023, 1024, 1025, 2049) if rows == 1024 else (179, 180, 181, 361)
    assert ms[-1] == 2 * rows + 1 and ms[-3] == rows
    wt = torch.randn((d * depth, n_pad), generator=g, dtype=torch.float64)
    b = torch.randn((n_pad,), generator=g, dtype=torch.float64)
    x = torch.randint(0, depth, (ms[-1], d), generator=g, dtype=torch.uint8)
    xd, wd, bd = x.cuda(), wt.cuda(), b.cuda()
    for relu in (False, True):
        want = _host_embed(x, depth, wt, b, relu)  # a row's sum does not depend on the rows around it: one reference
        for m in ms:
            out = _nan(m + 1, n_pad)  # one row behind the last stays NaN
            got = L.l1_embed64(xd[:m], depth, wd, bd, relu, out=out[:m])
            assert got.data_ptr() == out.data_ptr()
            assert bool(torch.isnan(out[m]).all()), (m, relu)
            assert not bool(torch.isnan(out[:m]).any()), (m, relu)
            assert torch.equal(out[:m].cpu(), want[:m]), (d, depth, n_pad, m, relu)


@torch.no_grad()
def test_l1_embed64_workgroup_wraps_onto_a_second_row_block():
    """(36, 36) at n_pad = 5120: 640 column tiles of 8, so gridDim.y = min(ceil(2048 / 640), steps) = 4 and m = 4 * 1024 + 1025
    has six row blocks — workgroups y = 0 and y = 1 go round again (r0 += gridDim.y * rows), re-staging state bytes over the
    ones just consumed; the last block is one state.  Bit equal to separate launches over the first, a middle and the
    wrapped slices, and 64 sampled columns against the host sum."""
    L = _L()
    d = depth = 36
    n_pad, m = 5120, 4 * 1024 + 1025
    assert _embed_tile(d, depth, n_pad) == (8, 1024)
    g = torch.Generator().manual_seed(36)
    wt = torch.randn((d * depth, n_pad), generator=g, dtype=torch.float64)
    b = torch.randn((n_pad,), generator=g, dtype=torch.float64)
    x = torch.randint(0, depth, (m, d), generator=g, dtype=torch.uint8)
    xd, wd, bd = x.cuda(), wt.cuda(), b.cuda()
    out = _nan(m, n_pad)
    L.l1_embed64(xd, depth, wd, bd, False, out=out)
    assert not bool(torch.isnan(out).any())
    for lo, hi in ((0, 1024), (2048, 3072), (4096, m)):
        assert torch.equal(L.l1_embed64(xd[lo:hi], depth, wd, bd, False), out[lo:hi]), (lo, hi)
    cols = torch.randperm(n_pad, generator=g)[:64].sort().values
    want = _host_embed(x, depth, wt[:, cols].contiguous(), b[cols], False)
    assert torch.equal(out[:, cols.cuda()].cpu(), want)


@torch.no_grad()
def test_l1_embed64_no_rows():
    L = _L()
    out = L.l1_embed64(torch.zeros((0, 16), dtype=torch.uint8, device="cuda"), 16, torch.zeros((256, 64), dtype=torch.float64, device="cuda"),
                       torch.zeros((64,), dtype=torch.float64, device="cuda"), True)
    assert tuple(out.shape) == (0, 64) and out.dtype == torch.float64


# ------------------------------------------------------------------------------- dca_head_gemv (F64 rows), dca_head_gemv64
HEAD_SHAPES = [(k, n_out) for k in (4, 8, 252, 256, 260, 1024) for n_out in (1, 2, 3, 8)] + [(2048, 8)]  # the last: 64 KB of LDS
HEAD_MS = (1, 3, 4, 5, 257)


def _head_both(L, x, w, b, what):
    """(dca_head_gemv64, dca_head_gemv on the same float64 rows), each into a NaN-filled buffer with one row to spare."""
    m, n_out = x.shape[0], w.shape[0]
    o64, o32 = _nan(m + 1, n_out), _nan(m + 1, n_out, torch.float32)
    L.head_gemv(x, w, b, out_dtype=torch.float64, out=o64[:m])
    L.head_gemv(x, w, b, out=o32[:m])
    for o in (o64, o32):
        assert bool(torch.isnan(o[m]).all()) and not bool(torch.isnan(o[:m]).any()), what
    # one rounding of the same sum
    assert torch.equal(o32[:m], o64[:m].float()), what
    return o64[:m], o32[:m]


@torch.no_grad()
def test_head_gemv_float64_rows_exact_bounded_and_position_independent():
    L = _L()
    worst = 0.0
    for k, n_out in HEAD_SHAPES:
        g = torch.Generator().manual_seed(100 * k + n_out)
        mm = HEAD_MS[-1]
        # integers: every product and partial sum exact, whatever the order
        xi = torch.randint(-4, 5, (mm, k), generator=g).double()
        xi[:, 0] += torch.arange(mm, dtype=torch.float64) % 7
        wi = torch.randint(-4, 5, (n_out, k), generator=g).float()
        wi[:, 0] += torch.arange(n_out, dtype=torch.float32)
        bi = torch.randint(-50, 51, (n_out,), generator=g).float()
        want_i = xi @ wi.double().t() + bi.double()
        # random
        x = torch.randn((mm, k), generator=g, dtype=torch.float64)
        w = torch.randn((n_out, k), generator=g)
        b = torch.randn((n_out,), generator=g)
        want = x @ w.double().t() + b.double()
        want_nb = x @ w.double().t()
        mag = x.abs() @ w.double().abs().t()
        xd, wd, bd = x.cuda(), w.cuda(), b.cuda()
        wide = _nan(mm, k + 8)
        wide[:, 4:4 + k] = xd
        full = None
        for m in reversed(HEAD_MS):
            what = (k, n_out, m)
            y64, _ = _head_both(L, xi[:m].cuda(), wi.cuda(), bi.cuda(), what)
            assert torch.equal(y64.cpu(), want_i[:m]), what
            y64, y32 = _head_both(L, xd[:m], wd, bd, what)
            bound = 2 * (k + 8) * U * (mag[:m] + b.double().abs())
            err = (y64.cpu() - want[:m]).abs()
            worst = max(worst, float((err / bound).max()))
            assert bool((err <= bound).all()), (what, float((err / bound).max()))
            n64, _ = _head_both(L, xd[:m], wd, None, what)  # bias = None
            err, bound = (n64.cpu() - want_nb[:m]).abs(), 2 * (k + 8) * U * mag[:m]
            worst = max(worst, float((err / bound).max()))
            assert bool((err <= bound).all()), what
            # a row's bits: the same in a column window of a wider matrix, in a shuffled batch, in a longer batch
            s64, s32 = _head_both(L, wide[:m, 4:4 + k], wd, bd, what)
            assert torch.equal(s64, y64) and torch.equal(s32, y32), what
            p = torch.randperm(m, generator=g).cuda()
            p64, p32 = _head_both(L, xd[:m][p].contiguous(), wd, bd, what)
            assert torch.equal(p64, y64[p]) and torch.equal(p32, y32[p]), what
            if full is None:
                full = y64
            assert torch.equal(y64, full[:m]), what
    print("RATIO head_gemv64 random data: worst error / bound = %.4f" % worst)


@torch.no_grad()
def test_head_gemv_grid_stride_second_trip():
    """m = 32771: the launch caps the grid at 8192 workgroups of four rows, so rows 32768.. are a workgroup's second trip
    (r += gridDim.x * 4) — for fp32, fp16 and bf16 rows, float64 rows rounded to fp32, and dca_head_gemv64."""
    L = _L()
    m, k, n_out = 32771, 4, 2
    g = torch.Generator().manual_seed(32771)
    x = torch.randn((m, k), generator=g, dtype=torch.float64)
    w = torch.randn((n_out, k), generator=g)
    b = torch.randn((n_out,), generator=g)
    wd, bd = w.cuda(), b.cuda()
    y64, y32 = _head_both(L, x.cuda(), wd, bd, "float64 rows")
    want = x @ w.double().t() + b.double()
    bound = 2 * (k + 8) * U * (x.abs() @ w.double().abs().t() + b.double().abs())
    err = (y64.cpu() - want).abs()
    print("RATIO head_gemv64 m = 32771: worst error / bound = %.4f" % float((err / bound).max()))
    assert bool((err <= bound).all())
    assert bool((err[32768:] <= bound[32768:]).all())  # (named: the second trip's rows)
    for dt in (torch.float32, torch.float16, torch.bfloat16):
        xs = x.to(dt)
        out = _nan(m + 1, n_out, torch.float32)
        L.head_gemv(xs.cuda(), wd, bd, out=out[:m])
        assert bool(torch.isnan(out[m]).all()) and not bool(torch.isnan(out[:m]).any()), dt
        ref = xs.double() @ w.double().t() + b.double()  # x as stored (exact in float64)
        scale = float((xs.double().abs() @ w.double().abs().t()).max()) + 1.0
        err = (out[:m].cpu().double() - ref).abs()
        print("RATIO head_gemv m = 32771 %s rows: worst error / (2e-6 * scale) = %.4f" % (dt, float(err.max()) / (2e-6 * scale)))
        assert float(err.max()) <= 2e-6 * scale and float(err[32768:].max()) <= 2e-6 * scale, dt


# --------------------------------------------------------------------------------------------------------------- refusals
def _p(t, off=0):
    return C.c_void_p(0 if t is None else t.data_ptr() + off)


def test_bad_arguments_are_refused_before_anything_is_launched():
    """Every DCA_ARG condition of dca_gemm64, dca_l1_embed64, dca_head_gemv and dca_head_gemv64: DCA_E_BADARG (-1), the error
    text names the condition (the embedding's geometry refusal has its own text), and no output is touched.  Every buffer is
    large enough for the call as written."""
    L_ = _L()
    L = L_.lib()
    i64 = C.c_int64
    st = L_.stream_ptr()
    ones = lambda *s, dt=torch.float64: torch.ones(s, dtype=dt, device="cuda")
    # dca_gemm64: 8 x 8 x 8 in 16 x 16 buffers
    ga, gw, gb, gs, go = ones(16, 16), ones(16, 16), ones(16), ones(16, 16), _nan(16, 16)

    def gemm(a=ga, aoff=0, m=8, k=8, lda=16, w=gw, woff=0, n=8, ldw=16, skip=None, out=go, ldo=16):
        return L.dca_gemm64(_p(a, aoff), i64(m), k, i64(lda), _p(w, woff), n, i64(ldw), _p(gb), _p(skip), 1, _p(out), i64(ldo), st)

    # dca_l1_embed64: (2, 4) into 16 columns; the table buffer holds (64, 64)'s 4096 rows, the states 64 bytes per row
    en, ew, eb, eo = torch.zeros((8, 64), dtype=torch.uint8, device="cuda"), ones(4096, 16), ones(16), _nan(8, 16)

    def embed(nn=en, m=8, d=2, depth=4, w=ew, n_pad=16, b=eb, out=eo):
        return L.dca_l1_embed64(_p(nn), i64(m), d, depth, _p(w), i64(n_pad), _p(b), 0, _p(out), st)

    # the output layer: 8 rows of k = 8 at ldx = 16, 2 outputs; buffers hold k = 2052 / n_out = 9 as written
    hx = {6: ones(8, 2064), 0: ones(8, 2064, dt=torch.float32), 1: ones(8, 2064, dt=torch.float16), 2: ones(8, 2064, dt=torch.bfloat16)}
    hw, hb = ones(9, 2064, dt=torch.float32), ones(16, dt=torch.float32)
    ho32, ho64 = _nan(8, 16, torch.float32), _nan(8, 16)

    def head(dt=6, x=0, xoff=0, m=8, k=8, ldx=16, w=hw, woff=0, n_out=2, out=ho32):
        return L.dca_head_gemv(_p(hx.get(dt, hx[2]) if x == 0 else x, xoff), dt, i64(m), k, i64(ldx), _p(w, woff), _p(hb), n_out, _p(out), st)

    def head64(x=hx[6], xoff=0, m=8, k=8, ldx=16, w=hw, woff=0, n_out=2, out=ho64):
        return L.dca_head_gemv64(_p(x, xoff), i64(m), k, i64(ldx), _p(w, woff), _p(hb), n_out, _p(out), st)

    bad = [
        ("gemm64 null a", lambda: gemm(a=None)), ("gemm64 null w", lambda: gemm(w=None)), ("gemm64 null out", lambda: gemm(out=None)),
        ("gemm64 m < 0", lambda: gemm(m=-1)), ("gemm64 k = 0", lambda: gemm(k=0)), ("gemm64 odd k", lambda: gemm(k=7)),
        ("gemm64 n = 0", lambda: gemm(n=0)), ("gemm64 lda < k", lambda: gemm(lda=6)), ("gemm64 ldw < k", lambda: gemm(ldw=6)),
        ("gemm64 ldo < n", lambda: gemm(ldo=6)), ("gemm64 odd lda", lambda: gemm(lda=9)), ("gemm64 odd ldw", lambda: gemm(ldw=9)),
        ("gemm64 misaligned a", lambda: gemm(aoff=8, m=7)), ("gemm64 misaligned w", lambda: gemm(woff=8, n=7)),
        ("gemm64 out == a", lambda: gemm(out=ga)), ("gemm64 skip == a", lambda: gemm(skip=ga)),
        ("embed64 null nnet_in", lambda: embed(nn=None)), ("embed64 null w_t", lambda: embed(w=None)),
        ("embed64 null bias", lambda: embed(b=None)), ("embed64 null out", lambda: embed(out=None)), ("embed64 m < 0", lambda: embed(m=-1)),
        ("embed64 depth = 0", lambda: embed(depth=0)), ("embed64 depth = 257", lambda: embed(depth=257)),
        ("embed64 n_pad = 0", lambda: embed(n_pad=0)), ("embed64 n_pad = 12", lambda: embed(n_pad=12)),
        ("embed64 state_dim = 0", lambda: embed(d=0)),
    ]
    for name, call, o in (("head_gemv", head, ho32), ("head_gemv64", head64, ho64)):
        bad += [
            (name + " null x", lambda c=call: c(x=None)), (name + " null w", lambda c=call: c(w=None)),
            (name + " null out", lambda c=call: c(out=None)), (name + " m < 0", lambda c=call: c(m=-1)),
            (name + " k = 0", lambda c=call: c(k=0)), (name + " k = 6", lambda c=call: c(k=6)),
            (name + " ldx < k", lambda c=call: c(ldx=4)), (name + " ldx % 4", lambda c=call: c(ldx=10)),
            (name + " n_out = 0", lambda c=call: c(n_out=0)), (name + " n_out = 9", lambda c=call: c(n_out=9)),
            (name + " n_out * k * 4 > 64 KB", lambda c=call: c(k=2052, ldx=2064, n_out=8)),
            (name + " misaligned x", lambda c=call: c(xoff=8, m=7)), (name + " misaligned w", lambda c=call: c(woff=4, n_out=1)),
        ]
    bad += [("head_gemv dtype 4", lambda: head(dt=4)), ("head_gemv dtype 5", lambda: head(dt=5)), ("head_gemv dtype 3", lambda: head(dt=3)),
            ("head_gemv misaligned fp32 x", lambda: head(dt=0, xoff=4, m=7)), ("head_gemv misaligned fp16 x", lambda: head(dt=1, xoff=2, m=7)),
            ("head_gemv misaligned bf16 x", lambda: head(dt=2, xoff=4, m=7))]
    for what, call in bad:
        assert call() == -1, what  # DCA_E_BADARG
        assert L.dca_last_error().decode().startswith("bad argument: "), (what, L.dca_last_error().decode())
    assert embed(d=64, depth=64) == -1
    assert "geometry (64, 64) does not fit LDS" in L.dca_last_error().decode()
    torch.cuda.synchronize()
    for o in (go, eo, ho32, ho64):
        assert bool(torch.isnan(o).all())
    assert bool((ga == 1.0).all())
    # the same calls with good arguments go through (the harness above is not what refuses them)
    assert gemm() == 0 and gemm(skip=gs) == 0 and embed() == 0 and head64() == 0
    assert all(head(dt=dt) == 0 for dt in (6, 0, 1, 2))
    torch.cuda.synchronize()
    assert bool((go[:8, :8] == 10.0).all()) and bool(torch.isnan(go[:8, 8:]).all()) and bool(torch.isnan(go[8:]).all())  # 8 + bias + skip
    assert bool((eo == 3.0).all())  # bias + two positions
    assert bool((ho64.view(-1)[:16] == 9.0).all()) and bool((ho32.view(-1)[:16] == 9.0).all())  # [8, 2], packed
    assert bool(torch.isnan(ho64.view(-1)[16:]).all()) and bool(torch.isnan(ho32.view(-1)[16:]).all())
    # and the wrappers turn a refusal into DcaError
    with pytest.raises(L_.DcaError, match="bad argument"):
        L_.gemm64(ga[:8, :7], gw[:8, :7], None, None, False)  # odd k


# ----------------------------------------------------------------------------------------- the narrow network, by value
@pytest.mark.parametrize("d,depth", GEOMETRIES)
@torch.no_grad()
def test_narrow_networks_against_the_module_in_float64_on_the_host(d, depth):
    """64/32 (one block) and 100/40 (two blocks) networks — h1 padded to 64 / 128, the residual width to 64, so dca_gemm64
    runs single-tile and partly idle — against the module itself in float64 on the CPU, on one-hot rows: the bar of
    test_fp64_at_scale_against_library_float64, <= 1e-9 max(1, |h|)."""
    from deepcubea_amd.utils.pytorch_models import Fp64Resnet, ResnetModel
    from deepcubea_amd.utils.synthetic_weights import load_synthetic_weights
    _L()
    for h1, r, nb in ((64, 32, 1), (100, 40, 2)):
        net = ResnetModel(d, depth, h1, r, nb, 1, True)
        load_synthetic_weights(net, 2028 + h1)
        net.eval()
        f = Fp64Resnet(net).cuda()
        ref = copy.deepcopy(net).double().eval()
        g = torch.Generator().manual_seed(d + depth + h1)
        x = torch.randint(0, depth, (1030, d), generator=g, dtype=torch.uint8)
        oh = torch.nn.functional.one_hot(x.long(), depth).view(x.shape[0], -1).double()
        want = ref.forward_onehot(oh)
        xd = x.cuda()
        whole = f.forward64(xd)
        for m in (1, 5, 1030):
            y = f.forward64(xd[:m].contiguous())
            rel = float(((y.cpu() - want[:m]).abs() / want[:m].abs().clamp_min(1.0)).max())
            print("NARROW (%d, %d) %d/%d m=%d: max |fp64 mode - module float64| / max(1, |h|) = %.3e, max |h| = %.3f"
                  % (d, depth, h1, r, m, rel, float(want[:m].abs().max())))
            assert rel <= 1e-9, (d, depth, h1, r, m, rel)
            assert torch.equal(f(xd[:m].contiguous()), y.float())  # one rounding, at the end
            assert torch.equal(y, whole[:m])
        for row in (0, 1029):
            assert torch.equal(f.forward64(xd[row:row + 1].contiguous())[0], whole[row]), row
