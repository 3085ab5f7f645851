"""GPU tests of the four operand-preparation kernels of the training step's dense layers (csrc/dca_gemm.hip: dca_absmax_bits,
dca_split_planes_scaled, dca_split_rows_scaled, dca_fill_inv_pow2), called directly through their `_lib` wrappers and compared
BIT FOR BIT with the same arithmetic written in a few lines of torch on the host.  The arithmetic is exact and deterministic:

    ex = ((bits >> 23) & 0xFF) - 127;  s = 2^(14 - ex) if -100 <= ex <= 100 else 1
    hi = (x * s).half();  lo = (x * s - hi.float()).half()

Next to the bit patterns stands one property that does not share the emulation's reading of the design:
|(hi + lo) / s - x| <= 2^-21 * amax (amax of the tensor, or of the row for the row kernel).  The output buffers are pre-filled
with fp16 NaN bits, so a pad column that a kernel leaves unwritten cannot pass by the allocator's luck."""
import ctypes as C

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

NAN16 = 0x7E00  # fp16 quiet NaN: the fill of every output buffer
SHAPES = [(1, 4, 64), (3, 68, 128), (300, 324, 384), (777, 1000, 1024), (2048, 5000, 5056), (4099, 5000, 5056)]


# ------------------------------------------------------------------------------ the host's copy of the arithmetic
def _bits(x: torch.Tensor) -> torch.Tensor:
    return x.contiguous().view(torch.int32)


def _absmax_bits_ref(x: torch.Tensor) -> int:
    """max over the bit patterns of |x| (non-negative floats, inf and NaN included, order like their bits)."""
    if x.numel() == 0:
        return 0
    return int((_bits(x) & 0x7FFFFFFF).max())


def _scale_ref(bits: int) -> float:
    ex = ((bits >> 23) & 0xFF) - 127
    return 2.0 ** (14 - ex) if -100 <= ex <= 100 else 1.0


def _planes_ref(x: torch.Tensor, s: float):
    u = x * torch.tensor(s, dtype=torch.float32)  # a power of two: only the exponent moves
    hi = u.half()
    lo = (u - hi.float()).half()
    return hi, lo


def _h16(t: torch.Tensor) -> torch.Tensor:
    return t.contiguous().view(torch.int16).cpu()


def _filled(shape, dev="cuda") -> torch.Tensor:
    return torch.full(shape, NAN16, dtype=torch.int16, device=dev).view(torch.float16)


def _assert_planes(out: torch.Tensor, x: torch.Tensor, s: float, n: int, n_pad: int, amax: float, prop: bool):
    """out [2, m, ldo] from the device against the host arithmetic on x [m, n] (cpu): data, pad and what lies beyond the pad."""
    hi, lo = _planes_ref(x, s)
    o = _h16(out)
    assert torch.equal(o[0, :, :n], _h16(hi)), "high plane"
    assert torch.equal(o[1, :, :n], _h16(lo)), "low plane"
    assert not bool((o[:, :, n:n_pad] != 0).any()), "pad columns are +0"
    if out.shape[2] > n_pad:
        assert bool((o[:, :, n_pad:] == NAN16).all()), "columns beyond n_pad keep the fill"
    if prop:
        got = (out[0, :, :n].double().cpu() + out[1, :, :n].double().cpu()) / s
        assert float((got - x.double()).abs().max()) <= 2.0 ** -21 * amax


def _spread(m: int, n: int, seed: int, binades: float = 20.0) -> torch.Tensor:
    g = torch.Generator().manual_seed(seed)
    return torch.randn(m, n, generator=g) * torch.exp2(-binades * torch.rand(m, n, generator=g)) * 3.0e-3


# ------------------------------------------------------------------------------ whole-tensor scale: absmax + planes
@pytest.mark.parametrize("m,n,n_pad", SHAPES)
def test_absmax_and_scaled_planes_bit_for_bit_at_every_shape(m, n, n_pad):
    """Contiguous source, ldo == n_pad and ldo > n_pad, scaled and unscaled.  All shapes but the first two exceed one wave of
    workgroups; (2048, 5000) and (4099, 5000) exceed the 768-block cap of k_absmax_bits by far, the last one also the
    8192-block cap of the split kernel (its grid-stride loop runs more than once)."""
    from deepcubea_amd import _lib
    _lib.require_gpu()
    x = _spread(m, n, 1000 * m + n)
    xd = x.cuda()
    bits = _lib.absmax_bits(xd)
    want_bits = _absmax_bits_ref(x)
    assert int(bits.item()) == want_bits
    s = _scale_ref(want_bits)
    amax = float(x.abs().max())
    assert 2.0 ** 14 <= amax * s < 2.0 ** 15
    for ldo in (n_pad, n_pad + 8):
        out = _lib.split_planes_scaled(xd, bits, n_pad=n_pad, ldo=ldo, out=_filled((2, m, ldo)))
        _assert_planes(out, x, s, n, n_pad, amax, prop=True)
    x1 = torch.randn(m, n, generator=torch.Generator().manual_seed(m)) * 4.0  # unscaled: amax_bits == NULL
    out = _lib.split_planes_scaled(x1.cuda(), None, n_pad=n_pad, out=_filled((2, m, n_pad)))
    _assert_planes(out, x1, 1.0, n, n_pad, float(x1.abs().max()), prop=False)
    # the wrapper's defaults: n_pad = n, freshly allocated planes
    out = _lib.split_planes_scaled(xd, bits)
    assert tuple(out.shape) == (2, m, n)
    _assert_planes(out, x, s, n, n, amax, prop=True)


@pytest.mark.parametrize("other", ["larger", "nan"])
@pytest.mark.parametrize("m,n,n_pad", [(3, 68, 128), (300, 324, 384), (2048, 5000, 5056)])
def test_strided_source_neighbours_reach_neither_the_max_nor_the_planes(m, n, n_pad, other):
    """ld > n: the operand is a column slice of a wider matrix whose other columns hold a larger value / a NaN."""
    from deepcubea_amd import _lib
    _lib.require_gpu()
    x = _spread(m, n, 77 * m + n)
    wide = torch.full((m, n + 12), 1.0e6 if other == "larger" else float("nan"))
    wide[:, 4:4 + n] = x
    wd = wide.cuda()
    view = wd[:, 4:4 + n]
    assert view.stride(0) == n + 12 and not view.is_contiguous()
    bits = _lib.absmax_bits(view)
    want_bits = _absmax_bits_ref(x)
    assert int(bits.item()) == want_bits
    s = _scale_ref(want_bits)
    out = _lib.split_planes_scaled(view, bits, n_pad=n_pad, ldo=n_pad + 4, out=_filled((2, m, n_pad + 4)))
    _assert_planes(out, x, s, n, n_pad, float(x.abs().max()), prop=True)
    # the same through explicit m / n / ld on the wide buffer's own storage
    bits2 = _lib.absmax_bits(wd.view(-1)[4:].view(1, -1), m=m, n=n, ld=n + 12)
    assert int(bits2.item()) == want_bits


def _nan32(bits: int) -> float:
    return float(np.array([bits], np.uint32).view(np.float32)[0])


@pytest.mark.parametrize("case", ["first", "last", "negative", "minus_zero", "zeros", "nan", "negative_nan", "inf", "nan_and_inf"])
def test_where_the_maximum_sits(case):
    """(2048, 1000): 2000 workgroups' worth of elements on the 768 k_absmax_bits launches, so every thread loops."""
    from deepcubea_amd import _lib
    _lib.require_gpu()
    m, n = 2048, 1000
    x = _spread(m, n, 9)
    big = 7.0
    special = None
    if case == "first":
        x[0, 0] = big
    elif case == "last":
        x[m - 1, n - 1] = big
    elif case == "negative":
        x[1000, 501] = -big
    elif case == "minus_zero":
        x = torch.zeros(m, n)
        x[5, 7] = -0.0
        assert int(_bits(x)[5, 7]) == -2 ** 31
    elif case == "zeros":
        x = torch.zeros(m, n)
    elif case == "nan":
        special = 0x7FC01234
        _bits_view = x.view(torch.int32)
        _bits_view[1234, 567] = special
    elif case == "negative_nan":
        special = 0x7FC00001
        x.view(torch.int32)[m - 1, n - 1] = special - 2 ** 31  # sign bit set: |.| clears it
    elif case == "inf":
        x[17, 3] = float("-inf")
        special = 0x7F800000
    elif case == "nan_and_inf":
        x[17, 3] = float("inf")
        x.view(torch.int32)[0, 1] = 0x7FC00000
        special = 0x7FC00000
    xd = x.cuda()
    sentinel = torch.full((1,), 0x55555555, dtype=torch.int32, device="cuda")
    bits = _lib.absmax_bits(xd, out=sentinel)
    got = int(bits.item())
    if case in ("first", "last", "negative"):
        assert got == int(_bits(torch.tensor([big]))[0])
    elif case in ("minus_zero", "zeros"):
        assert got == 0
    else:
        assert got == special
    assert got == _absmax_bits_ref(x)
    inv = _lib.fill_inv_pow2(bits, 5)
    w = torch.ones(8, 64, device="cuda")
    _, cs = _lib.split_rows_scaled(w, bits)
    if case in ("first", "last", "negative"):
        assert torch.equal(inv.cpu(), torch.full((5,), 2.0 ** (2 - 14)))  # 7 = 1.75 * 2^2
        assert torch.equal(cs.cpu(), torch.full((8,), 2.0 ** -14 * 2.0 ** (2 - 14)))
    else:  # zero / NaN / inf: the scale is left at 1
        assert torch.equal(inv.cpu(), torch.ones(5))
        assert torch.equal(cs.cpu(), torch.full((8,), 2.0 ** -14))
    if case in ("minus_zero", "zeros"):
        out = _lib.split_planes_scaled(xd, bits, n_pad=1024, out=_filled((2, m, 1024)))
        o = _h16(out)
        assert not bool((o[1] != 0).any()) and int((o[0] & 0x7FFF).max()) == 0  # (hi of -0.0 is -0.0, its lo +0)
        _assert_planes(out, x, 1.0, n, 1024, 0.0, prop=True)


def test_absmax_of_zero_rows_zeroes_the_output_word():
    from deepcubea_amd import _lib
    _lib.require_gpu()
    buf = torch.full((4, 8), 3.0, device="cuda")
    word = torch.full((1,), 0x55555555, dtype=torch.int32, device="cuda")
    _lib.absmax_bits(buf, m=0, n=8, ld=8, out=word)
    assert int(word.item()) == 0
    planes = _filled((2, 4, 8))
    i64 = C.c_int64  # m == 0 with real output pointers (the wrapper's own planes would be empty): accepted, nothing is written
    assert _lib.lib().dca_split_planes_scaled(_p(buf), i64(0), i64(8), i64(8), _p(word), _p(planes[0]), _p(planes[1]), i64(8), i64(8),
                                              _lib.stream_ptr()) == 0
    assert bool((_h16(planes) == NAN16).all())


# ------------------------------------------------------------------------------ the scale's edges
EDGE_E = [-127, -101, -100, -99, -15, 0, 15, 99, 100, 101]


@pytest.mark.parametrize("e", EDGE_E)
def test_scale_is_exactly_two_to_the_14_minus_e_inside_the_range_and_one_outside(e):
    """amax = 2^e * {1, 1.5, 2 - 2^-23}: the first and the last value of a binade and one between.  Inside [-100, 100] the scale
    is 2^(14 - e) exactly; outside (e = -127 is a denormal amax) it is 1.  dca_fill_inv_pow2 writes its exact reciprocal into
    every element, the row kernel's col_scale is 1 / (row scale * this scale) bit for bit."""
    from deepcubea_amd import _lib
    _lib.require_gpu()
    g = torch.Generator().manual_seed(e + 500)
    for mant in (1.0, 1.5, 2.0 - 2.0 ** -23):
        amax64 = mant * 2.0 ** e
        amax = float(torch.tensor(amax64, dtype=torch.float64).float())
        x = ((torch.rand(8, 64, generator=g, dtype=torch.float64) * 2 - 1) * amax64 * 0.99).float()
        x[3, 17] = -amax
        assert float(x.abs().max()) == amax
        xd = x.cuda()
        bits = _lib.absmax_bits(xd)
        want_bits = _absmax_bits_ref(x)
        assert int(bits.item()) == want_bits
        ex = ((want_bits >> 23) & 0xFF) - 127
        inside = -100 <= e <= 100
        if e > -127 and mant < 1.9:
            assert ex == e
        s = _scale_ref(want_bits)
        assert s == (2.0 ** (14 - e) if inside else 1.0)
        inv = _lib.fill_inv_pow2(bits, 1000)  # not a multiple of 256
        assert torch.equal(inv.cpu(), torch.full((1000,), 1.0 / s, dtype=torch.float32))
        out = _lib.split_planes_scaled(xd, bits, n_pad=128, ldo=136, out=_filled((2, 8, 136)))
        _assert_planes(out, x, s, 64, 128, amax, prop=inside)
        # the row kernel on the same matrix (every row its own scale) with this tensor as the OTHER operand, and with none
        for other in (bits, None):
            so = s if other is not None else 1.0
            rows, cs = _lib.split_rows_scaled(xd, other, k_pad=128, ldo=136, out=_filled((2, 8, 136)))
            _assert_rows(rows, cs, x, so, 64, 128, prop=inside)


def test_fill_inv_pow2_covers_more_than_its_grid():
    """n above 1024 * 256: the grid-stride loop of k_fill_inv_pow2 runs twice; the guard element behind n is not written."""
    from deepcubea_amd import _lib
    _lib.require_gpu()
    n = 1024 * 256 + 777
    bits = torch.tensor([int(_bits(torch.tensor([3.0e-5]))[0])], dtype=torch.int32, device="cuda")
    buf = torch.full((n + 3,), -7.0, device="cuda")
    _lib.fill_inv_pow2(bits, n, out=buf)
    s = _scale_ref(int(bits.item()))
    assert s == 2.0 ** 30  # 3e-5 = 1.97 * 2^-16
    assert torch.equal(buf[:n].cpu(), torch.full((n,), 2.0 ** -30)) and torch.equal(buf[n:].cpu(), torch.full((3,), -7.0))
    _lib.fill_inv_pow2(bits, 0, out=buf)  # n == 0: nothing happens
    assert float(buf[0]) == 2.0 ** -30


# ------------------------------------------------------------------------------ per-row scales
def _assert_rows(out: torch.Tensor, cs: torch.Tensor, w: torch.Tensor, s_other: float, k: int, k_pad: int, prop: bool = True):
    """out [2, n, ldo] and col_scale [n] from the device against the host arithmetic, row by row (vectorised)."""
    n = w.shape[0]
    rb = (_bits(w) & 0x7FFFFFFF).amax(dim=1)
    ex = ((rb >> 23) & 0xFF) - 127
    ok = (ex >= -100) & (ex <= 100)
    s = torch.where(ok, ((127 + 14 - ex).clamp(1, 254).to(torch.int32) << 23).view(torch.float32), torch.ones(n))  # 2^(14 - ex)
    u = w * s[:, None]
    hi = u.half()
    lo = (u - hi.float()).half()
    o = _h16(out)
    assert torch.equal(o[0, :, :k], _h16(hi)), "high plane"
    assert torch.equal(o[1, :, :k], _h16(lo)), "low plane"
    assert not bool((o[:, :, k:k_pad] != 0).any()), "pad columns are +0"
    if out.shape[2] > k_pad:
        assert bool((o[:, :, k_pad:] == NAN16).all()), "columns beyond k_pad keep the fill"
    want_cs = (1.0 / s) * torch.tensor(1.0 / s_other, dtype=torch.float32)
    assert torch.equal(_bits(cs.cpu()), _bits(want_cs)), "col_scale"
    if prop:
        got = (out[0, :, :k].double().cpu() + out[1, :, :k].double().cpu()) / s.double()[:, None]
        err = (got - w.double()).abs().amax(dim=1)
        amax = w.double().abs().amax(dim=1)
        assert bool((err[ok] <= 2.0 ** -21 * amax[ok]).all())


def _row_matrix(n: int, k: int, seed: int) -> torch.Tensor:
    """Rows whose magnitudes span 40 binades, plus the rows where a reduction goes wrong: all zero, only the last element set,
    only the first, the maximum in each of the four waves' share of the first pass, denormals."""
    g = torch.Generator().manual_seed(seed)
    w = torch.randn(n, k, generator=g) * torch.exp2(-40.0 * torch.rand(n, 1, generator=g))
    w[1] = 0.0
    w[2] = 0.0
    w[2, k - 1] = -3.0e-9
    w[3] = 0.0
    w[3, 0] = 5.0e4
    w[4] = (torch.rand(k, generator=g) * 2 - 1) * 1.0e-40  # denormals: scale 1, planes zero
    for j, row in enumerate(range(5, 9)):  # the row's maximum under lane 0 of wave j (columns 256 j .. 256 j + 3), where there is one
        col = min(256 * j, k - 4)
        w[row, col] = 1.0e3
    w[9, :] = torch.exp2(-40.0 * torch.rand(k, generator=g))  # 40 binades within ONE row
    return w


@pytest.mark.parametrize("n,k", [(300, 4), (300, 1024), (1000, 5000), (5000, 324)])
def test_split_rows_scaled_bit_for_bit(n, k):
    """k = 4: one lane has data; k = 1024: every lane exactly once; k = 5000: the 256-thread loop wraps (1250 float4 per row).
    With the other operand's |max| given and with NULL, ldo == k_pad and ldo > k_pad, contiguous source and a column slice."""
    from deepcubea_amd import _lib
    _lib.require_gpu()
    k_pad = (k + 63) // 64 * 64
    w = _row_matrix(n, k, n + k)
    wd = w.cuda()
    other_val = torch.tensor([2.5e-6])
    other = _bits(other_val).cuda()
    s_other = _scale_ref(int(other.item()))
    assert s_other == 2.0 ** 33  # 2.5e-6 = 1.31 * 2^-19
    for oth, so in ((other, s_other), (None, 1.0)):
        for ldo in (k_pad, k_pad + 8):
            out, cs = _lib.split_rows_scaled(wd, oth, k_pad=k_pad, ldo=ldo, out=_filled((2, n, ldo)),
                                             col_scale=torch.full((n,), float("nan"), device="cuda"))
            _assert_rows(out, cs, w, so, k, k_pad)
    # all-zero row: scale 1, planes zero, col_scale = 1 / s_other
    out, cs = _lib.split_rows_scaled(wd, other, k_pad=k_pad)
    assert float(cs[1]) == 2.0 ** -33 and not bool((_h16(out)[:, 1] != 0).any())
    assert float(cs[4]) == 2.0 ** -33 and int((_h16(out)[:, 4] & 0x7FFF).max()) == 0  # denormal row
    # strided source: a column slice whose neighbours are larger / NaN
    wide = torch.full((n, k + 8), float("nan"))
    wide[:, :4] = 1.0e9
    wide[:, 4:4 + k] = w
    view = wide.cuda()[:, 4:4 + k]
    out, cs = _lib.split_rows_scaled(view, other, k_pad=k_pad, ldo=k_pad + 4, out=_filled((2, n, k_pad + 4)))
    _assert_rows(out, cs, w, s_other, k, k_pad)


# ------------------------------------------------------------------------------ refused arguments
def _p(t, off=0):
    return C.c_void_p(0) if t is None else C.c_void_p(t.data_ptr() + off)


def test_bad_arguments_are_refused_before_anything_is_launched():
    """Every DCA_ARG condition of the four entry points: DCA_E_BADARG (-1), the error text names the condition, and neither the
    output word nor the planes nor col_scale are touched (dca_absmax_bits zeroes its word only after the checks)."""
    from deepcubea_amd import _lib
    _lib.require_gpu()
    L = _lib.lib()
    i64 = C.c_int64
    st = _lib.stream_ptr()
    x = torch.ones(16, 64, device="cuda")
    word = torch.full((1,), 0x55555555, dtype=torch.int32, device="cuda")
    planes = _filled((2, 16, 136))
    cs = torch.full((16,), -7.0, device="cuda")
    inv = torch.full((16,), -7.0, device="cuda")
    oh, ol = planes[0], planes[1]

    def absmax(xx=x, xoff=0, m=16, n=64, ld=64, out=word):
        return L.dca_absmax_bits(_p(xx, xoff), i64(m), i64(n), i64(ld), _p(out), st)

    def planes_(xx=x, xoff=0, m=16, n=64, ld=64, h=oh, l_=ol, hoff=0, ldo=136, n_pad=128):
        return L.dca_split_planes_scaled(_p(xx, xoff), i64(m), i64(n), i64(ld), _p(word), _p(h, hoff), _p(l_), i64(ldo), i64(n_pad), st)

    def rows_(ww=x, woff=0, n=16, k=64, ld=64, h=oh, l_=ol, hoff=0, ldo=136, k_pad=128, c=cs):
        return L.dca_split_rows_scaled(_p(ww, woff), i64(n), i64(k), i64(ld), _p(h, hoff), _p(l_), i64(ldo), i64(k_pad), _p(c), _p(word), st)

    def fill_(out=inv, n=16, am=word):
        return L.dca_fill_inv_pow2(_p(out), i64(n), _p(am), st)

    bad = [
        ("absmax n % 4", lambda: absmax(n=62)), ("absmax n < 4", lambda: absmax(n=0)), ("absmax ld < n", lambda: absmax(ld=60)),
        ("absmax ld % 4", lambda: absmax(n=60, ld=62)), ("absmax m < 0", lambda: absmax(m=-1)),
        ("absmax misaligned x", lambda: absmax(xoff=4, m=15)), ("absmax null x", lambda: absmax(xx=None)),
        ("absmax null out", lambda: absmax(out=None)),
        ("planes n % 4", lambda: planes_(n=62)), ("planes n < 4", lambda: planes_(n=0)), ("planes ld < n", lambda: planes_(ld=60)),
        ("planes ld % 4", lambda: planes_(n=60, ld=62)), ("planes m < 0", lambda: planes_(m=-1)),
        ("planes n_pad < n", lambda: planes_(n_pad=60)), ("planes n_pad % 4", lambda: planes_(n_pad=126)),
        ("planes ldo < n_pad", lambda: planes_(ldo=124)), ("planes ldo % 4", lambda: planes_(ldo=134)),
        ("planes misaligned x", lambda: planes_(xoff=4, m=15)), ("planes misaligned out", lambda: planes_(hoff=2, m=15)),
        ("planes null x", lambda: planes_(xx=None)), ("planes null out_h", lambda: planes_(h=None)),
        ("planes null out_l", lambda: planes_(l_=None)),
        ("rows k % 4", lambda: rows_(k=62)), ("rows k < 4", lambda: rows_(k=0)), ("rows ld < k", lambda: rows_(ld=60)),
        ("rows ld % 4", lambda: rows_(k=60, ld=62)), ("rows n < 0", lambda: rows_(n=-1)), ("rows n >= 2^31", lambda: rows_(n=2 ** 31)),
        ("rows k_pad < k", lambda: rows_(k_pad=60)), ("rows k_pad % 4", lambda: rows_(k_pad=126)),
        ("rows ldo < k_pad", lambda: rows_(ldo=124)), ("rows ldo % 4", lambda: rows_(ldo=134)),
        ("rows misaligned w", lambda: rows_(woff=4, n=15)), ("rows misaligned out", lambda: rows_(hoff=2, n=15)),
        ("rows null w", lambda: rows_(ww=None)), ("rows null out_h", lambda: rows_(h=None)), ("rows null out_l", lambda: rows_(l_=None)),
        ("rows null col_scale", lambda: rows_(c=None)),
        ("fill null out", lambda: fill_(out=None)), ("fill null amax", lambda: fill_(am=None)), ("fill n < 0", lambda: fill_(n=-1)),
    ]
    for what, call in bad:
        assert call() == -1, what  # DCA_E_BADARG
        assert L.dca_last_error().decode().startswith("bad argument: "), what
    torch.cuda.synchronize()
    assert int(word.item()) == 0x55555555
    assert bool((_h16(planes) == NAN16).all())
    assert torch.equal(cs.cpu(), torch.full((16,), -7.0)) and torch.equal(inv.cpu(), torch.full((16,), -7.0))
    # the same calls with good arguments go through (the harness above is not what refuses them)
    assert absmax() == 0 and planes_() == 0 and rows_() == 0 and fill_() == 0
    torch.cuda.synchronize()
    assert int(word.item()) == 0x3F800000 and float(inv[0]) == 2.0 ** -14 and float(cs[0]) == 2.0 ** -28
    # and the wrappers turn a refusal into DcaError
    with pytest.raises(_lib.DcaError, match="bad argument"):
        _lib.absmax_bits(x, n=62)
    with pytest.raises(_lib.DcaError, match="bad argument"):
        _lib.split_planes_scaled(x, word, n_pad=60)
