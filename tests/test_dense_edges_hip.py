"""The inference dense-layer kernels — dca_f16x3_gemm (csrc/dca_gemm.hip), dca_gemm16 (csrc/dca_gemm16.hip), dca_gemm8 and
dca_gemm8_mx (csrc/dca_gemm8.hip) — and the converters dca_split_planes / dca_quant_e4m3 away from the round, contiguous
shapes of the 5000/1000 network: ragged m / n (the element-wise right edge, n = 1, 3, 5, 63, 65, 257, ...), nine M-tiles (the
tile map's second group of eight with its seven exiting workgroups), one K-step up to the schedules' steady state with both
drain paths, row strides larger than the widths, operand and output windows of wider matrices, every layer form, every output
combination, every schedule variant, every compiled tail beside the general one, and every DCA_ARG refusal.  The C ABI is
called directly (ctypes on data pointers), so that strides and offsets reach the kernels.

What is exact, and why.  Every operand is a small integer, or a small integer times a power of two (col_scale, alpha, scale,
w_scale, the E8M0 block scales, out8_scale): each product is then a dyadic number of a few bits, every partial sum of a row's
products — in any order, on any MFMA — is bounded by sum |a||w| < 2^24 units of the data's granularity and therefore exact in
fp32, and so are the scaling, the bias add and the skip add.  The pre-rounding value v is thus fixed, and the outputs bit for
bit: v itself (fp32), torch's round-to-nearest-even of v to fp16 / bf16, `v.clamp(-448, 448).to(float8_e4m3fn)`, and for
f16x3's planes hi = half(v), lo = half(v - hi).  The host evaluates v in float64 and asserts the 2^24 condition before every
comparison (_exact): nothing here carries a tolerance.  The fp8 MFMA, which adds an instruction's 64 products with less than
fp32 precision on general data (tests/test_gemm8_hip.py), is exact on these integers too:
test_fp8_integer_sums_are_exact_in_a_round_interior_tile checks that first, on tiles with no edge in them.

Poison and guards.  Operands live in wider buffers whose padding holds NaN (fp16 / bf16 NaN, the e4m3 NaN byte 0x7F, 0xFF for
E8M0 scale bytes); bias, col_scale, scale and w_scale are n-long windows of longer vectors with NaN on both sides: one padding
element read into a sum poisons it (and raises f16x3's overflow flag, which must stay 0).  Outputs are windows of buffers with
a spare row and spare columns, pre-filled with NaN / 0x7F / 0xA5: after the launch every padding element still holds the fill's
bits and no in-range element is NaN — the kernels write [0, m) x [0, n) and nothing else."""
import ctypes as C

import pytest
import torch

pytestmark = pytest.mark.gpu

F16, BF16, F32, U8 = torch.float16, torch.bfloat16, torch.float32, torch.uint8
E4M3 = torch.float8_e4m3fn
DT_CODE = {F32: 0, F16: 1, BF16: 2}  # DCA_DT_*
BADARG = -1  # DCA_E_BADARG
i64 = C.c_int64
_INT = {F32: torch.int32, F16: torch.int16, BF16: torch.int16}


def _L():
    from deepcubea_amd import _lib
    _lib.require_gpu()
    return _lib


def _p(t, off=0):
    """Data pointer of a tensor or view (+ off bytes); NULL for None."""
    return C.c_void_p(0 if t is None else t.data_ptr() + off)


def _r4(n):
    return (n + 3) // 4 * 4


def _q(x):
    """fp32 -> e4m3 with saturation (what the kernels do), on the host; as bytes."""
    return x.float().clamp(-448.0, 448.0).to(E4M3).view(U8)


def _bits(t):
    return t if t.dtype == U8 else t.view(_INT[t.dtype])


def _poison(rows, cols, dtype, byte=0x7F, dev="cuda"):
    if dtype == U8:
        return torch.full((rows, cols), byte, dtype=U8, device=dev)
    return torch.full((rows, cols), float("nan"), dtype=dtype, device=dev)


def _padded(t, ld, col0=0, byte=0x7F):
    """t [m, w] (cpu) -> its copy on the device as the window [:, col0:col0 + w] of a poisoned [m, ld] buffer."""
    buf = _poison(t.shape[0], ld, t.dtype, byte)
    view = buf[:, col0:col0 + t.shape[1]]
    view.copy_(t)
    assert view.stride(0) == ld
    return view


def _vec(t):
    """t [n] fp32 (cpu) -> an n-long, 16-byte aligned window of a longer device vector with NaN in front and behind."""
    buf = torch.full((t.shape[0] + 8,), float("nan"), dtype=F32, device="cuda")
    view = buf[4:4 + t.shape[0]]
    view.copy_(t)
    assert view.data_ptr() % 16 == 0
    return view


class _Out:
    """An output (or skip) window: rows [0, m), columns [off, off + n) of a poisoned [m + 1, ld] buffer."""

    def __init__(self, m, n, ld, off, dtype, byte=0x7F):
        assert off + n <= ld
        self.m, self.n, self.off, self.byte = m, n, off, byte
        self.buf = _poison(m + 1, ld, dtype, byte)
        self.fill = _bits(self.buf)[0, 0].clone()
        self.view = self.buf[:m, off:off + n]

    def bits(self):
        return _bits(self.view)

    def check(self, what):
        """Every in-range element written (no NaN left), every element outside the window still the fill's bits."""
        if self.view.dtype != U8:
            assert not bool(torch.isnan(self.view).any()), ("an in-range element is NaN", what)
        elif self.byte == 0x7F:
            assert not bool(((self.view & 0x7F) == 0x7F).any()), ("an in-range e4m3 byte is NaN", what)
        b = _bits(self.buf).clone()
        b[:self.m, self.off:self.off + self.n] = self.fill
        assert bool((b == self.fill).all()), ("an element outside [0, m) x [0, n) was written", what)


def _exact(x, gran=1.0):
    """The condition that makes bit equality a theorem: x is a multiple of `gran` and |x| < 2^24 units of it."""
    u = x / gran
    assert bool((u == u.round()).all()) and float(u.abs().max()) < 2.0 ** 24, float(u.abs().max())


def _mm(a, w):
    return torch.from_numpy(a.numpy() @ w.numpy().T)


def _int_problem(m, n, k, seed):
    """max |a.w^T + bias + skip| <= 163 at every shape used here; asymmetric w, distinct rows."""
    g = torch.Generator().manual_seed(seed)
    a = torch.randint(-1, 2, (m, k), generator=g).double()
    a[:, 0] += torch.arange(m, dtype=torch.float64) % 3
    w = torch.randint(-2, 3, (n, k), generator=g).double()
    w[:, 0] += torch.arange(n, dtype=torch.float64) % 5
    bias = torch.randint(-8, 9, (n,), generator=g).double()
    skip = torch.randint(-16, 17, (m, n), generator=g).double()
    return a, w, bias, skip


# (name, lda - k, column offset of a, ldw - k, ldo - r4(n), element offset of out / skip in their rows)
LAYOUTS16 = [("contiguous", 0, 0, 0, 0, 0), ("strided", 8, 0, 16, 4, 0), ("window", 16, 8, 16, 8, 4)]
# every m, n and k of the lists at least once; m, n and k ragged together; the nine M-tiles at the smallest k
SHAPES16 = [(1, 1, 64), (31, 3, 128), (33, 5, 192), (127, 63, 320), (129, 65, 64), (255, 255, 128), (256, 256, 192), (257, 257, 320),
            (513, 515, 64), (257, 260, 64), (2049, 257, 64), (1, 4, 128), (513, 260, 192)]
TAIL_SHAPES = [(513, 515), (257, 260)]  # interior tile(s), a right strip and a bottom strip in one call


# ------------------------------------------------------------------------------------------------------------ dca_f16x3_gemm
def _f16x3_call(L, ah, al, m, k, lda, wh, wl, n, ldw, cs, alpha, bias, skip, relu, oh, ol, x, ldo, ovf):
    return L.lib().dca_f16x3_gemm(_p(ah), _p(al), i64(m), int(k), i64(lda), _p(wh), _p(wl), int(n), i64(ldw), _p(cs), C.c_double(alpha),
                                  _p(bias), _p(skip), int(relu), _p(oh), _p(ol), _p(x), i64(ldo), _p(ovf), L.stream_ptr())


def _f16x3_problem(m, n, k, seed):
    """Independent integer data in each of the four planes: v = ah.wh^T + al.wh^T + ah.wl^T (no lo.lo term)."""
    g = torch.Generator().manual_seed(seed)
    ah = torch.randint(-8, 9, (m, k), generator=g).double()
    ah[:, 0] += torch.arange(m, dtype=torch.float64) % 3
    al = torch.randint(-3, 4, (m, k), generator=g).double()
    wh = torch.randint(-8, 9, (n, k), generator=g).double()
    wh[:, 0] += torch.arange(n, dtype=torch.float64) % 5
    wl = torch.randint(-3, 4, (n, k), generator=g).double()
    cs = torch.pow(torch.tensor(2.0, dtype=torch.float64), (torch.arange(n) % 4 - 2).double())  # 1/4, 1/2, 1, 2 by column
    bias = torch.randint(-8, 9, (n,), generator=g).double()
    skip = torch.randint(-16, 17, (m, n), generator=g).double()
    prod = _mm(ah, wh) + _mm(al, wh) + _mm(ah, wl)
    _exact(_mm(ah.abs(), wh.abs()) + _mm(al.abs(), wh.abs()) + _mm(ah.abs(), wl.abs()))  # bounds every partial sum
    return ah, al, wh, wl, cs, bias, skip, prod


def _f16x3_want(prod, cs, alpha, bias, skip, relu):
    """(fp32 result, high plane, low plane) as device bit patterns, from the host's float64 value."""
    v = prod * alpha * (cs if cs is not None else 1.0)
    _exact(v, 2.0 ** -3)
    v = v + (bias if bias is not None else 0.0) + (skip if skip is not None else 0.0)
    _exact(v, 2.0 ** -3)
    assert float(v.abs().max()) <= 60000.0
    x = (v.relu() if relu else v).float()
    hi = x.half()
    lo = (x - hi.float()).half()
    return _bits(x).cuda(), _bits(hi).cuda(), _bits(lo).cuda()


# (name, col_scale, alpha, bias, skip, relu)
F16X3_FORMS = [("plain", False, 1.0, False, False, False), ("bias_relu", True, 0.5, True, False, True),
               ("bias_skip_relu", True, 1.0, True, True, True), ("skip_no_bias", True, 1.0, False, True, True),
               ("no_relu", True, 0.5, True, True, False)]
F16X3_OUTS = [("planes", True, False), ("fp32", False, True), ("both", True, True)]


@pytest.mark.parametrize("m,n,k", SHAPES16)
@torch.no_grad()
def test_f16x3_exact_at_ragged_shapes_strides_and_windows(m, n, k):
    """Every form x every output combination x three layouts x schedule variants 2 and 3, bit for bit against the host: the
    fp32 result, and the planes as the host split of it.  The overflow flag stays 0."""
    L = _L()
    ah, al, wh, wl, cs, bias, skip, prod = _f16x3_problem(m, n, k, 1000 * m + 10 * n + k)
    wants = {name: _f16x3_want(prod, cs if use_cs else None, alpha, bias if use_b else None, skip if use_s else None, relu)
             for name, use_cs, alpha, use_b, use_s, relu in F16X3_FORMS}
    csd, bd, skd = _vec(cs.float()), _vec(bias.float()), skip.float().cuda()
    ovf = torch.zeros(4, dtype=torch.int32, device="cuda")
    try:
        for lname, a_pad, a_off, w_pad, o_pad, o_off in LAYOUTS16:
            lda, ldw, ldo = k + a_pad, k + w_pad, _r4(n) + o_pad
            ahd, ald = _padded(ah.half(), lda, a_off), _padded(al.half(), lda, a_off)
            whd, wld = _padded(wh.half(), ldw), _padded(wl.half(), ldw)
            assert ahd.data_ptr() % 16 == 0 and (a_off == 0 or ahd.data_ptr() != ahd.untyped_storage().data_ptr())
            for variant in (2, 3):
                L.f16x3_gemm_variant(variant)
                for name, use_cs, alpha, use_b, use_s, relu in F16X3_FORMS:
                    for oname, planes, fp32 in F16X3_OUTS:
                        what = (m, n, k, lname, variant, name, oname)
                        oh, ol = (_Out(m, n, ldo, o_off, F16), _Out(m, n, ldo, o_off, F16)) if planes else (None, None)
                        xo = _Out(m, n, ldo, o_off, F32) if fp32 else None
                        sk = None
                        if use_s:
                            sk = _Out(m, n, ldo, o_off, F32)
                            sk.view.copy_(skd)
                        rc = _f16x3_call(L, ahd, ald, m, k, lda, whd, wld, n, ldw, csd if use_cs else None, alpha, bd if use_b else None,
                                         sk.view if sk else None, relu, oh.view if planes else None, ol.view if planes else None,
                                         xo.view if fp32 else None, ldo, ovf)
                        assert rc == 0, (what, L.lib().dca_last_error())
                        wx, whi, wlo = wants[name]
                        if fp32:
                            xo.check(what)
                            assert torch.equal(xo.bits(), wx), what
                        if planes:
                            oh.check(what)
                            ol.check(what)
                            assert torch.equal(oh.bits(), whi) and torch.equal(ol.bits(), wlo), what
                assert int(ovf[0]) == 0, ("overflow flag raised", m, n, k, lname, variant)
    finally:
        L.f16x3_gemm_variant(3)


@pytest.mark.parametrize("mode", [3, 4, 6, 7])
@torch.no_grad()
def test_f16x3_compiled_tails_beside_the_general_tail(mode):
    """relu(. * col_scale + bias (+ skip)) with (bit 0 skip, bit 1 fp32 output, bit 2 planes) = mode: interior tiles take the tail
    compiled for the mode, the right and bottom strips of the same call the general one.  Beside it the same call without ReLU —
    general tail everywhere — with the ReLU applied on the host: both bit-equal to each other and to the host value."""
    L = _L()
    use_s, fp32, planes = bool(mode & 1), bool(mode & 2), bool(mode & 4)
    try:
        for m, n in TAIL_SHAPES:
            k = 64
            ah, al, wh, wl, cs, bias, skip, prod = _f16x3_problem(m, n, k, 77 * m + n + mode)
            wx, whi, wlo = _f16x3_want(prod, cs, 0.5, bias, skip if use_s else None, True)
            nx, nhi, nlo = _f16x3_want(prod, cs, 0.5, bias, skip if use_s else None, False)
            pos = nx.view(F32) > 0
            lda, ldw, ldo = k + 8, k + 16, _r4(n) + 4
            ahd, ald, whd, wld = _padded(ah.half(), lda), _padded(al.half(), lda), _padded(wh.half(), ldw), _padded(wl.half(), ldw)
            csd, bd = _vec(cs.float()), _vec(bias.float())
            ovf = torch.zeros(4, dtype=torch.int32, device="cuda")
            for variant in (2, 3):
                L.f16x3_gemm_variant(variant)
                got = {}
                for relu in (True, False):
                    what = (mode, m, n, variant, relu)
                    oh, ol = (_Out(m, n, ldo, 0, F16), _Out(m, n, ldo, 0, F16)) if planes else (None, None)
                    xo = _Out(m, n, ldo, 0, F32) if fp32 else None
                    sk = None
                    if use_s:
                        sk = _Out(m, n, ldo, 0, F32)
                        sk.view.copy_(skip.float().cuda())
                    rc = _f16x3_call(L, ahd, ald, m, k, lda, whd, wld, n, ldw, csd, 0.5, bd, sk.view if sk else None, relu,
                                     oh.view if planes else None, ol.view if planes else None, xo.view if fp32 else None, ldo, ovf)
                    assert rc == 0, what
                    for o in (oh, ol, xo):
                        if o is not None:
                            o.check(what)
                    got[relu] = (xo.bits().clone() if fp32 else None, oh.bits().clone() if planes else None, ol.bits().clone() if planes else None)
                    ex = (wx, whi, wlo) if relu else (nx, nhi, nlo)
                    for gt, e in zip(got[relu], ex):
                        assert gt is None or torch.equal(gt, e), what
                for gr, gn in zip(got[True], got[False]):  # the two tails, the ReLU of the second applied here
                    if gr is not None:
                        assert torch.equal(gr, torch.where(pos, gn, torch.zeros_like(gn))), (mode, m, n, variant)
                assert int(ovf[0]) == 0
    finally:
        L.f16x3_gemm_variant(3)


# ---------------------------------------------------------------------------------------------------------------- dca_gemm16
def _gemm16_call(L, a, m, k, lda, w, n, ldw, dt, bias, skip, relu, out, ldo):
    return L.lib().dca_gemm16(_p(a), i64(m), int(k), i64(lda), _p(w), int(n), i64(ldw), DT_CODE[dt], _p(bias), _p(skip), int(relu),
                              _p(out), i64(ldo), L.stream_ptr())


def _want16(prod, bias, skip, relu, dt):
    v = prod + (bias if bias is not None else 0.0) + (skip if skip is not None else 0.0)
    _exact(v)
    return _bits((v.relu() if relu else v).float().to(dt)).cuda()


# (name, bias, skip, relu, out == skip)
FORMS16 = [("plain", False, False, False, False), ("bias_relu", True, False, True, False), ("bias_skip_relu", True, True, True, False),
           ("skip_no_bias", False, True, True, False), ("no_relu", True, True, False, False), ("inplace_residual", True, True, True, True),
           ("inplace_no_bias", False, True, True, True)]


@pytest.mark.parametrize("dt", [BF16, F16], ids=["bf16", "f16"])
@pytest.mark.parametrize("m,n,k", SHAPES16)
@torch.no_grad()
def test_gemm16_exact_at_ragged_shapes_strides_and_windows(m, n, k, dt):
    """Every form (the in-place residual out == skip included) x three layouts x schedule variants 1, 2 and 3, bit for bit
    against the host.  The window layout puts out / skip 8 bytes into their rows: legal, and not the lean tail's to take."""
    L = _L()
    a, w, bias, skip = _int_problem(m, n, k, 1000 * m + 10 * n + k)
    prod = _mm(a, w)
    _exact(_mm(a.abs(), w.abs()))
    wants = {name: _want16(prod, bias if use_b else None, skip if use_s else None, relu, dt) for name, use_b, use_s, relu, _ in FORMS16}
    bd, skd = _vec(bias.float()), skip.to(dt).cuda()
    try:
        for lname, a_pad, a_off, w_pad, o_pad, o_off in LAYOUTS16:
            lda, ldw, ldo = k + a_pad, k + w_pad, _r4(n) + o_pad
            ad, wd = _padded(a.to(dt), lda, a_off), _padded(w.to(dt), ldw)
            assert ad.data_ptr() % 16 == 0
            for variant in (1, 2, 3):
                L.gemm16_variant(variant)
                for name, use_b, use_s, relu, inplace in FORMS16:
                    what = (m, n, k, dt, lname, variant, name)
                    out = _Out(m, n, ldo, o_off, dt)
                    assert out.view.data_ptr() % 16 == (8 if o_off else 0)
                    sk = None
                    if use_s and inplace:
                        out.view.copy_(skd)
                        sk = out
                    elif use_s:
                        sk = _Out(m, n, ldo, o_off, dt)
                        sk.view.copy_(skd)
                    rc = _gemm16_call(L, ad, m, k, lda, wd, n, ldw, dt, bd if use_b else None, sk.view if sk else None, relu, out.view, ldo)
                    assert rc == 0, (what, L.lib().dca_last_error())
                    out.check(what)
                    assert torch.equal(out.bits(), wants[name]), what
    finally:
        L.gemm16_variant(3)


@pytest.mark.parametrize("use_b", [False, True], ids=["nobias", "bias"])
@pytest.mark.parametrize("use_s", [False, True], ids=["noskip", "skip"])
@pytest.mark.parametrize("dt", [BF16, F16], ids=["bf16", "f16"])
@torch.no_grad()
def test_gemm16_lean_kernels_beside_the_general_tail(dt, use_s, use_b):
    """Variant 3's eight lean kernels (type x skip x bias, ReLU) on the interior tiles of one call whose right and bottom strips
    the launcher re-launches on the general kernel with w, bias, skip and out offset by hand; beside it the same call under
    variant 2 (general tail everywhere), and under variant 3 with out / skip 8 bytes into their rows (no lean tail): bit-equal
    to each other and to the host, with the skip in its own buffer and in the output's."""
    L = _L()
    try:
        for m, n in TAIL_SHAPES:
            k = 64
            a, w, bias, skip = _int_problem(m, n, k, 31 * m + n)
            want = _want16(_mm(a, w), bias if use_b else None, skip if use_s else None, True, dt)
            ad, wd, bd, skd = _padded(a.to(dt), k + 8), _padded(w.to(dt), k + 16), _vec(bias.float()), skip.to(dt).cuda()
            for inplace in ((False, True) if use_s else (False,)):
                got = []
                ldo = (n + 7) // 8 * 8 + 8  # (a multiple of 8: what the lean tail wants of the stride)
                for variant, off in ((3, 0), (2, 0), (3, 4)):
                    L.gemm16_variant(variant)
                    what = (dt, use_s, use_b, m, n, inplace, variant, off)
                    out = _Out(m, n, ldo, off, dt)
                    sk = None
                    if use_s and inplace:
                        out.view.copy_(skd)
                        sk = out
                    elif use_s:
                        sk = _Out(m, n, ldo, off, dt)
                        sk.view.copy_(skd)
                    rc = _gemm16_call(L, ad, m, k, k + 8, wd, n, k + 16, dt, bd if use_b else None, sk.view if sk else None, True, out.view, ldo)
                    assert rc == 0, what
                    out.check(what)
                    assert torch.equal(out.bits(), want), what
                    got.append(out.bits().clone())
                assert torch.equal(got[0], got[1]) and torch.equal(got[0], got[2])
    finally:
        L.gemm16_variant(3)


# ------------------------------------------------------------------------------------------------- dca_gemm8, dca_gemm8_mx
# (name, lda - k, column offset of a, ldw - k, ldo16 - r4(n), offset of out16 / skip, ldo8 - r4(n), offset of out8,
#  ld_asc - k / 64, offset of a_scale, ld_osc - n / 64, offset of out8_scale)
LAYOUTS8 = [("contiguous", 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0), ("strided", 16, 0, 32, 4, 0, 8, 0, 4, 0, 3, 0),
            ("window", 32, 16, 32, 8, 4, 16, 8, 8, 4, 3, 1)]
SHAPES8 = [(1, 1, 128), (31, 3, 256), (33, 5, 384), (127, 63, 128), (129, 65, 256), (255, 255, 384), (256, 256, 128), (257, 257, 256),
           (513, 515, 128), (257, 260, 128), (2049, 257, 128), (1, 4, 256), (513, 260, 384)]
# out8 + block scales want n % 64 == 0: those shapes run with and without them, the ragged n with out16 alone
SHAPES8_MX = [(1, 64, 256), (31, 1, 256), (33, 192, 512), (127, 3, 512), (129, 320, 768), (255, 63, 768), (256, 256, 256), (257, 257, 256),
              (513, 515, 256), (257, 260, 256), (2049, 257, 256), (255, 5, 512), (129, 65, 256), (513, 320, 768), (33, 4, 256),
              (256, 255, 512)]
OUT8_SCALE = 4.0  # |v| reaches 163: v * 4 crosses 448, so the saturation is in play
FORMS8 = FORMS16
OUTS8 = [("out16", True, False), ("out8", False, True), ("both", True, True)]


def _gemm8_call(L, a, m, k, lda, w, n, ldw, scale, bias, skip, relu, out16, ldo16, out8, ldo8, out8_scale):
    return L.lib().dca_gemm8(_p(a), i64(m), int(k), i64(lda), _p(w), int(n), i64(ldw), _p(scale), _p(bias), _p(skip), int(relu),
                             _p(out16), i64(ldo16), _p(out8), i64(ldo8), C.c_double(out8_scale), L.stream_ptr())


def _mx_call(L, a, asc, m, k, lda, ld_asc, w, n, ldw, wsc, bias, skip, relu, out16, ldo16, out8, ldo8, osc, ld_osc):
    return L.lib().dca_gemm8_mx(_p(a), _p(asc), i64(m), int(k), i64(lda), i64(ld_asc), _p(w), int(n), i64(ldw), _p(wsc), _p(bias),
                                _p(skip), int(relu), _p(out16), i64(ldo16), _p(out8), i64(ldo8), _p(osc), i64(ld_osc), L.stream_ptr())


def _scale_vec(n):
    return torch.pow(torch.tensor(2.0, dtype=torch.float64), -(torch.arange(n) % 3).double())  # 1, 1/2, 1/4 by column


def _value8(prod, scale, bias, skip, relu):
    v = prod * scale
    _exact(v, 2.0 ** -3)
    v = v + (bias if bias is not None else 0.0) + (skip if skip is not None else 0.0)
    _exact(v, 2.0 ** -3)
    return v.relu() if relu else v


def _want8(prod, scale, bias, skip, relu):
    """(bf16 bits, e4m3 bytes at OUT8_SCALE) of the host's float64 value, on the device."""
    v = _value8(prod, scale, bias, skip, relu)
    return _bits(v.float().to(BF16)).cuda(), _q(v * OUT8_SCALE).cuda()


def _want8_mx(prod, scale, bias, skip, relu, blocks):
    """(bf16 bits, e4m3 bytes, E8M0 bytes): e = ceil(log2(amax / 448)) per row and 64 columns, clamped; bytes = e4m3(v / 2^e)."""
    v = _value8(prod, scale, bias, skip, relu)
    w16 = _bits(v.float().to(BF16)).cuda()
    if not blocks:
        return w16, None, None
    m, n = v.shape
    am = v.abs().view(m, n // 64, 64).amax(dim=2)
    e = torch.ceil(torch.log2((am / 448.0).clamp_min(2.0 ** -126))).clamp(-126, 126)
    f = torch.pow(torch.tensor(2.0, dtype=torch.float64), e).repeat_interleave(64, dim=1)
    return w16, _q(v / f).cuda(), (e + 127.0).to(U8).cuda()


def _fp8_problem(m, n, k, seed, mx):
    """a, w as e4m3 bytes of small integers (exact); mx: E8M0 bytes in {126, 127, 128} that differ between rows and between
    the two 64-deep halves of every K-tile.  -> (a bytes, a_scale bytes or None, w bytes, scale, bias, skip, a . w^T)."""
    a, w, bias, skip = _int_problem(m, n, k, seed)
    asc, av = None, a
    if mx:
        r, j = torch.arange(m).view(m, 1), torch.arange(k // 64).view(1, k // 64)
        asc = (126 + (r + j) % 3).to(U8)
        av = a * torch.pow(torch.tensor(2.0, dtype=torch.float64), asc.double() - 127.0).repeat_interleave(64, dim=1)
    _exact(_mm(av.abs(), w.abs()), 0.5)
    return _q(a), asc, _q(w), _scale_vec(n), bias, skip, _mm(av, w)


def _run_fp8(L, mx, m, n, k, layouts, forms, outs, seed):
    """One shape of dca_gemm8 / dca_gemm8_mx through `layouts` x `forms` x `outs`, bit for bit against the host."""
    a8, asc, w8, scale, bias, skip, prod = _fp8_problem(m, n, k, seed, mx)
    wants = {}
    for name, use_b, use_s, relu, _ in forms:
        args = (prod, scale, bias if use_b else None, skip if use_s else None, relu)
        wants[name] = _want8_mx(*args, n % 64 == 0) if mx else _want8(*args)
    sd, bd, skd = _vec(scale.float()), _vec(bias.float()), skip.to(BF16).cuda()
    for lname, a_pad, a_off, w_pad, p16, o16, p8, o8, pasc, oasc, posc, oosc in layouts:
        lda, ldw, ldo16, ldo8 = k + a_pad, k + w_pad, _r4(n) + p16, _r4(n) + p8
        ld_asc, ld_osc = k // 64 + pasc, n // 64 + posc
        ad, wd = _padded(a8, lda, a_off), _padded(w8, ldw)
        ascd = _padded(asc, ld_asc, oasc, 0xFF) if mx else None
        assert ad.data_ptr() % 16 == 0 and (not mx or ascd.data_ptr() % 4 == 0)
        for name, use_b, use_s, relu, inplace in forms:
            for oname, has16, has8 in outs:
                if (inplace and not has16) or (mx and has8 and n % 64 != 0):
                    continue
                what = ("mx" if mx else "gemm8", m, n, k, lname, name, oname)
                out16 = _Out(m, n, ldo16, o16, BF16) if has16 else None
                out8 = _Out(m, n, ldo8, o8, U8) if has8 else None
                osc = _Out(m, n // 64, ld_osc, oosc, U8, 0xA5) if (mx and has8) else None
                sk = None
                if use_s and inplace:
                    out16.view.copy_(skd)
                    sk = out16
                elif use_s:
                    sk = _Out(m, n, ldo16, o16, BF16)
                    sk.view.copy_(skd)
                if mx:
                    rc = _mx_call(L, ad, ascd, m, k, lda, ld_asc, wd, n, ldw, sd, bd if use_b else None, sk.view if sk else None, relu,
                                  out16.view if has16 else None, ldo16, out8.view if has8 else None, ldo8, osc.view if has8 else None, ld_osc)
                else:
                    rc = _gemm8_call(L, ad, m, k, lda, wd, n, ldw, sd, bd if use_b else None, sk.view if sk else None, relu,
                                     out16.view if has16 else None, ldo16, out8.view if has8 else None, ldo8, OUT8_SCALE)
                assert rc == 0, (what, L.lib().dca_last_error())
                if has16:
                    out16.check(what)
                    assert torch.equal(out16.bits(), wants[name][0]), what
                if has8:
                    out8.check(what)
                    assert torch.equal(out8.view, wants[name][1]), what
                if osc is not None:
                    osc.check(what)
                    assert torch.equal(osc.view, wants[name][2]), what


@torch.no_grad()
def test_fp8_integer_sums_are_exact_in_a_round_interior_tile():
    """The premise of the fp8 cases below, on tiles with no edge in them (256 x 256; dca_gemm8 at k = 128 and 256, dca_gemm8_mx
    at k = 256 and 512): the e4m3 MFMA, plain and block-scaled, sums these small integers exactly — bit equality with the host."""
    L = _L()
    for mx, k in ((False, 128), (False, 256), (True, 256), (True, 512)):
        _run_fp8(L, mx, 256, 256, k, LAYOUTS8[:1], [FORMS8[0], FORMS8[2]], OUTS8[2:], 8000 + k)


@pytest.mark.parametrize("m,n,k", SHAPES8)
@torch.no_grad()
def test_gemm8_exact_at_ragged_shapes_strides_and_windows(m, n, k):
    """Every form x (out16, out8, both) x three layouts: the bf16 result and the e4m3 bytes e4m3(sat(v * 4)) bit for bit."""
    _run_fp8(_L(), False, m, n, k, LAYOUTS8, FORMS8, OUTS8, 1000 * m + 10 * n + k)


@pytest.mark.parametrize("m,n,k", SHAPES8_MX)
@torch.no_grad()
def test_gemm8_mx_exact_at_ragged_shapes_strides_and_windows(m, n, k):
    """Block-scaled operand (scale bytes 126 / 127 / 128 by row and 64-deep half) x every form x three layouts; where
    n % 64 == 0 also the e4m3 blocks and their E8M0 bytes as the host model quantises the exact value block by block."""
    _run_fp8(_L(), True, m, n, k, LAYOUTS8, FORMS8, OUTS8, 1000 * m + 10 * n + k)


@pytest.mark.parametrize("kind,mode", [("gemm8", 3), ("gemm8", 7), ("gemm8", 11), ("gemm8", 12), ("gemm8", 14), ("gemm8", 15), ("mx", 3), ("mx", 11)])
@torch.no_grad()
def test_gemm8_compiled_tails_beside_the_general_tail(kind, mode):
    """(bit 0 skip, bit 1 bf16 output, bit 2 e4m3 output, bit 3 bias) = mode, with ReLU: interior tiles take the tail compiled for
    the mode (dca_gemm8_mx reaches 3 and 11 when it writes no blocks), the strips of the same call the general one.  Beside it
    the same call without ReLU — general tail everywhere — with the ReLU applied on the host: bit-equal."""
    L = _L()
    mx = kind == "mx"
    use_s, has16, has8, use_b = bool(mode & 1), bool(mode & 2), bool(mode & 4), bool(mode & 8)
    for m, n in TAIL_SHAPES:
        k = 256 if mx else 128
        a8, asc, w8, scale, bias, skip, prod = _fp8_problem(m, n, k, 13 * m + n + mode, mx)
        args = (prod, scale, bias if use_b else None, skip if use_s else None)
        lda, ldw, ldo16, ldo8, ld_asc = k + 16, k + 32, _r4(n) + 4, _r4(n) + 8, k // 64 + 4
        ad, wd, sd, bd = _padded(a8, lda), _padded(w8, ldw), _vec(scale.float()), _vec(bias.float())
        ascd = _padded(asc, ld_asc, 0, 0xFF) if mx else None
        got = {}
        for relu in (True, False):
            what = (kind, mode, m, n, relu)
            w16, w8b = _want8(*args, relu)
            out16 = _Out(m, n, ldo16, 0, BF16) if has16 else None
            out8 = _Out(m, n, ldo8, 0, U8) if has8 else None
            sk = None
            if use_s:
                sk = _Out(m, n, ldo16, 0, BF16)
                sk.view.copy_(skip.to(BF16).cuda())
            if mx:
                rc = _mx_call(L, ad, ascd, m, k, lda, ld_asc, wd, n, ldw, sd, bd if use_b else None, sk.view if sk else None, relu,
                              out16.view, ldo16, None, 0, None, 0)
            else:
                rc = _gemm8_call(L, ad, m, k, lda, wd, n, ldw, sd, bd if use_b else None, sk.view if sk else None, relu,
                                 out16.view if has16 else None, ldo16, out8.view if has8 else None, ldo8, OUT8_SCALE)
            assert rc == 0, what
            if has16:
                out16.check(what)
                assert torch.equal(out16.bits(), w16), what
            if has8:
                out8.check(what)
                assert torch.equal(out8.view, w8b), what
            got[relu] = (out16.bits().clone() if has16 else None, out8.view.clone() if has8 else None)
        if has16:  # sign bit clear and not zero <=> v > 0
            g = got[False][0]
            assert torch.equal(got[True][0], torch.where(g > 0, g, torch.zeros_like(g))), (kind, mode, m, n)
        if has8:
            g = got[False][1]
            assert torch.equal(got[True][1], torch.where(g < 0x80, g, torch.zeros_like(g))), (kind, mode, m, n)


# ---------------------------------------------------------------------------------------------------------- small converters
@pytest.mark.parametrize("m", [1, 257])
@pytest.mark.parametrize("n", [4, 8, 260])
@torch.no_grad()
def test_split_planes_and_quant_e4m3_with_strides_and_guards(m, n):
    """dca_split_planes, and dca_quant_e4m3 on fp32 and bf16 input, with ld > n and ldo > n: conversions are exactly defined,
    so bit for bit against the host's; the input's padding is NaN (a padding element converted would land as NaN in range or
    raise the flag), the outputs' padding keeps its fill."""
    L = _L()
    lib = L.lib()
    g = torch.Generator().manual_seed(100 * m + n)
    x = torch.randn((m, n), generator=g) * 100.0
    x[0, :4] = torch.tensor([0.0, -0.0, 448.0, -1000.0])
    for ld, ldo, off in ((n, n, 0), (n + 4, n + 8, 0), (n + 8, n + 8, 4)):
        what = (m, n, ld, ldo, off)
        xd = _padded(x, ld, off)
        oh, ol = _Out(m, n, ldo, off, F16), _Out(m, n, ldo, off, F16)
        ovf = torch.zeros(4, dtype=torch.int32, device="cuda")
        assert lib.dca_split_planes(_p(xd), i64(m), i64(n), i64(ld), _p(oh.view), _p(ol.view), i64(ldo), _p(ovf), L.stream_ptr()) == 0, what
        oh.check(what)
        ol.check(what)
        hi = x.half()
        assert torch.equal(oh.bits(), _bits(hi).cuda()) and torch.equal(ol.bits(), _bits((x - hi.float()).half()).cuda()), what
        assert int(ovf[0]) == 0, what
        for dt in (F32, BF16):
            xs = x.to(dt)
            o8 = _Out(m, n, ldo, off, U8)
            rc = lib.dca_quant_e4m3(_p(_padded(xs, ld, off)), DT_CODE[dt], i64(m), i64(n), i64(ld), C.c_double(0.75), _p(o8.view), i64(ldo),
                                    L.stream_ptr())
            assert rc == 0, (what, dt)
            o8.check((what, dt))
            assert torch.equal(o8.view, _q(xs.float() * 0.75).cuda()), (what, dt)  # (one fp32 product, as on the device)


# ------------------------------------------------------------------------------------------------------------------ refusals
# Each entry point's cases are built by a function of (library, stream, device) that returns (bad calls, outputs with their fill,
# good calls): every DCA_ARG clause of the launcher gets a call that breaks that clause alone, on buffers large enough that the
# call would stay inside them were it accepted.
def _full(shape, value, dtype, dev):
    return torch.full(shape, value, dtype=dtype, device=dev)


def _f16x3_refusals(lib, st, dev):
    ah, al, wh, wl = (_full((32, 256), 1.0, F16, dev) for _ in range(4))
    cs, bias = _full((64,), 1.0, F32, dev), _full((64,), 1.0, F32, dev)
    skip = _full((32, 16), 1.0, F32, dev)
    oh, ol, xo = _poison(32, 16, F16, dev=dev), _poison(32, 16, F16, dev=dev), _poison(32, 16, F32, dev=dev)
    ovf = torch.zeros(4, dtype=torch.int32, device=dev)

    def call(ah=(ah, 0), al=(al, 0), m=8, k=64, lda=72, wh=(wh, 0), wl=(wl, 0), n=8, ldw=72, skip=(None, 0), oh=(oh, 0), ol=(ol, 0),
             xo=(xo, 0), ldo=16):
        return lib.dca_f16x3_gemm(_p(*ah), _p(*al), i64(m), k, i64(lda), _p(*wh), _p(*wl), n, i64(ldw), _p(cs), C.c_double(1.0), _p(bias),
                                  _p(*skip), 1, _p(*oh), _p(*ol), _p(*xo), i64(ldo), _p(ovf), st)

    N = (None, 0)
    bad = [("null a_h", lambda: call(ah=N)), ("null a_l", lambda: call(al=N)), ("null w_h", lambda: call(wh=N)), ("null w_l", lambda: call(wl=N)),
           ("m < 0", lambda: call(m=-1)), ("n = 0", lambda: call(n=0)), ("k = 0", lambda: call(k=0)), ("k = 32", lambda: call(k=32)),
           ("k = 96", lambda: call(k=96, lda=128, ldw=128)),
           ("lda < k", lambda: call(lda=56)), ("ldw < k", lambda: call(ldw=56)), ("lda % 8", lambda: call(lda=68)), ("ldw % 8", lambda: call(ldw=68)),
           ("ldo < n", lambda: call(ldo=4)),
           ("out_h without out_l", lambda: call(ol=N)), ("out_l without out_h", lambda: call(oh=N)), ("no output", lambda: call(oh=N, ol=N, xo=N)),
           ("misaligned a_h", lambda: call(ah=(ah, 8))), ("misaligned a_l", lambda: call(al=(al, 8))),
           ("misaligned w_h", lambda: call(wh=(wh, 8))), ("misaligned w_l", lambda: call(wl=(wl, 8))),
           ("ldo % 4", lambda: call(ldo=18)), ("misaligned out_h", lambda: call(oh=(oh, 4))), ("misaligned out_l", lambda: call(ol=(ol, 4))),
           ("misaligned x_out", lambda: call(xo=(xo, 8))), ("misaligned skip", lambda: call(skip=(skip, 8)))]
    good = [lambda: call(), lambda: call(skip=(skip, 0))]
    return "dca_f16x3_gemm", bad, [(oh, 8), (ol, 8), (xo, 8)], good, lambda: call(m=0)


def _gemm16_refusals(lib, st, dev):
    a, w = _full((32, 256), 1.0, BF16, dev), _full((32, 256), 1.0, BF16, dev)
    bias, skip, out = _full((64,), 1.0, F32, dev), _full((32, 16), 1.0, BF16, dev), _poison(32, 16, BF16, dev=dev)

    def call(a=(a, 0), m=8, k=64, lda=72, w=(w, 0), n=8, ldw=72, dtype=2, skip=(None, 0), out=(out, 0), ldo=16):
        return lib.dca_gemm16(_p(*a), i64(m), k, i64(lda), _p(*w), n, i64(ldw), dtype, _p(bias), _p(*skip), 1, _p(*out), i64(ldo), st)

    N = (None, 0)
    bad = [("null a", lambda: call(a=N)), ("null w", lambda: call(w=N)), ("null out", lambda: call(out=N)), ("m < 0", lambda: call(m=-1)),
           ("n = 0", lambda: call(n=0)), ("k = 0", lambda: call(k=0)), ("k = 32", lambda: call(k=32)), ("k = 96", lambda: call(k=96, lda=128, ldw=128)),
           ("dtype fp32", lambda: call(dtype=0)), ("dtype 4", lambda: call(dtype=4)),
           ("lda < k", lambda: call(lda=56)), ("ldw < k", lambda: call(ldw=56)), ("lda % 8", lambda: call(lda=68)), ("ldw % 8", lambda: call(ldw=68)),
           ("ldo < n", lambda: call(ldo=4)), ("ldo % 4", lambda: call(ldo=18)),
           ("misaligned a", lambda: call(a=(a, 8))), ("misaligned w", lambda: call(w=(w, 8))),
           ("misaligned out", lambda: call(out=(out, 4))), ("misaligned skip", lambda: call(skip=(skip, 4))),
           ("out == a", lambda: call(out=(a, 0))), ("out inside a", lambda: call(out=(a, 64))),
           ("out ends inside a", lambda: call(a=(a, 1024), out=(a, 0), ldo=256))]
    good = [lambda: call(), lambda: call(skip=(skip, 0))]
    return "dca_gemm16", bad, [(out, 8)], good, lambda: call(m=0)


def _gemm8_refusals(lib, st, dev):
    a, w = _full((32, 512), 0x38, U8, dev), _full((32, 512), 0x38, U8, dev)  # 0x38 = 1.0 in e4m3
    scale, bias = _full((64,), 1.0, F32, dev), _full((64,), 1.0, F32, dev)
    skip, out16, out8 = _full((32, 16), 1.0, BF16, dev), _poison(32, 16, BF16, dev=dev), _poison(32, 16, U8, dev=dev)

    def call(a=(a, 0), m=8, k=128, lda=144, w=(w, 0), n=8, ldw=144, scale=(scale, 0), skip=(None, 0), out16=(out16, 0), ldo16=16,
             out8=(out8, 0), ldo8=16, out8_scale=1.0):
        return lib.dca_gemm8(_p(*a), i64(m), k, i64(lda), _p(*w), n, i64(ldw), _p(*scale), _p(bias), _p(*skip), 1, _p(*out16), i64(ldo16),
                             _p(*out8), i64(ldo8), C.c_double(out8_scale), st)

    N = (None, 0)
    bad = [("null a", lambda: call(a=N)), ("null w", lambda: call(w=N)), ("null scale", lambda: call(scale=N)),
           ("no output", lambda: call(out16=N, out8=N)), ("m < 0", lambda: call(m=-1)), ("n = 0", lambda: call(n=0)),
           ("k = 0", lambda: call(k=0)), ("k = 64", lambda: call(k=64)), ("k = 192", lambda: call(k=192, lda=256, ldw=256)),
           ("lda < k", lambda: call(lda=112)), ("ldw < k", lambda: call(ldw=112)), ("lda % 16", lambda: call(lda=136)), ("ldw % 16", lambda: call(ldw=136)),
           ("misaligned a", lambda: call(a=(a, 8))), ("misaligned w", lambda: call(w=(w, 8))),
           ("ldo16 < n", lambda: call(ldo16=4)), ("ldo16 % 4", lambda: call(ldo16=18)), ("misaligned out16", lambda: call(out16=(out16, 4))),
           ("misaligned skip", lambda: call(skip=(skip, 4))), ("skip alone, ldo16 < n", lambda: call(out16=N, skip=(skip, 0), ldo16=4)),
           ("ldo8 < n", lambda: call(ldo8=4)), ("ldo8 % 4", lambda: call(ldo8=18)), ("misaligned out8", lambda: call(out8=(out8, 2))),
           ("out8_scale = 0", lambda: call(out8_scale=0.0)), ("out8_scale < 0", lambda: call(out8_scale=-1.0)),
           ("out8 inside a", lambda: call(out8=(a, 64))), ("out16 inside a", lambda: call(out16=(a, 64))), ("out8 == a", lambda: call(out8=(a, 0)))]
    good = [lambda: call(), lambda: call(skip=(skip, 0)), lambda: call(out8=N), lambda: call(out16=N)]
    return "dca_gemm8", bad, [(out16, 8), (out8, 8)], good, lambda: call(m=0)


def _gemm8_mx_refusals(lib, st, dev):
    a, w = _full((16, 8704), 0x38, U8, dev), _full((80, 8704), 0x38, U8, dev)
    asc = _full((16, 256), 127, U8, dev)
    wsc, bias = _full((128,), 1.0, F32, dev), _full((128,), 1.0, F32, dev)
    skip, out16, out8 = _full((16, 72), 1.0, BF16, dev), _poison(16, 72, BF16, dev=dev), _poison(16, 72, U8, dev=dev)
    osc = _poison(16, 2, U8, 0xA5, dev=dev)

    def call(a=(a, 0), asc=(asc, 0), m=8, k=256, lda=272, ld_asc=8, w=(w, 0), n=64, ldw=272, wsc=(wsc, 0), skip=(None, 0), out16=(out16, 0),
             ldo16=72, out8=(out8, 0), ldo8=72, osc=(osc, 0), ld_osc=2):
        return lib.dca_gemm8_mx(_p(*a), _p(*asc), i64(m), k, i64(lda), i64(ld_asc), _p(*w), n, i64(ldw), _p(*wsc), _p(bias), _p(*skip), 1,
                                _p(*out16), i64(ldo16), _p(*out8), i64(ldo8), _p(*osc), i64(ld_osc), st)

    N = (None, 0)
    bad = [("null a", lambda: call(a=N)), ("null a_scale", lambda: call(asc=N)), ("null w", lambda: call(w=N)), ("null w_scale", lambda: call(wsc=N)),
           ("no output", lambda: call(out16=N, out8=N, osc=N)), ("m < 0", lambda: call(m=-1)), ("n = 0", lambda: call(n=0, out8=N, osc=N)),
           ("k = 0", lambda: call(k=0)), ("k = 128", lambda: call(k=128)), ("k = 384", lambda: call(k=384, lda=512, ldw=512)),
           ("k = 8448", lambda: call(k=8448, lda=8704, ldw=8704, ld_asc=256)),
           ("lda < k", lambda: call(lda=240)), ("ldw < k", lambda: call(ldw=240)), ("lda % 16", lambda: call(lda=264)), ("ldw % 16", lambda: call(ldw=264)),
           ("ld_asc < k / 64", lambda: call(ld_asc=0)), ("ld_asc % 4", lambda: call(ld_asc=6)),
           ("misaligned a", lambda: call(a=(a, 8))), ("misaligned w", lambda: call(w=(w, 8))), ("misaligned a_scale", lambda: call(asc=(asc, 2))),
           ("ldo16 < n", lambda: call(ldo16=60)), ("ldo16 % 4", lambda: call(ldo16=74)), ("misaligned out16", lambda: call(out16=(out16, 4))),
           ("misaligned skip", lambda: call(skip=(skip, 4))),
           ("out8 without out8_scale", lambda: call(osc=N)), ("out8_scale without out8", lambda: call(out8=N)),
           ("ldo8 < n", lambda: call(ldo8=60)), ("ldo8 % 4", lambda: call(ldo8=74)), ("misaligned out8", lambda: call(out8=(out8, 2))),
           ("n % 64 with out8", lambda: call(n=32)), ("ld_osc < n / 64", lambda: call(ld_osc=0)),
           ("out8 inside a", lambda: call(out8=(a, 64))), ("out16 inside a", lambda: call(out16=(a, 64))),
           ("out8_scale == a_scale", lambda: call(osc=(asc, 0)))]
    good = [lambda: call(), lambda: call(skip=(skip, 0)), lambda: call(out8=N, osc=N), lambda: call(out16=N)]
    return "dca_gemm8_mx", bad, [(out16, 64), (out8, 64), (osc, 1)], good, lambda: call(m=0)


def _split_planes_refusals(lib, st, dev):
    x = _full((16, 32), 1.0, F32, dev)
    oh, ol = _poison(16, 16, F16, dev=dev), _poison(16, 16, F16, dev=dev)
    ovf = torch.zeros(4, dtype=torch.int32, device=dev)

    def call(x=(x, 0), m=8, n=8, ld=16, oh=(oh, 0), ol=(ol, 0), ldo=16):
        return lib.dca_split_planes(_p(*x), i64(m), i64(n), i64(ld), _p(*oh), _p(*ol), i64(ldo), _p(ovf), st)

    N = (None, 0)
    bad = [("null x", lambda: call(x=N)), ("null out_h", lambda: call(oh=N)), ("null out_l", lambda: call(ol=N)), ("m < 0", lambda: call(m=-1)),
           ("n = 0", lambda: call(n=0)), ("n = 6", lambda: call(n=6)), ("ld < n", lambda: call(ld=4)), ("ld % 4", lambda: call(ld=10)),
           ("ldo < n", lambda: call(ldo=4)), ("ldo % 4", lambda: call(ldo=10)),
           ("misaligned x", lambda: call(x=(x, 8))), ("misaligned out_h", lambda: call(oh=(oh, 4))), ("misaligned out_l", lambda: call(ol=(ol, 4)))]
    return "dca_split_planes", bad, [(oh, 8), (ol, 8)], [lambda: call()], lambda: call(m=0)


def _quant_e4m3_refusals(lib, st, dev):
    x32, x16 = _full((16, 32), 1.0, F32, dev), _full((16, 32), 1.0, BF16, dev)
    out = _poison(16, 16, U8, dev=dev)

    def call(x=(x32, 0), dtype=0, m=8, n=8, ld=16, scale=1.0, out=(out, 0), ldo=16):
        return lib.dca_quant_e4m3(_p(*x), dtype, i64(m), i64(n), i64(ld), C.c_double(scale), _p(*out), i64(ldo), st)

    N = (None, 0)
    bad = [("null x", lambda: call(x=N)), ("null out", lambda: call(out=N)), ("m < 0", lambda: call(m=-1)), ("n = 0", lambda: call(n=0)),
           ("n = 6", lambda: call(n=6)), ("ld < n", lambda: call(ld=4)), ("ld % 4", lambda: call(ld=10)), ("ldo < n", lambda: call(ldo=4)),
           ("ldo % 4", lambda: call(ldo=10)), ("scale = 0", lambda: call(scale=0.0)), ("scale < 0", lambda: call(scale=-1.0)),
           ("dtype fp16", lambda: call(dtype=1)), ("dtype 6", lambda: call(dtype=6)),
           ("misaligned fp32 x", lambda: call(x=(x32, 8))), ("misaligned bf16 x", lambda: call(x=(x16, 4), dtype=2)),
           ("misaligned out", lambda: call(out=(out, 2)))]
    return "dca_quant_e4m3", bad, [(out, 8)], [lambda: call(), lambda: call(x=(x16, 0), dtype=2)], lambda: call(m=0)


REFUSALS = [_f16x3_refusals, _gemm16_refusals, _gemm8_refusals, _gemm8_mx_refusals, _split_planes_refusals, _quant_e4m3_refusals]


def _untouched(outs):
    for o, _ in outs:
        b = _bits(o)
        assert bool((b == b[0, 0]).all()), "a refused call wrote to an output"


@pytest.mark.parametrize("cases", REFUSALS, ids=lambda f: f.__name__.strip("_"))
def test_bad_arguments_are_refused_before_anything_is_launched(cases):
    """Every DCA_ARG clause of the launcher, broken alone: DCA_E_BADARG, the error text says `bad argument` and names the entry
    point, and after a synchronize the sentinel-filled outputs are untouched; m == 0 returns 0 and writes nothing; the same
    harness with good arguments goes through and writes rows [0, 8) x its n columns, nothing else."""
    L_ = _L()
    L = L_.lib()
    fn, bad, outs, good, empty = cases(L, L_.stream_ptr(), "cuda")
    for what, call in bad:
        assert call() == BADARG, (fn, what)
        text = L.dca_last_error().decode()
        assert text.startswith("bad argument: ") and fn in text, (fn, what, text)
    assert empty() == 0, fn
    torch.cuda.synchronize()
    _untouched(outs)
    for call in good:
        assert call() == 0, (fn, L.dca_last_error().decode())
    torch.cuda.synchronize()
    for o, cols in outs:
        b = _bits(o)
        fill = b[-1, -1].clone()
        assert bool((b[:8, :cols] != fill).all()), fn
        b = b.clone()
        b[:8, :cols] = fill
        assert bool((b == fill).all()), fn
