"""GPU: every kernel behind ipa_conv2d_dev / ipa_sepconv2d_dev (csrc/conv.hip and the wave
kernels it routes to) on both sides of every selection threshold, against the plain float64
reference of tests/conv_ref.py.

Which kernel a case runs is asked of the library (ipa_conv_path, the launchers' own
arithmetic) and asserted before the case runs.  Frames are the smallest that still go wrong:
below the kernel radius, one 128 x 32 tile exactly and +- 1, across the 248 / 256 strip step of
the wave kernels, shorter than a 63-tap radius.  Data is signed (sums cancel), kernels are signed,
not normalised and hold an exact 0.0 tap; cval is 0.3.

Tolerance (derived, conv_ref.bound): |got - ref| <= (n + 2) u sum |k| |img| per pixel, n the
number of products, u = 2^-24 / 2^-53 - what any summation order in the image's precision keeps,
no margin added.  Bit identity is asked in one place: a call with pitches and frame strides
against the same call on contiguous copies.

The worst err / bound per path is printed by the last test of the module.
"""
import ctypes as C

import numpy as np
import pytest

from . import conv_ref as ref
from . import conv_cases as cc

pytestmark = pytest.mark.gpu

F32, F64 = np.float32, np.float64
WORST = {}          # path name -> worst err / bound seen
FILL = -5.0         # what the destination holds before a call
CONV_NAMES = {cc.WAVE: 'conv2d wave', cc.TILE: 'conv2d LDS tile', cc.GENERIC: 'conv2d generic'}
SEP_NAMES = {cc.SEP_WAVE: 'sepconv2d wave', cc.SEP_LDS: 'sepconv2d LDS',
             cc.SEP_LDS_BIG: 'sepconv2d LDS > 64 KiB', cc.SEP_TWO_GENERIC: 'sepconv2d 2 x generic',
             cc.SEP_ONE_GENERIC: 'sepconv2d 1 x generic'}


@pytest.fixture(scope='module')
def ctx():
    import imgprocessor_amd
    return imgprocessor_amd.default_context(0)


def note(name, dt, ratio):
    key = '%s %s' % (name, np.dtype(dt).name)
    WORST[key] = max(WORST.get(key, 0.0), ratio)
    return ratio


# ------------------------------------------------- the C ABI, directly ----
def _embed(a, pitch, pad_rows, guard):
    """(n, h, w) -> (n, h + pad_rows, pitch) with a in the top-left corner of every frame and
    +-guard, alternating, everywhere else"""
    n, h, w = a.shape
    big = np.empty((n, h + pad_rows, pitch), a.dtype)
    big[...] = guard
    if a.dtype.kind == 'f':
        big.reshape(-1)[1::2] = -guard
    big[:, :h, :w] = a
    return big


def _dp(v):
    v = np.ascontiguousarray(v, dtype=F64).ravel()
    return v, v.ctypes.data_as(C.POINTER(C.c_double))


def call(ctx, src, k, mode='reflect', mode_y=None, cval=cc.CVAL, mask=None, sp=None, dp=None,
         mp=None, pad_rows=0, status=False):
    """ipa_conv2d_dev (k a 2-D array) or ipa_sepconv2d_dev (k a pair (ky, kx)) on the frames
    src (n, h, w), with row pitches sp / dp / mp (elements; default: the width) and pad_rows
    rows between frames.  -> the whole destination buffer (n, h + pad_rows, dp), or the status"""
    from imgprocessor_amd import ops
    from imgprocessor_amd.device import dtype_id
    n, h, w = src.shape
    sp, dp, mp = sp or w, dp or w, mp or w
    bx, by = ops.border_id(mode), ops.border_id(mode_y if mode_y is not None else mode)
    d_src = ctx.to_device(_embed(src, sp, pad_rows, 1e30))
    d_dst = ctx.to_device(np.full((n, h + pad_rows, dp), FILL, src.dtype))
    dt = dtype_id(src.dtype)
    if isinstance(k, tuple):
        assert mask is None
        (ky, pky), (kx, pkx) = (_dp(t if t is not None else []) for t in k)
        rc = ctx._lib.ipa_sepconv2d_dev(ctx.handle, d_src.ptr, dt, h, w, sp, pky, ky.size, pkx,
                                        kx.size, d_dst.ptr, dp, n, (h + pad_rows) * sp,
                                        (h + pad_rows) * dp, by, bx, float(cval))
    else:
        kk, pk = _dp(k)
        d_m = None
        if mask is not None:
            d_m = ctx.to_device(_embed(mask[None], mp, 0, 1)[0])
        rc = ctx._lib.ipa_conv2d_dev(ctx.handle, d_src.ptr, dt, h, w, sp, pk, k.shape[0], k.shape[1],
                                     d_m.ptr if d_m is not None else None, mp, d_dst.ptr, dp, n,
                                     (h + pad_rows) * sp, (h + pad_rows) * dp, bx, by, float(cval))
    if status:
        return rc
    ctx._check(rc, 'conv')
    return d_dst.get()


def knobs_of(case):
    """the tuning a CONV_CASES entry runs under: big_wave = 0 where it asks for the tile kernel,
    rank1_sep = 0 for an unmasked float32 9x9 (the dense kernel, whatever the values)"""
    dt, kh, kw, flags = case[:4]
    kn = {}
    if flags & cc.BIG_WAVE_OFF:
        kn['big_wave'] = 0
    if dt is F32 and kh == kw == 9 and not flags & cc.MASKED:
        kn['rank1_sep'] = 0
    return kn


class tuned:
    def __init__(self, ctx, **knobs):
        self.ctx, self.knobs = ctx, knobs

    def __enter__(self):
        self.old = self.ctx.set_tuning(**self.knobs) if self.knobs else {}

    def __exit__(self, *exc):
        if self.old:
            self.ctx.set_tuning(**self.old)


def oracle_says(oracle, img, k, mode, mode_y, mask, want, bnd):
    """the second opinion, for the message of a failure"""
    try:
        if isinstance(k, tuple):
            if mode_y is not None:
                return 'oracle: takes one mode'
            o = oracle.sepconv2d(img, k[0], k[1], mode, cc.CVAL)
        else:
            o = oracle.conv2d(img, k, mode, cc.CVAL, mask, mode_y)
        return 'oracle at %.3g of the bound' % cc.compare(o, want, bnd, 'oracle')
    except AssertionError as e:
        return 'THE ORACLE FAILS TOO: %s' % e


def check(oracle, got, img, k, mode, mode_y, mask, what):
    want = ref.ref_conv2d(img, k, mode, cc.CVAL, mode_y, mask) if not isinstance(k, tuple) \
        else ref.ref_sepconv2d(img, k[0], k[1], mode, cc.CVAL, mode_y)
    bnd = ref.bound(img, k, mode, cc.CVAL, mode_y, mask)
    assert got.dtype == img.dtype, what
    try:
        return cc.compare(got, want, bnd, what)
    except AssertionError as e:
        raise AssertionError('%s [%s]' % (e, oracle_says(oracle, img, k, mode, mode_y, mask, want,
                                                          bnd)))


# ------------------------------------------------------------------ conv2d ----
@pytest.mark.parametrize('border', cc.BORDERS, ids=cc.border_id)
@pytest.mark.parametrize('case', cc.CONV_CASES, ids=cc.conv_id)
def test_conv2d(ctx, oracle, case, border):
    """1 - 4 of the list: float32 on the wave, on the tile kernel with a mask and with
    big_wave = 0; float64 on the tile kernel and, from 9x9, the generic one; the generic kernel's
    own shapes - 'reflect' on every frame, the other borders on the border frames"""
    dt, kh, kw, flags, want_path = case
    assert cc.path('conv2d', dt, kh, kw, flags) == want_path
    mode, mode_y = border
    worst = 0.0
    with tuned(ctx, **knobs_of(case)):
        before = ctx.get_tuning('rank1_routed')
        for shape in (cc.FRAMES if border == cc.BORDERS[0] else cc.BORDER_FRAMES):
            img, k, m = cc.conv_inputs(case, shape)
            got = call(ctx, img[None], k, mode, mode_y, mask=m)[0]
            worst = max(worst, check(oracle, got, img, k, mode, mode_y, m, '%s %s %s' % (
                cc.conv_id(case), shape, cc.border_id(border))))
        assert ctx.get_tuning('rank1_routed') == before
    print('%s %s: %.3f of the bound' % (cc.conv_id(case), cc.border_id(border),
                                        note(CONV_NAMES[want_path], dt, worst)))


@pytest.mark.parametrize('case', cc.CONV_GENERIC + cc.CONV_F32[::4] + cc.CONV_F64[1::3],
                         ids=cc.conv_id)
def test_conv2d_batch(ctx, oracle, case):
    """three different frames in one call: the generic kernel takes the frame from blockIdx.z,
    the others from blockIdx.y"""
    dt, kh, kw, flags, want_path = case
    assert cc.path('conv2d', dt, kh, kw, flags) == want_path
    shape = (33, 129)
    src = cc.batch(shape, dt)
    _, k, m = cc.conv_inputs(case, shape)
    with tuned(ctx, **knobs_of(case)):
        got = call(ctx, src, k, 'mirror', 'constant', mask=m)
    for i in range(3):
        note(CONV_NAMES[want_path], dt, check(oracle, got[i], src[i], k, 'mirror', 'constant', m,
                                              '%s frame %d' % (cc.conv_id(case), i)))


def test_conv2d_rank1_route(ctx, oracle):
    """a float32 9x9 outer product under the default knobs goes to the separable wave kernel
    (counter rank1_routed) and meets the dense reference; with a non-zero constant border the
    second pass would pad with cval instead of cval * sum(ky), so it stays dense"""
    k = cc.rank1_kernel(9)
    assert ctx.get_tuning('rank1_sep') & 2 and ctx.get_tuning('big_wave') != 0
    for shape in ((2, 3), (33, 129), (37, 261)):
        img = cc.frame(shape, F32)
        for mode, mode_y, routed in (('reflect', None, 1), ('wrap', 'nearest', 1),
                                     ('constant', None, 0), ('nearest', 'constant', 0)):
            before = ctx.get_tuning('rank1_routed')
            got = call(ctx, img[None], k, mode, mode_y)[0]
            assert ctx.get_tuning('rank1_routed') == before + routed, (shape, mode, mode_y)
            r = check(oracle, got, img, k, mode, mode_y, None, 'rank-1 9x9 %s %s/%s' % (
                shape, mode, mode_y))
            note('conv2d 9x9 rank-1 route' if routed else CONV_NAMES[cc.WAVE], F32, r)


# --------------------------------------------------------------- sepconv2d ----
@pytest.mark.parametrize('border', cc.BORDERS, ids=cc.border_id)
@pytest.mark.parametrize('case', cc.SEP_CASES, ids=cc.sep_id)
def test_sepconv2d(ctx, oracle, case, border):
    """5 - 6 of the list: the wave, the LDS kernel on both sides of the 64 KiB opt-in and of its
    end (63 | 65 taps, 150 KiB), one axis only on every path"""
    dt, nky, nkx, want_path = case
    assert cc.path('sepconv2d', dt, nky, nkx) == want_path
    mode, mode_y = border
    k = cc.sep_taps(nky, nkx)
    frames = cc.sep_frames(nky, nkx)
    if border != cc.BORDERS[0] and frames is cc.FRAMES:
        frames = cc.BORDER_FRAMES
    worst = 0.0
    for shape in frames:
        img = cc.frame(shape, dt)
        got = call(ctx, img[None], k, mode, mode_y)[0]
        worst = max(worst, check(oracle, got, img, k, mode, mode_y, None, '%s %s %s' % (
            cc.sep_id(case), shape, cc.border_id(border))))
    print('%s %s: %.3f of the bound' % (cc.sep_id(case), cc.border_id(border),
                                        note(SEP_NAMES[want_path], dt, worst)))


# ----------------------------------------------------- pitches and strides ----
PITCHED = (('conv', (F32, 5, 5, 0, cc.WAVE)), ('conv', (F32, 9, 9, 0, cc.WAVE)),
           ('conv', (F32, 7, 7, cc.MASKED, cc.TILE)), ('conv', (F64, 5, 5, cc.MASKED, cc.TILE)),
           ('conv', (F32, 6, 4, cc.MASKED, cc.GENERIC)), ('conv', (F64, 13, 13, 0, cc.GENERIC)),
           ('sep', (F32, 5, 5, cc.SEP_WAVE)), ('sep', (F32, 11, 11, cc.SEP_LDS)),
           ('sep', (F64, 9, 9, cc.SEP_LDS_BIG)), ('sep', (F32, 0, 5, cc.SEP_LDS)),
           ('sep', (F32, 65, 65, cc.SEP_TWO_GENERIC)), ('sep', (F32, 65, 0, cc.SEP_ONE_GENERIC)))


@pytest.mark.parametrize('odd', [0, 1], ids=['aligned', 'odd'])
@pytest.mark.parametrize('op,case', PITCHED,
                         ids=[o + '-' + (cc.conv_id(c) if o == 'conv' else cc.sep_id(c))
                              for o, c in PITCHED])
def test_pitches_and_strides(ctx, oracle, op, case, odd):
    """a batch of 3 inside larger buffers: 16-byte aligned pitches (the vector loads and stores)
    and odd ones (the element-wise branches), a frame stride larger than a frame, the mask with
    a pitch of its own.  The padding of the source holds +-1e30 and must never be read; that of
    the destination must come back untouched; the frames must be the bits of the same call on
    contiguous copies, and within the bound of the reference."""
    dt = case[0]
    shape = (37, 261)
    h, w = shape
    src = cc.batch(shape, dt)
    m = None
    if op == 'conv':
        assert cc.path('conv2d', *case[:4]) == case[4]
        _, k, m = cc.conv_inputs(case, shape)
        kn = knobs_of(case)
        name = CONV_NAMES[case[4]]
    else:
        assert cc.path('sepconv2d', *case[:3]) == case[3]
        k, kn, name = cc.sep_taps(case[1], case[2]), {}, SEP_NAMES[case[3]]
    w4 = (w + 3) // 4 * 4
    sp, dp, mp = (w + 5, w + 3, w + 7) if odd else (w4 + 8, w4 + 4, w4 + 16)
    mode, mode_y = 'constant', 'mirror'
    with tuned(ctx, **kn):
        plain = call(ctx, src, k, mode, mode_y, mask=m)
        got = call(ctx, src, k, mode, mode_y, mask=m, sp=sp, dp=dp, mp=mp, pad_rows=2)
    bits = np.uint32 if dt is F32 else np.uint64
    inner = np.ascontiguousarray(got[:, :h, :w])
    assert np.array_equal(inner.view(bits), plain.view(bits)), \
        '%d values differ from the contiguous call' % (inner.view(bits) != plain.view(bits)).sum()
    assert (got[:, h:, :] == FILL).all() and (got[:, :, w:] == FILL).all(), 'wrote outside'
    for i in range(3):
        note(name, dt, check(oracle, inner[i], src[i], k, mode, mode_y, m, 'pitched frame %d' % i))


# ---------------------------------------------------------- non-finite data ----
def _nonfinite(ctx, oracle, k, dt, window, m, name):
    shape = (33, 129) if window <= 13 else (70, 150)
    img = cc.nonfinite_frame(shape, dt, window)
    got = call(ctx, img[None], k, 'constant', mask=m)[0]
    want = ref.ref_conv2d(img, k, 'constant', cc.CVAL, None, m) if not isinstance(k, tuple) \
        else ref.ref_sepconv2d(img, k[0], k[1], 'constant', cc.CVAL)
    assert np.isnan(want).any() and np.isinf(want).any() and np.isfinite(want).any()
    note(name, dt, check(oracle, got, img, k, 'constant', None, m, 'non-finite'))


@pytest.mark.parametrize('case', cc.CONV_CASES, ids=cc.conv_id)
def test_conv2d_nonfinite(ctx, oracle, case):
    """NaN on an edge pixel and in the interior, +inf, -inf, and a kernel with an exact 0.0 tap:
    the NaN / inf pattern is the reference's (0 x inf is NaN), the finite pixels meet the bound"""
    dt, kh, kw, flags, want_path = case
    assert cc.path('conv2d', dt, kh, kw, flags) == want_path
    m = cc.mask((33, 129)) if flags & cc.MASKED else None
    with tuned(ctx, **knobs_of(case)):
        _nonfinite(ctx, oracle, cc.kernel2d(kh, kw), dt, max(kh, kw), m, CONV_NAMES[want_path])


@pytest.mark.parametrize('case', cc.SEP_CASES, ids=cc.sep_id)
def test_sepconv2d_nonfinite(ctx, oracle, case):
    dt, nky, nkx, want_path = case
    assert cc.path('sepconv2d', dt, nky, nkx) == want_path
    _nonfinite(ctx, oracle, cc.sep_taps(nky, nkx), dt, max(nky, nkx), None, SEP_NAMES[want_path])


# ---------------------------------------------------------------- refusals ----
def test_refusals(ctx):
    """pinned as they are: in place, integer images, a pitch below the width, a border id out of
    range, short even tap counts - and the destination untouched"""
    from imgprocessor_amd import _lib, ops
    from imgprocessor_amd.device import dtype_id
    L, hnd = ctx._lib, ctx.handle
    h, w = 9, 20
    img = cc.frame((h, w), F32)
    src, dst = ctx.to_device(img), ctx.to_device(np.full((h, w), FILL, F32))
    _, pk = _dp(cc.kernel2d(3, 3))
    _, pt = _dp(cc.taps(3))
    _, pe = _dp(cc.taps(4))
    f32, refl = dtype_id(F32), ops.border_id('reflect')

    def conv(s=src, d=dst, dt=f32, sp=w, dp=w, bx=refl, by=refl):
        return L.ipa_conv2d_dev(hnd, s.ptr, dt, h, w, sp, pk, 3, 3, None, 0, d.ptr, dp, 1, h * w,
                                h * w, bx, by, 0.0)

    def sep(s=src, d=dst, dt=f32, sp=w, dp=w, bx=refl, by=refl, ky=(pt, 3), kx=(pt, 3)):
        return L.ipa_sepconv2d_dev(hnd, s.ptr, dt, h, w, sp, ky[0], ky[1], kx[0], kx[1], d.ptr, dp,
                                   1, h * w, h * w, by, bx, 0.0)
    for f in (conv, sep):
        assert f() == _lib.OK
        dst.set(np.full((h, w), FILL, F32))
        assert f(d=src) == _lib.ERR_BAD_ARG                      # in place
        for dt in (np.uint8, np.uint16):
            assert f(dt=dtype_id(dt)) == _lib.ERR_UNSUPPORTED    # integer images
        assert f(sp=w - 1) == _lib.ERR_BAD_ARG and f(dp=w - 1) == _lib.ERR_BAD_ARG
        for b in (-1, 5):
            assert f(bx=b) == _lib.ERR_BAD_ARG and f(by=b) == _lib.ERR_BAD_ARG
    for ky, kx in (((pe, 4), (pe, 4)), ((pe, 4), (pt, 3)), ((pt, 3), (pe, 4)), ((pe, 4), (pt, 0)),
                   ((pt, 0), (pe, 4))):
        assert sep(ky=ky, kx=kx) == _lib.ERR_BAD_ARG             # short even tap counts
    assert (dst.get() == FILL).all()
    assert np.array_equal(src.get(), img)


# (name, entry point, the arguments that differ from a good call, status).  The statuses are those of the checks
# in the order the entry points make them: every BAD_ARG check before the dtype's UNSUPPORTED, short even tap
# counts before the dtype, long ones never.  `inplace`: the destination is the source.
U8 = np.uint8
REFUSAL_ORDER = (
    ('conv2d-null-kernel', 'conv', dict(k=None), 'ERR_BAD_ARG'),
    ('conv2d-kh0', 'conv', dict(kh=0), 'ERR_BAD_ARG'),
    ('conv2d-frames0', 'conv', dict(n=0), 'ERR_BAD_ARG'),
    ('conv2d-frames65536', 'conv', dict(n=65536), 'ERR_BAD_ARG'),
    ('conv2d-mask-pitch', 'conv', dict(mask=True, mp=19), 'ERR_BAD_ARG'),
    ('conv2d-u8-src-pitch', 'conv', dict(dt=U8, sp=19), 'ERR_BAD_ARG'),       # pitch before dtype
    ('conv2d-u8-border', 'conv', dict(dt=U8, bx=-1), 'ERR_BAD_ARG'),
    ('conv2d-u8-inplace', 'conv', dict(dt=U8, inplace=True), 'ERR_BAD_ARG'),
    ('conv2d-257x256', 'conv', dict(k=(257, 256)), 'ERR_BAD_ARG'),            # 65 792 taps
    ('sep-nky-1', 'sep', dict(ky=3, nky=-1), 'ERR_BAD_ARG'),
    ('sep-null-ky', 'sep', dict(ky=None, nky=3), 'ERR_BAD_ARG'),
    ('sep-4taps-u8', 'sep', dict(ky=4, kx=4, dt=U8), 'ERR_BAD_ARG'),          # odd taps before dtype
    ('sep-3taps-u8-dst-pitch', 'sep', dict(dt=U8, dp=19), 'ERR_BAD_ARG'),
    ('sep-3taps-u8', 'sep', dict(dt=U8), 'ERR_UNSUPPORTED'),
    ('sep-64taps-u8', 'sep', dict(ky=64, kx=64, dt=U8), 'ERR_UNSUPPORTED'),
    ('sep-64taps-inplace', 'sep', dict(ky=64, kx=64, inplace=True), 'ERR_BAD_ARG'),
    ('sep-64taps-src-pitch', 'sep', dict(ky=64, kx=64, sp=19), 'ERR_BAD_ARG'),
    # these two: refused before the temporary of the two generic launches is sized from n_frames
    ('sep-64taps-frames-1', 'sep', dict(ky=64, kx=64, n=-1), 'ERR_BAD_ARG'),
    ('sep-64taps-frames0', 'sep', dict(ky=64, kx=64, n=0), 'ERR_BAD_ARG'),
    # ... and so before the first generic launch met the dtype: it was UNSUPPORTED while the destination's pitch
    # was looked at by the second launch only
    ('sep-64taps-u8-dst-pitch', 'sep', dict(ky=64, kx=64, dt=U8, dp=19), 'ERR_BAD_ARG'),
    ('sep-65537taps', 'sep', dict(ky=65537, kx=0), 'ERR_BAD_ARG'),            # more than the generic kernel takes
    ('sep-0taps', 'sep', dict(ky=0, kx=0), 'OK'),                             # no axis: a copy
)


@pytest.mark.parametrize('row', REFUSAL_ORDER, ids=[r[0] for r in REFUSAL_ORDER])
def test_refusal_order(ctx, row):
    """the status of every refusal whose place among the checks decides it, on the C ABI alone: a 9 x 20 float32
    frame, FILL in the destination.  Afterwards the destination is still FILL - after the one call that succeeds,
    without taps on either axis, the bits of the source - and the source is intact."""
    from imgprocessor_amd import _lib, ops
    from imgprocessor_amd.device import dtype_id
    name, op, a, want = row
    L, hnd = ctx._lib, ctx.handle
    h, w = 9, 20
    assert a.get('sp', w) in (w, w - 1) and a.get('dp', w) in (w, w - 1) and a.get('mp', w) in (w, w - 1)
    img = cc.frame((h, w), F32)
    src, dst = ctx.to_device(img), ctx.to_device(np.full((h, w), FILL, F32))
    d = src if a.get('inplace') else dst
    dt, refl = dtype_id(a.get('dt', F32)), ops.border_id('reflect')
    n, sp, dp = a.get('n', 1), a.get('sp', w), a.get('dp', w)
    keep = []

    def ptr(v, make):
        """null for None, else the float64 array make(v) - kept alive until the call returns"""
        if v is None:
            return None
        arr, p = _dp(make(v))
        keep.append(arr)
        return p

    if op == 'conv':
        kshape = a.get('k', (3, 3))
        pk = ptr(kshape, lambda s: np.full(s, 1.0 / (s[0] * s[1])))
        kh, kw = kshape if kshape is not None else (3, 3)
        m = ctx.to_device(np.ones((h, w), np.uint8)) if a.get('mask') else None
        rc = L.ipa_conv2d_dev(hnd, src.ptr, dt, h, w, sp, pk, a.get('kh', kh), kw, m.ptr if m is not None else None,
                              a.get('mp', w), d.ptr, dp, n, h * w, h * w, a.get('bx', refl), refl, 0.0)
    else:
        ky, kx = a.get('ky', 3), a.get('kx', 3)
        pky, pkx = (ptr(t, lambda c: cc.taps(c) if c else np.zeros(1)) for t in (ky, kx))
        rc = L.ipa_sepconv2d_dev(hnd, src.ptr, dt, h, w, sp, pky, a.get('nky', ky), pkx, kx, d.ptr, dp, n, h * w,
                                 h * w, refl, refl, 0.0)
    assert rc == getattr(_lib, want), '%s: status %d (%s)' % (
        name, rc, (L.ipa_last_error(hnd) or b'').decode() if rc else '')
    out = dst.get()
    if want == 'OK':
        assert np.array_equal(out.view(np.uint32), img.view(np.uint32)), 'no taps: not the bits of the source'
    else:
        assert (out == FILL).all(), 'a refused call wrote to the destination'
    assert np.array_equal(src.get(), img)


@pytest.mark.parametrize('nky,nkx', [(64, 0), (0, 64), (64, 3), (64, 64)])
def test_long_even_taps_are_accepted(ctx, oracle, nky, nkx):
    """64 taps on an axis leave for the generic kernel BEFORE the odd-tap check that refuses 4:
    accepted, with the centre at k // 2 like scipy's (the inconsistency is stated in the header
    comment of ipa_sepconv2d_dev)"""
    want_path = cc.SEP_ONE_GENERIC if 0 in (nky, nkx) else cc.SEP_TWO_GENERIC
    k = cc.sep_taps(nky, nkx)
    for dt in cc.DTYPES:
        assert cc.path('sepconv2d', dt, nky, nkx) == want_path
        for shape in cc.LONG:
            img = cc.frame(shape, dt)
            for mode in ('reflect', 'constant'):
                got = call(ctx, img[None], k, mode)[0]
                note(SEP_NAMES[want_path], dt, check(oracle, got, img, k, mode, None, None,
                                                     '%dx%d %s %s' % (nky, nkx, shape, mode)))


def test_zz_report():
    """the figures of this run (reported values, not thresholds)"""
    print()
    for key in sorted(WORST):
        print('worst err / bound  %-34s %.3f' % (key, WORST[key]))
    assert all(v <= 1.0 for v in WORST.values())
