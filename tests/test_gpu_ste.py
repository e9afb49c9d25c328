"""GPU: single-time-effect removal (csrc/ste.hip, features/SingleTimeEffectDetection.py) and
removeSinglePixels, bit-equal to the reference's outputs (tests/golden/ste.npz) and to the numpy
restatement of test_cpu_ste.py on ragged sizes, a 4K frame, every frames-per-launch boundary,
the threshold's special values, the decision's knife edge and pitched frames.
"""
import numpy as np
import pytest

from .conftest import load_golden
from .test_cpu_ste import SteNumpy, bounded_nlf, same_f64

pytestmark = pytest.mark.gpu


@pytest.fixture(scope='module')
def ctx():
    import imgprocessor_amd
    return imgprocessor_amd.default_context(0)


def _S():
    from imgprocessor_amd.features import SingleTimeEffectDetection
    return SingleTimeEffectDetection


def _bits(a, b, what):
    assert same_f64(a, b), '%s differs at %d pixels' % (what, int(np.sum(
        (np.asarray(a).view(np.int64) != np.asarray(b).view(np.int64)) &
        ~(np.isnan(a) & np.isnan(b)))))


def _check(s, ref, what):
    _bits(s.threshold, ref.thr, what + ' threshold')
    _bits(s.noSTE, ref.avg, what + ' noSTE')
    assert np.array_equal(s.mask_clean, ref.mask_clean), what + ' mask_clean'
    if s.mask_STE is not None:
        assert np.array_equal(s.mask_STE, ref.mask_ste), what + ' mask_STE'


def _scene(n, h, w, dtype, seed, nan=True):
    rng = np.random.default_rng(seed)
    y, x = np.mgrid[0:h, 0:w].astype(np.float64)
    base = 200 + 1500 * (x + y) / max(h + w - 2, 1)
    f = base + 6 * rng.standard_normal((n, h, w))
    f += (rng.random((n, h, w)) < 0.01) * 600                      # hits
    f += (rng.random((n, h, w)) < 0.04) * rng.uniform(20, 60, (n, h, w))   # near the threshold
    for k in range(n):                                              # pairs, so that some survive
        ys, xs = rng.integers(0, h, 8), rng.integers(0, w, 8)
        f[k, ys, xs] += 700
        f[k, ys, np.minimum(xs + 1, w - 1)] += 700
    if dtype == np.uint8:
        f = f / 8
    if np.dtype(dtype).kind == 'f':
        if nan:
            f[rng.random((n, h, w)) < 0.002] = np.nan
        return f.astype(dtype)
    return np.clip(np.round(f), 0, np.iinfo(dtype).max).astype(dtype)


NLF = (3.0, 150.0, 1.1)
NLF8 = (1.0, 20.0, 0.4)   # for uint8 frames (the scene / 8)


def test_ste_golden(ctx):
    S = _S()
    g = load_golden('ste.npz')
    print('running mean of the fixture: %s' % g['mma_source'])
    for i in range(int(g['n_cases'])):
        p = 'c%d_' % i
        fr = g[p + 'frames']
        s = S(list(fr), tuple(g[p + 'nlf']), float(g[p + 'nstd']), save_ste_indices=True)
        assert np.array_equal(s.threshold.view(np.int64), g[p + 'thr'].view(np.int64)), p + 'thr'
        _bits(s.noSTE, g[p + 'noSTE'], p + 'noSTE')
        assert np.array_equal(s.mask_clean, g[p + 'mask_clean']), p + 'mask_clean'
        assert np.array_equal(s.mask_STE, g[p + 'mask_ste']), p + 'mask_STE'
        s.addImage(g[p + 'add'], g[p + 'add_mask'])
        _bits(s.noSTE, g[p + 'noSTE2'], p + 'noSTE2')
        assert np.array_equal(s.mask_clean, g[p + 'mask_clean2']), p + 'mask_clean2'
        assert np.array_equal(s.mask_STE, g[p + 'mask_ste2']), p + 'mask_STE2'
        assert s.relativeAreaSTE() == np.sum(g[p + 'mask_ste2']) / fr[0].size
        # device frames give device results, the same bits
        d = S(ctx.to_device(fr), tuple(g[p + 'nlf']), float(g[p + 'nstd']))
        _bits(d.noSTE.get(), g[p + 'noSTE'], p + 'device noSTE')
        assert np.array_equal(d.mask_clean.get() != 0, g[p + 'mask_clean']), p + 'device clean'


def test_remove_single_pixels_golden(ctx):
    from imgprocessor_amd.filters import removeSinglePixels
    g = load_golden('ste.npz')
    for j in range(int(g['n_rsp'])):
        a = g['rsp%d_in' % j].copy()
        removeSinglePixels(a)
        assert np.array_equal(a, g['rsp%d_out' % j]), 'rsp%d host' % j
        d = ctx.to_device(g['rsp%d_in' % j].astype(np.uint8))
        removeSinglePixels(d)
        assert np.array_equal(d.get() != 0, g['rsp%d_out' % j]), 'rsp%d device' % j


@pytest.mark.parametrize('shape', [(1, 1), (1, 300), (250, 1), (203, 391)])
@pytest.mark.parametrize('dtype', [np.uint8, np.uint16, np.float32, np.float64])
def test_ste_ragged(ctx, shape, dtype):
    fr = _scene(5, shape[0], shape[1], dtype, 3)
    nlf = NLF8 if dtype == np.uint8 else NLF
    ref = SteNumpy(fr, nlf, 4)
    _check(_S()(fr, nlf, 4, save_ste_indices=True), ref, '%s %s' % (shape, np.dtype(dtype)))


@pytest.mark.parametrize('n', [2, 3, 4, 7, 8, 9, 16, 17])
def test_ste_frame_counts(ctx, n):
    fr = _scene(n, 150, 260, np.float32, 10 + n)
    ref = SteNumpy(fr, NLF, 2.5)
    s = _S()(ctx.to_device(fr), NLF, 2.5, save_ste_indices=True)
    _bits(s.noSTE.get(), ref.avg, 'n=%d noSTE' % n)
    _bits(s.threshold.get(), ref.thr, 'n=%d thr' % n)
    assert np.array_equal(s.mask_STE.get() != 0, ref.mask_ste), 'n=%d mask_STE' % n
    assert np.array_equal(s.mask_clean.get() != 0, ref.mask_clean), 'n=%d mask_clean' % n
    # one launch per frame: the same bits
    ctx.set_tuning(ste_frames=1)
    try:
        s1 = _S()(ctx.to_device(fr), NLF, 2.5, save_ste_indices=True)
    finally:
        ctx.set_tuning(ste_frames=8)
    _bits(s1.noSTE.get(), ref.avg, 'n=%d F=1 noSTE' % n)
    assert np.array_equal(s1.mask_STE.get() != 0, ref.mask_ste), 'n=%d F=1 mask_STE' % n


def test_ste_4k(ctx):
    fr = _scene(6, 2160, 3840, np.uint16, 42)
    ref = SteNumpy(fr, NLF, 4)
    _check(_S()(fr, NLF, 4, save_ste_indices=True), ref, '4K')


def test_ste_threshold_special_values(ctx):
    rng = np.random.default_rng(5)
    v = np.concatenate([
        np.array([0.0, -0.0, -1.0, -1e300, 5e-324, -5e-324, 2.2e-308, np.inf, -np.inf, np.nan,
                  150.0, np.nextafter(150.0, 0), np.nextafter(150.0, 1e9), 1e308, 1.7e308]),
        rng.standard_normal(300000) * 10.0 ** rng.integers(-320, 308, 300000),
        rng.uniform(-10, 1e4, 300000),
        rng.integers(0, 2 ** 64, 399985, dtype=np.uint64).view(np.float64)])
    assert v.size == 10 ** 6
    img = v.reshape(1000, 1000)
    for tri in [(-1.0, 0.0, 1.5), (0.25, 150.0, 3.0), (-2.0, -5.0, -0.7), (1e-320, 1e-310, 1e300)]:
        s = _S()(np.stack([img, img]), tri, 4)
        want = bounded_nlf(img, *tri) * 4
        got = s.threshold
        assert np.array_equal(got.view(np.int64)[~np.isnan(want)],
                              want.view(np.int64)[~np.isnan(want)]), tri
        assert np.array_equal(np.isnan(got), np.isnan(want)), tri


def test_ste_knife_edge(ctx):
    def fresh():   # avg 0, thr = max(0.5 * sqrt(0), 4) * 4 = 16
        s = _S()(np.zeros((2, 16, 16)), (4.0, 0.0, 0.5), 4)
        assert np.all(s.threshold == 16.0)
        return s

    g = np.zeros((16, 16))
    g[5, 5] = g[5, 6] = 16.0                       # d == thr: no STE
    s = fresh().addImage(g)
    assert s.mask_clean[5, 5] and s.mask_clean[5, 6]
    g[5, 5] = g[5, 6] = np.nextafter(16.0, np.inf)   # d just above: an STE pair
    g[9, 9] = 1e9                                    # a lone pixel is always cleared
    s = fresh().addImage(g)
    assert not s.mask_clean[5, 5] and not s.mask_clean[5, 6] and s.mask_clean[9, 9]


def test_ste_construction_then_add_image(ctx):
    fr = _scene(9, 120, 200, np.uint16, 77)
    a = _S()(fr, NLF, 4, save_ste_indices=True)
    b = _S()(fr[:2], NLF, 4, save_ste_indices=True)
    for f in fr[2:]:
        b.addImage(f)
    _bits(a.noSTE, b.noSTE, 'noSTE')
    _bits(a.threshold, b.threshold, 'threshold')
    assert np.array_equal(a.mask_STE, b.mask_STE) and np.array_equal(a.mask_clean, b.mask_clean)
    _check(a, SteNumpy(fr, NLF, 4), 'n=9')
    # a caller mask on addImage
    m = np.random.default_rng(1).random((120, 200)) < 0.7
    ref = SteNumpy(fr[:2], NLF, 4)
    ref.add(fr[2], m)
    c = _S()(fr[:2], NLF, 4, save_ste_indices=True).addImage(fr[2], m)
    _check(c, ref, 'masked addImage')


def test_ste_callable_nlf(ctx):
    from imgprocessor_amd.features import SingleTimeEffectDetection as S
    fr = _scene(4, 90, 170, np.float32, 8)
    a = S(fr, NLF, 4, save_ste_indices=True)
    b = S(list(fr), lambda x: bounded_nlf(x, *NLF), 4, save_ste_indices=True)
    _bits(a.threshold, b.threshold, 'threshold')
    _bits(a.noSTE, b.noSTE, 'noSTE')
    assert np.array_equal(a.mask_STE, b.mask_STE)
    d = S([ctx.to_device(f) for f in fr], lambda x: bounded_nlf(x, *NLF), 4)
    _bits(d.noSTE.get(), a.noSTE, 'device list, callable')


def test_ste_pitched_frames(ctx):
    from imgprocessor_amd import DeviceArray, _lib as L
    n, h, w, pitch, rows = 7, 70, 150, 173, 77
    fr = _scene(n, h, w, np.float32, 9)
    ref = SteNumpy(fr, NLF, 4)
    big = np.full((n, rows, pitch), 1e30, np.float32)   # padding: an STE everywhere if read
    big[:, 1::2, w:] = -1e30
    big[:, :h, :w] = fr
    d = ctx.to_device(big)
    sp = 181
    avg, thr = DeviceArray(ctx, (h, sp), np.float64), DeviceArray(ctx, (h, sp), np.float64)
    cnt = DeviceArray.counts(ctx, (h, sp))
    ste, clean = DeviceArray(ctx, (h, sp), np.uint8), DeviceArray(ctx, (h, sp), np.uint8)
    ctx._check(ctx._lib.ipa_memset(ctx.handle, ste.ptr, 0, ste.nbytes))
    for F in (8, 1):
        ctx.set_tuning(ste_frames=F)
        try:
            ctx._check(ctx._lib.ipa_ste_dev(ctx.handle, d.ptr, L.F32, n, h, w, pitch, rows * pitch,
                                            1, L.dbl(NLF, 3), 4.0, avg.ptr, cnt.ptr, thr.ptr, sp,
                                            None, ste.ptr, clean.ptr, sp))
        finally:
            ctx.set_tuning(ste_frames=8)
        _bits(avg.get()[:, :w], ref.avg, 'pitched noSTE F=%d' % F)
        _bits(thr.get()[:, :w], ref.thr, 'pitched thr F=%d' % F)
        assert np.array_equal(ste.get()[:, :w] != 0, ref.mask_ste)
        assert np.array_equal(clean.get()[:, :w] != 0, ref.mask_clean)


def test_ste_bad_args(ctx):
    from imgprocessor_amd import DeviceArray, _lib as L
    h, w = 8, 8
    fr = ctx.to_device(np.zeros((3, h, w), np.float32))
    st = [DeviceArray(ctx, (h, w), np.float64), DeviceArray.counts(ctx, (h, w)),
          DeviceArray(ctx, (h, w), np.float64)]
    lib, nlf = ctx._lib, L.dbl(NLF, 3)

    def call(frames, n, first, nlf_, avg, cnt, thr):
        return lib.ipa_ste_dev(ctx.handle, frames, L.F32, n, h, w, w, h * w, first, nlf_, 4.0,
                               avg, cnt, thr, w, None, None, None, w)

    assert call(fr.ptr, 1, 1, nlf, st[0].ptr, st[1].ptr, st[2].ptr) == L.ERR_BAD_ARG
    assert call(fr.ptr, 2, 1, None, st[0].ptr, st[1].ptr, None) == L.ERR_BAD_ARG
    assert call(fr.ptr, 2, 1, nlf, fr.ptr, st[1].ptr, st[2].ptr) == L.ERR_BAD_ARG   # overlap
    assert call(fr.ptr, 2, 1, nlf, st[0].ptr, st[1].ptr, st[0].ptr) == L.ERR_BAD_ARG
    assert call(fr.ptr, 2, 1, nlf, st[0].ptr, st[1].ptr, st[2].ptr) == L.OK
    ctx.synchronize()


@pytest.mark.parametrize('frames_per_launch', [8, 1])
@pytest.mark.parametrize('n_more', [1, 8, 9, 16, 17])
def test_ste_continuation_launches(ctx, n_more, frames_per_launch):
    """ops.ste_update continuing a stored state over n_more frames in ONE call: one launch
    (state copied to the workspace first), an even number of launches (the first reads the
    caller's state) and an odd number above one (copy, then alternation), with a caller mask"""
    from imgprocessor_amd import DeviceArray, ops
    h, w = 140, 270
    fr = _scene(2 + n_more, h, w, np.uint16, 300 + n_more)
    m = np.random.default_rng(n_more).random((h, w)) < 0.85
    ref = SteNumpy(fr[:2], NLF, 4)
    for f in fr[2:]:
        ref.add(f, m)
    avg, thr = DeviceArray(ctx, (h, w), np.float64), DeviceArray(ctx, (h, w), np.float64)
    cnt = DeviceArray.counts(ctx, (h, w))
    ste, clean = DeviceArray(ctx, (h, w), np.uint8), DeviceArray(ctx, (h, w), np.uint8)
    ctx._check(ctx._lib.ipa_memset(ctx.handle, ste.ptr, 0, ste.nbytes))
    ops.ste_update(fr[:2], avg, cnt, thr, first_pair=True, nlf=NLF, nstd=4, mask_ste=ste,
                   mask_clean=clean)
    old = ctx.set_tuning(ste_frames=frames_per_launch)
    try:
        ops.ste_update(ctx.to_device(fr[2:]), avg, cnt, thr, first_pair=False, mask=m,
                       mask_ste=ste, mask_clean=clean)
    finally:
        ctx.set_tuning(**old)
    what = 'n_more=%d F=%d' % (n_more, frames_per_launch)
    _bits(avg.get(), ref.avg, what + ' noSTE')
    assert np.array_equal(cnt.get(), ref.count), what + ' count'
    _bits(thr.get(), ref.thr, what + ' thr')
    assert np.array_equal(ste.get() != 0, ref.mask_ste), what + ' mask_STE'
    assert np.array_equal(clean.get() != 0, ref.mask_clean), what + ' mask_clean'
