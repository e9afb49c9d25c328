"""GPU: single-time-effect removal (csrc/ste.hip, features/SingleTimeEffectDetection.py) and
removeSinglePixels, bit-equal to the reference's outputs (tests/golden/ste.npz) and to the numpy
restatement of test_cpu_ste.py on ragged sizes, a 4K frame, every frames-per-launch boundary,
the threshold's special values, the decision's knife edge and pitched frames.

The fuse and adjacency scenes of tests/ste_cases.py put a dependency chain of exactly `steps`
pixels across every kind of tile border of every launch, and candidate pairs across every wave
row boundary, the seam of the two ballot words, the output-tile borders and the image's edges;
test_cpu_ste.py proves on the CPU which defect of the tile algorithm each of them sees.
"""
import ctypes as C

import numpy as np
import pytest

from .conftest import load_golden
from . import ste_cases as sc
from .ste_cases import NLF, NLF8, random_scene as _scene
from .test_cpu_ste import SteNumpy, bounded_nlf, remove_single_pixels, same_f64

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


# ------------------------------------------------------------ built scenes (ste_cases.py) ----
def _check_dev(s, ref, what):
    _bits(s.threshold.get(), ref.thr, what + ' thr')
    _bits(s.noSTE.get(), ref.avg, what + ' noSTE')
    assert np.array_equal(s.mask_STE.get() != 0, ref.mask_ste), what + ' mask_STE'
    assert np.array_equal(s.mask_clean.get() != 0, ref.mask_clean), what + ' mask_clean'


@pytest.mark.parametrize('steps', sc.FUSE_STEPS)
def test_ste_fuses(ctx, steps):
    """a chain of `st` pixels into the first and last output pixel of the tiles of every launch,
    from all eight directions: every steps-per-launch from 1 to 8, and calls of 2 and 3 launches"""
    fr, fuses, ref = sc.fuse_case(steps)
    s = _S()(ctx.to_device(fr), sc.NLF_CONST, sc.NSTD_CONST, save_ste_indices=True)
    _check_dev(s, ref, 'fuses, %d steps' % steps)
    ste = s.mask_STE.get()
    assert all(ste[f['P']] for f in fuses if f['kind'] != 'unlit')


@pytest.mark.parametrize('n_more', sc.CONT_MORE)
def test_ste_fuses_continuing(ctx, n_more):
    """the same through ops.ste_update on a stored state: one launch (the state copied to the
    workspace first), two, and three, under a caller mask that covers one link of some fuses"""
    from imgprocessor_amd import DeviceArray, ops
    fr, fuses, m, ref, hit = sc.cont_case(n_more)
    h, w = sc.FUSE_HW
    avg, thr = DeviceArray(ctx, (h, w), np.float64), DeviceArray(ctx, (h, w), np.float64)
    cnt = DeviceArray.counts(ctx, (h, w))
    ste, clean = DeviceArray(ctx, (h, w), np.uint8), DeviceArray(ctx, (h, w), np.uint8)
    ctx._check(ctx._lib.ipa_memset(ctx.handle, ste.ptr, 0, ste.nbytes))
    ops.ste_update(fr[:2], avg, cnt, thr, first_pair=True, nlf=sc.NLF_CONST, nstd=sc.NSTD_CONST,
                   mask_ste=ste, mask_clean=clean)
    ops.ste_update(ctx.to_device(fr[2:]), avg, cnt, thr, first_pair=False, mask=m, mask_ste=ste,
                   mask_clean=clean)
    what = 'fuses, %d more frames' % n_more
    _bits(avg.get(), ref.avg, what + ' noSTE')
    assert np.array_equal(cnt.get(), ref.count), what + ' count'
    assert np.array_equal(ste.get() != 0, ref.mask_ste), what + ' mask_STE'
    assert np.array_equal(clean.get() != 0, ref.mask_clean), what + ' mask_clean'


@pytest.mark.parametrize('dtype', sc.ADJ_DTYPES)
@pytest.mark.parametrize('st', sc.ADJ_STEPS)
def test_ste_adjacency(ctx, st, dtype):
    """pairs in all eight directions across every wave row boundary, the 63 | 64 seam, the
    output-tile borders and the image's edges and corners, in step 0 and step 1 of a launch"""
    fr, pairs, ref = sc.adj_case(st, dtype)
    assert fr.dtype == dtype
    s = _S()(ctx.to_device(fr), sc.NLF_CONST, sc.NSTD_CONST, save_ste_indices=True)
    _check_dev(s, ref, 'pairs, %d steps, %s' % (st, np.dtype(dtype).name))


def _rsp_input(shape, seed):
    rng = np.random.default_rng(seed)
    a = rng.random(shape) < 0.12
    a.flat[0] = a.flat[-1] = True
    if shape[1] > 64:
        a[0, 63] = a[-1, 64] = True       # across two workgroups in x
    if shape[0] > 4:
        a[3, 1] = a[4, 2] = True          # and in y
    return a


@pytest.mark.parametrize('shape', [(1, 1), (1, 65), (5, 64), (4, 129), (9, 63)])
def test_remove_single_pixels_shapes(ctx, shape):
    from imgprocessor_amd import ops
    a = _rsp_input(shape, shape[0] * 131 + shape[1])
    want = remove_single_pixels(a)
    assert np.array_equal(ops.remove_single_pixels(a, ctx=ctx), want)
    d = ops.remove_single_pixels(ctx.to_device(a.astype(np.uint8) * 7))   # non-zero is set
    assert d.dtype == np.uint8 and np.array_equal(d.get(), want.astype(np.uint8))


def test_remove_single_pixels_pitched_and_in_place(ctx):
    h, w, ip, op = 9, 129, 140, 133
    a = _rsp_input((h, w), 5)
    big = np.ones((h + 1, ip), np.uint8)       # set padding: a neighbour everywhere if read
    big[:h, :w] = a
    d_in = ctx.to_device(big)
    d_out = ctx.to_device(np.full((h + 1, op), 9, np.uint8))
    ctx._check(ctx._lib.ipa_remove_single_pixels_dev(ctx.handle, d_in.ptr, h, w, ip, d_out.ptr, op))
    got = d_out.get()
    assert np.array_equal(got[:h, :w], remove_single_pixels(a).astype(np.uint8))
    assert (got[h:] == 9).all() and (got[:, w:] == 9).all(), 'wrote outside'
    # in place, or overlapping by one row: refused on the host, nothing written
    from imgprocessor_amd import _lib as L
    assert ctx._lib.ipa_remove_single_pixels_dev(ctx.handle, d_in.ptr, h, w, ip, d_in.ptr, ip) == L.ERR_BAD_ARG
    last_row = C.c_void_p(d_in.ptr.value + (h - 1) * ip)
    assert ctx._lib.ipa_remove_single_pixels_dev(ctx.handle, d_in.ptr, h, w, ip, last_row, ip) == L.ERR_BAD_ARG
    ctx.synchronize()
    assert np.array_equal(d_in.get(), big)
