"""GPU: the flat field from spot images (csrc/spot.hip, camera/flatField/vignettingFromSpotAverage.py)
against the numpy restatement (tests/spot_ref.py), numpy's own histogram, scipy's minimum_filter and
scipy.ndimage.label, and the fixture the unchanged reference wrote (tests/golden/spot.npz).

Everything up to the take is integer or selection arithmetic: counts, thresholds, masks, labels, n,
sizes and coordinate sums are compared bit for bit.  The take's sum is added in the device's fixed
order: it lies within count * 2**-53 * sum|x| of math.fsum - the bound of any summation order - and
repeats its bits from call to call.

Shapes: 1 x 1, single rows and columns, one labelling tile (16 x 64) and one tile plus or minus one
pixel in each direction, 3 x 3 tiles, one histogram workgroup's share (256 lanes x 8 pixels) plus
or minus one pixel, and one frame of 2.2 M pixels whose single component fills it (more than one
trip of every grid-stride loop).  Pitched rows with guard-valued padding go through the C ABI.
"""
import ctypes as C
import gc
import math

import numpy as np
import pytest
from scipy import ndimage

from . import spot_cases as sc
from . import spot_ref as ref
from .conftest import load_golden
from .test_cpu_dark import same
from .test_gpu_dark import DT_ID, GUARD, padded

pytestmark = pytest.mark.gpu

EIGHT = np.ones((3, 3), int)
IGUARD = -77
SCENES = sc.scenes()
SHARE = 256 * 8     # pixels one workgroup of the histogram takes per trip


@pytest.fixture(scope='module')
def ctx():
    import imgprocessor_amd
    return imgprocessor_amd.default_context(0)


@pytest.fixture(scope='module')
def g():
    return load_golden('spot.npz')


def _ops():
    from imgprocessor_amd import ops
    return ops


def frame_of(rng, shape, dtype):
    top = 250 if np.dtype(dtype) == np.uint8 else 4000
    a = rng.uniform(0, top, shape)
    return np.round(a).astype(dtype) if np.dtype(dtype).kind == 'u' else a.astype(dtype)


def backgrounds(rng, shape):
    return {'none': None, 'scalar': 3.25, 'array': rng.uniform(0, 9, shape)}


def minus(img, bg):
    return ref.frame(img, 0.0 if bg is None else bg)


def scipy_label(m, conn):
    return ndimage.label(m, EIGHT if conn == 2 else None)


# ------------------------------------------------------------------ histogram, Otsu
@pytest.mark.parametrize('dtype', sc.ALL_DTYPES, ids=lambda d: np.dtype(d).name)
def test_histogram_and_otsu_types_and_backgrounds(ctx, dtype):
    ops, rng = _ops(), np.random.default_rng(1)
    img = frame_of(rng, (37, 301), dtype)
    for kind, bg in backgrounds(rng, img.shape).items():
        x = minus(img, bg)
        for nbins in (1, 256, 2048):
            counts, edges = ops.histogram(img, nbins, bg=bg, ctx=ctx)
            want, want_edges = np.histogram(x, nbins)
            assert same(edges, want_edges) and counts.dtype == np.int64
            assert np.array_equal(counts, want), (kind, nbins)
            assert np.array_equal(counts, ref.histogram(x, nbins)[0])
        for nbins in (256, 2048):
            assert ops.otsu_threshold(img, bg=bg, nbins=nbins, ctx=ctx) == ref.otsu(x, nbins), (kind, nbins)
    # device frame, device background
    d_img, d_bg = ctx.to_device(img), ctx.to_device(np.ascontiguousarray(backgrounds(rng, img.shape)['array']))
    counts, _ = ops.histogram(d_img, 256, bg=d_bg)
    assert np.array_equal(counts, np.histogram(minus(img, d_bg.get()), 256)[0])


@pytest.mark.parametrize('top', (7, 100, 255))
def test_histogram_values_on_bin_edges(ctx, top):
    ops, rng = _ops(), np.random.default_rng(top)
    img = rng.integers(0, top + 1, (23, 117)).astype(np.uint8)
    img[0, :2] = 0, top
    for dtype in (np.uint8, np.float64):
        for nbins in (1, top, 256, 2048):
            counts, edges = ops.histogram(img.astype(dtype), nbins, ctx=ctx)
            want, want_edges = np.histogram(img.astype(np.float64), nbins)
            assert same(edges, want_edges) and np.array_equal(counts, want), (dtype, nbins)
        assert ops.otsu_threshold(img.astype(dtype), ctx=ctx) == ref.otsu(img)


@pytest.mark.parametrize('shape', [(1, 1), (1, 257), (1, SHARE - 1), (1, SHARE), (1, SHARE + 1), (3, 683)],
                         ids=lambda s: '%dx%d' % s)
def test_histogram_shapes(ctx, shape):
    ops, rng = _ops(), np.random.default_rng(shape[1])
    img = frame_of(rng, shape, np.uint16)
    for nbins in (1, 256, 2048):
        counts, edges = ops.histogram(img, nbins, bg=1.5, ctx=ctx)
        want, want_edges = np.histogram(minus(img, 1.5), nbins)
        assert same(edges, want_edges) and np.array_equal(counts, want), nbins
    assert ops.otsu_threshold(img, bg=1.5, ctx=ctx) == ref.otsu(minus(img, 1.5))


def test_otsu_all_equal_and_non_finite(ctx):
    ops = _ops()
    assert ops.otsu_threshold(np.full((9, 70), 7, np.uint8), bg=2.5, ctx=ctx) == 4.5
    z = np.zeros((3, 5))
    z[0, 0] = -0.0
    t = ops.otsu_threshold(z, ctx=ctx)
    assert t == 0.0 and np.signbit(t)                                  # the first pixel itself
    assert ops.otsu_threshold(np.full((2, 2), np.inf), ctx=ctx) == np.inf
    counts, edges = ops.histogram(np.full((9, 70), 7, np.uint8), 4, ctx=ctx)
    assert same(edges, np.histogram(np.full(3, 7.0), 4)[1]) and counts.tolist() == [0, 0, 630, 0]
    for bad in (np.nan, np.inf, -np.inf):
        x = np.random.default_rng(2).random((6, 40)).astype(np.float32)
        x[3, 17] = bad
        with pytest.raises(ValueError):
            ops.otsu_threshold(x, ctx=ctx)
        with pytest.raises(ValueError):
            ops.histogram(x, ctx=ctx)
    with pytest.raises(ValueError):
        ops.otsu_threshold(np.zeros((4, 4, 3), np.float32), ctx=ctx)


def src_args(ctx, img, bg, pitch_extra=3):
    """the leading arguments of a spot entry point over pitched rows; the padding holds a value that
    would show in every result"""
    h, w = img.shape
    fill = 201 if img.dtype == np.uint8 else 60000
    d_img = ctx.to_device(padded(img, w + pitch_extra, fill))
    d_bg = None if bg is None or np.ndim(bg) == 0 else ctx.to_device(padded(np.asarray(bg, np.float64), w + 2, 1e9))
    args = (ctx.handle, d_img.ptr, DT_ID[img.dtype], h, w, w + pitch_extra, d_bg.ptr if d_bg is not None else None,
            w + 2 if d_bg is not None else 0, 0.0 if d_bg is not None or bg is None else float(bg))
    return (d_img, d_bg), args


def test_pitched_frames_through_the_abi(ctx):
    rng = np.random.default_rng(3)
    img = frame_of(rng, (21, 131), np.uint16)
    for bg in (None, 2.5, rng.uniform(0, 5, img.shape)):
        x = minus(img, bg)
        keep, args = src_args(ctx, img, bg)
        r = (C.c_double * 5)()
        assert ctx._lib.ipa_spot_range_dev(*(args + (r,))) == 0
        assert list(r) == [x.min(), x.max(), 0.0, 0.0, x[0, 0]]
        want, edges = np.histogram(x, 256)
        counts = np.zeros(256, np.uint64)
        assert ctx._lib.ipa_spot_histogram_dev(*(args + (edges.ctypes.data_as(C.POINTER(C.c_double)), 256,
                                                         counts.ctypes.data_as(C.c_void_p)))) == 0
        assert np.array_equal(counts.astype(np.int64), want)
        t = float(np.median(x))
        d_mask = ctx.to_device(np.full((21, 131 + 5), 9, np.uint8))
        assert ctx._lib.ipa_spot_mask_dev(*(args + (t, d_mask.ptr, 131 + 5))) == 0
        got = d_mask.get()
        assert (got[:, 131:] == 9).all() and np.array_equal(got[:, :131], ref.spot_mask(x, t))


# ------------------------------------------------------------------ spot mask
@pytest.mark.parametrize('dtype', sc.ALL_DTYPES, ids=lambda d: np.dtype(d).name)
def test_spot_mask(ctx, dtype):
    ops = _ops()
    h, w = 19, 70
    img = np.full((h, w), 10, dtype)
    for r, c in ((0, 0), (0, w - 5), (h - 5, 0), (h - 5, w - 5), (0, 30), (h - 5, 30), (7, 0), (7, w - 5), (7, 20)):
        img[r:r + 5, c:c + 5] = 100                  # a spot on every corner and edge, one inside
    img[8, 40:60] = 100                              # one pixel wide
    img[12:14, 40:60] = 100                          # two pixels wide
    img[16, 45] = 100                                # a single pixel
    img[2, 2] = 50                                   # exactly the threshold inside a spot: not above it
    for bg, t in ((None, 50.0), (5.0, 45.0), (np.full((h, w), 5.0), 45.0)):
        x = minus(img, bg)
        got = ops.spot_mask(img, t, bg=bg, ctx=ctx)
        want = ndimage.minimum_filter(x > t, 3)
        assert got.dtype == np.uint8 and np.array_equal(got, want) and np.array_equal(got, ref.spot_mask(x, t))
        # the border keeps a spot that touches it; thin features vanish; x == t is not above t
        assert got[0, 0] == 1 and got[0, 4] == 0 and got[1, 1] == 0 and got[4, 0] == 0
        assert got[0, w - 1] == 1 and got[h - 1, 0] == 1 and got[h - 1, w - 1] == 1
        assert got[0, 32] == 1 and got[h - 1, 32] == 1 and got[9, 0] == 1 and got[9, w - 1] == 1 and got[9, 22] == 1
        assert not got[8, 40:60].any() and not got[12:14, 40:60].any() and got[16, 45] == 0
        assert got.sum() == want.sum() > 50
    d = ops.spot_mask(ctx.to_device(img), 50.0)
    assert d.dtype == np.uint8 and np.array_equal(d.get(), ref.spot_mask(img, 50.0))
    for shape in ((1, 1), (1, 9), (6, 1)):
        one = np.full(shape, 3, dtype)
        assert ops.spot_mask(one, 2.0, ctx=ctx).all() and not ops.spot_mask(one, 3.0, ctx=ctx).any()
    if np.dtype(dtype).kind == 'f':
        x = np.full((5, 6), 3, dtype)
        x[2, 2] = np.nan
        assert np.array_equal(ops.spot_mask(x, 2.0, ctx=ctx), ref.spot_mask(x, 2.0))


# ------------------------------------------------------------------ labelling
PATTERNS = {
    'false': lambda s: np.zeros(s, np.uint8),
    'true': lambda s: np.ones(s, np.uint8),
    'checker': sc.checkerboard,
    'spiral': sc.spiral,
    'u': sc.u_shape,
    'random30': lambda s: sc.random_field(s, 0.30, 30),
    'random50': lambda s: sc.random_field(s, 0.50, 50),
    'random62': lambda s: sc.random_field(s, 0.62, 62),
}


@pytest.mark.parametrize('conn', (1, 2))
@pytest.mark.parametrize('pattern', sorted(PATTERNS))
def test_label_patterns_at_every_shape(ctx, pattern, conn):
    ops = _ops()
    for shape in sc.LABEL_SHAPES:
        m = PATTERNS[pattern](shape)
        want, n_want = scipy_label(m, conn)
        labels, n, sizes = ops.label(m, conn, return_sizes=True, ctx=ctx)
        assert labels.dtype == np.int32 and n == n_want, (shape, n, n_want)
        assert np.array_equal(labels, want), shape
        assert sizes.dtype == np.int64 and np.array_equal(sizes, np.bincount(want.ravel(), minlength=n + 1)[1:])
        if pattern == 'checker' and min(shape) > 1:
            assert n == (1 if conn == 2 else (shape[0] * shape[1] + 1) // 2)
        if pattern in ('spiral', 'u', 'true'):
            assert n == 1 and labels[0, 0 if pattern != 'u' or shape[1] < 3 else 1] == 1


@pytest.mark.parametrize('conn', (1, 2))
def test_label_equals_the_stored_skimage_and_scipy_labels(ctx, g, conn):
    ops = _ops()
    for name, m in sc.golden_patterns().items():
        labels, n = ops.label(m.astype(bool), conn, ctx=ctx)
        assert n == int(g['label_%s_c%d_n' % (name, conn)]), name
        assert np.array_equal(labels, g['label_%s_c%d' % (name, conn)]), name
        ref_labels, ref_n = ref.label(m, conn)
        assert n == ref_n and np.array_equal(labels, ref_labels)
        if name.startswith('diag'):
            assert n == (1 if conn == 2 else 2)       # joined only by a diagonal across a tile corner


def test_label_device_arrays_and_pitched_masks(ctx):
    ops = _ops()
    from imgprocessor_amd import DeviceArray
    m = sc.random_field((2 * sc.TILE_H + 3, 2 * sc.TILE_W + 5), 0.55, 8)
    h, w = m.shape
    d_labels, n = ops.label(ctx.to_device(m), 2)
    want, n_want = scipy_label(m, 2)
    assert isinstance(d_labels, DeviceArray) and d_labels.dtype == np.int32
    assert n == n_want and np.array_equal(d_labels.get(), want)
    for conn in (1, 2):
        # a set padding would join components if it were read; the labels' padding keeps its guard
        d_mask = ctx.to_device(padded(m, w + 3, 1))
        d_out = DeviceArray.counts(ctx, (h, w + 6))
        d_out.set(np.full((h, w + 6), IGUARD, np.int32))
        cnt = C.c_int(-1)
        assert ctx._lib.ipa_label_dev(ctx.handle, d_mask.ptr, h, w, w + 3, conn, d_out.ptr, w + 6, C.byref(cnt)) == 0
        got = d_out.get()
        want, n_want = scipy_label(m, conn)
        assert (got[:, w:] == IGUARD).all() and cnt.value == n_want and np.array_equal(got[:, :w], want)
        big = (C.c_longlong * 4)()
        assert ctx._lib.ipa_label_largest_dev(ctx.handle, d_out.ptr, h, w, w + 6, cnt.value, big) == 0
        k, size, (sy, sx) = ref.largest(want, n_want)
        assert list(big) == [k, size, sy, sx]
    assert ctx._lib.ipa_label_dev(ctx.handle, d_mask.ptr, h, w, w + 3, 3, d_out.ptr, w + 6, C.byref(cnt)) == -1


# ------------------------------------------------------------------ sizes, largest component
def test_largest_component(ctx):
    ops = _ops()
    m = np.zeros((2 * sc.TILE_H + 1, 2 * sc.TILE_W + 9), np.uint8)
    m[0:2, 70:73] = 1          # 6 pixels, first in raster order, across no seam
    m[14:17, 62:64] = 1        # 6 pixels across a horizontal seam
    m[30, 5:10] = 1            # 5 pixels
    labels, n, sizes = ops.label(m, 2, return_sizes=True, ctx=ctx)
    assert n == 3 and sizes.tolist() == [6, 6, 5]
    assert ops.largest_component(labels, n, ctx=ctx) == (1, 6, (3, 6 * 71)) == ref.largest(labels, n)
    assert ops.largest_component(m, ctx=ctx) == (1, 6, (3, 6 * 71))            # a mask is labelled first
    assert ops.largest_component(ctx.to_device(m)) == (1, 6, (3, 6 * 71))
    m[14:17, 61] = 1           # now the second one is larger
    assert ops.largest_component(m.astype(bool), ctx=ctx) == (2, 9, (3 * 45, 3 * (61 + 62 + 63)))
    assert ops.largest_component(np.zeros((5, 7), np.uint8), ctx=ctx) is None
    assert ops.largest_component(np.zeros((5, 7), np.int32), 0, ctx=ctx) is None
    for d, conn in ((0.3, 1), (0.5, 2), (0.62, 2), (0.62, 1)):
        m = sc.random_field((3 * sc.TILE_H + 2, 3 * sc.TILE_W + 1), d, 77)
        want, n_want = scipy_label(m, conn)
        labels, n, sizes = ops.label(m, conn, return_sizes=True, ctx=ctx)
        assert n == n_want and np.array_equal(sizes, np.bincount(want.ravel(), minlength=n + 1)[1:])
        assert ops.largest_component(labels, n, ctx=ctx) == ref.largest(want, n_want)
        assert ops.largest_component(m, connectivity=conn, ctx=ctx) == ref.largest(want, n_want)


def test_a_frame_filling_component(ctx):
    """2.2 M pixels, one component around two holes and two small ones inside them: every grid-stride loop
    takes more than one trip, and the sizes are wave sums, not one add per pixel"""
    ops = _ops()
    h, w = 1100, 2003
    m = np.ones((h, w), np.uint8)
    m[100:200, 300:900] = 0
    m[140:150, 500:520] = 1
    m[700:900, 1000:1900] = 0
    m[800, 1500] = 1
    labels, n, sizes = ops.label(ctx.to_device(m), 1, return_sizes=True)
    want, n_want = scipy_label(m, 1)
    assert n == n_want == 3 and np.array_equal(labels.get(), want)
    assert sizes.tolist() == [h * w - 100 * 600 - 200 * 900, 200, 1]
    k, size, (sy, sx) = ops.largest_component(labels, n)
    yy, xx = np.nonzero(want == 1)
    assert (k, size, sy, sx) == (1, int(sizes[0]), int(yy.sum()), int(xx.sum()))


# ------------------------------------------------------------------ take
def sum_bound(values):
    """the error bound of any order of summation: count * 2**-53 * sum|x|"""
    v = np.asarray(values, np.float64).ravel()
    return v.size * 2.0 ** -53 * math.fsum(np.abs(v))


@pytest.mark.parametrize('dtype', sc.ALL_DTYPES, ids=lambda d: np.dtype(d).name)
def test_spot_take(ctx, dtype):
    ops, rng = _ops(), np.random.default_rng(5)
    h, w = 2 * sc.TILE_H + 3, 4 * 256 + 9
    img = frame_of(rng, (h, w), dtype)
    m = np.zeros((h, w), np.uint8)
    m[3:30, 100:900] = 1
    m[10, 300] = 0
    m[0:2, 0:2] = 1
    labels, n = ref.label(m)
    for kind, bg in backgrounds(rng, (h, w)).items():
        x = minus(img, bg)
        # the spot form
        sel = labels == 2
        fit, mask, mx, total, count = ops.spot_take(img, labels, 2, bg=bg, ctx=ctx)
        assert same(fit, np.where(sel, x, 0.0)) and same(mask, sel.astype(np.uint8))
        assert mx == x[sel].max() and count == sel.sum()
        exact = math.fsum(x[sel])
        print('%s %s: sum error %.3e, bound %.3e' % (np.dtype(dtype).name, kind, abs(total - exact), sum_bound(x[sel])))
        assert abs(total - exact) <= sum_bound(x[sel])
        again = ops.spot_take(img, labels, 2, bg=bg, ctx=ctx)
        assert again[2:] == (mx, total, count) and same(again[0], fit)          # identical bits
        # the row form, into the same arrays on the device
        d_fit, d_mask = ctx.to_device(fit), ctx.to_device(mask)
        out = ops.spot_take(ctx.to_device(img), rows=(h - 1, 5), bg=bg, fit=d_fit, mask=d_mask)
        assert out[0] is d_fit and out[1] is d_mask
        rows = np.array([h - 1, 5])
        want_fit, want_mask = np.where(sel, x, 0.0), sel.astype(np.uint8)
        want_fit[rows], want_mask[rows] = x[rows], 1
        assert same(d_fit.get(), want_fit) and same(d_mask.get(), want_mask)
        assert out[2] == x[rows].max() and out[4] == 2 * w and abs(out[3] - math.fsum(x[rows].ravel())) <= sum_bound(x[rows])
        one = ops.spot_take(img, rows=(7, 7), bg=bg, ctx=ctx)
        assert one[2] == x[7].max() and one[4] == w and same(one[1], (np.arange(h) == 7)[:, None] * np.ones(w, np.uint8))
    nothing = ops.spot_take(img, labels, 3, ctx=ctx)
    assert nothing[2:] == (-np.inf, 0.0, 0) and not nothing[0].any() and not nothing[1].any()
    with pytest.raises(IndexError):
        ops.spot_take(img, rows=(0, h), ctx=ctx)
    if np.dtype(dtype).kind == 'f':
        x = img.copy()
        x[10, 200] = np.nan
        assert np.isnan(ops.spot_take(x, rows=(10, 11), ctx=ctx)[2])            # np.max's answer


def test_spot_take_pitched_through_the_abi(ctx):
    from imgprocessor_amd import DeviceArray
    rng = np.random.default_rng(6)
    h, w = 9, 300
    img = frame_of(rng, (h, w), np.float32)
    bg = rng.uniform(0, 5, (h, w))
    x = minus(img, bg)
    labels = np.zeros((h, w), np.int32)
    labels[2:7, 250:] = 4
    keep, args = src_args(ctx, img, bg)
    d_labels = DeviceArray.counts(ctx, (h, w + 1))
    d_labels.set(padded(labels, w + 1, 4))
    d_fit = ctx.to_device(np.full((h, w + 4), GUARD))
    d_mask = ctx.to_device(np.full((h, w + 7), 9, np.uint8))
    r = (C.c_double * 3)()
    assert ctx._lib.ipa_spot_take_dev(*(args + (d_labels.ptr, w + 1, 4, 0, 0, d_fit.ptr, w + 4, d_mask.ptr, w + 7,
                                                r))) == 0
    sel = labels == 4
    assert same(d_fit.get(), np.where(padded(sel, w + 4, False), padded(x, w + 4, 0.0), GUARD))
    assert same(d_mask.get(), np.where(padded(sel, w + 7, False), 1, 9).astype(np.uint8))
    assert r[0] == x[sel].max() and r[2] == sel.sum() and abs(r[1] - math.fsum(x[sel])) <= sum_bound(x[sel])
    # the refusals: label 0, a row beyond the frame, an output that overlaps the frame
    assert ctx._lib.ipa_spot_take_dev(*(args + (d_labels.ptr, w + 1, 0, 0, 0, d_fit.ptr, w + 4, d_mask.ptr, w + 7,
                                                r))) == -1
    assert ctx._lib.ipa_spot_take_dev(*(args + (None, 0, 0, 0, h, d_fit.ptr, w + 4, d_mask.ptr, w + 7, r))) == -1
    assert ctx._lib.ipa_spot_take_dev(*(args + (None, 0, 0, 0, 1, d_fit.ptr, w + 4, keep[0].ptr, w + 7, r))) == -1


# ------------------------------------------------------------------ the whole routine
def V():
    from imgprocessor_amd.camera.flatField import vignettingFromSpotAverage
    return vignettingFromSpotAverage


def ulps(a, b):
    """the distance in units of the last place of b, elementwise; 0 where both are NaN"""
    a, b = np.asarray(a, np.float64), np.asarray(b, np.float64)
    both_nan = np.isnan(a) & np.isnan(b)
    with np.errstate(invalid='ignore'):
        d = np.abs(a - b) / np.spacing(np.abs(b))
    return np.where(both_nan | (a == b), 0.0, d)


def live_device_arrays():
    from imgprocessor_amd import DeviceArray
    gc.collect()
    return sum(isinstance(o, DeviceArray) for o in gc.get_objects())


@pytest.mark.parametrize('dev', (False, True), ids=('host', 'device'))
@pytest.mark.parametrize('name', sorted(SCENES))
def test_the_routine_on_the_fixtures_scenes(ctx, g, capsys, name, dev):
    from imgprocessor_amd import DeviceArray
    scene = SCENES[name]
    up = ctx.to_device if dev else (lambda a: a.copy())
    images = [up(f) for f in scene['images']]
    bg = scene['bg'] if np.ndim(scene['bg']) == 0 else [up(b) for b in scene['bg']]
    kw = dict(averageSpot=scene['averageSpot'], thresh=scene['thresh'])
    if scene['raises'] is not None:
        before = live_device_arrays()
        with pytest.raises(scene['raises']):
            V()(images, bg, **kw)
        assert live_device_arrays() == before, 'the refused call left device arrays behind'
        assert capsys.readouterr().out == str(g[name + '_printed'])
        return
    fitimg, mask = V()(images, bg, **kw)
    assert capsys.readouterr().out == str(g[name + '_printed'])
    if dev:
        assert isinstance(fitimg, DeviceArray) and isinstance(mask, DeviceArray) and mask.dtype == np.uint8
        fitimg, mask = fitimg.get(), mask.get().astype(bool)
    assert fitimg.dtype == np.float64 and mask.dtype == bool
    assert np.array_equal(mask, g[name + '_mask'])
    if scene['averageSpot']:
        assert same(fitimg, g[name + '_fitimg'])
    else:
        # one differing sum, then one division
        worst = ulps(fitimg, g[name + '_fitimg']).max()
        print('%s: fitimg differs from the fixture by at most %.2f ulp' % (name, worst))
        assert worst <= 4


@pytest.mark.parametrize('name', [n for n in sorted(SCENES) if not SCENES[n]['averageSpot']])
def test_the_spot_means_and_mx(ctx, g, name):
    """the routine's per-frame steps through ops: thresholds, label images, counts and the chosen
    labels bit for bit; each spot mean = device sum / count lies within the bound of any summation
    order, carried through the one division, of the exactly rounded mean - and so does mx"""
    ops = _ops()
    scene = SCENES[name]
    bg = ref.background(scene['bg'])
    means, bounds = [], []
    for k, im in enumerate(scene['images']):
        x = ref.frame(im, bg)
        t = ops.otsu_threshold(im, bg=bg, ctx=ctx) if scene['thresh'] is None else scene['thresh']
        assert t == g[name + '_t'][k]
        if scene['thresh'] is None and x.min() != x.max():
            assert np.array_equal(ops.histogram(im, 256, bg=bg, ctx=ctx)[0], g[name + '_counts'][k])
        spots, n, sizes = ops.label(ops.spot_mask(im, t, bg=bg, ctx=ctx), return_sizes=True, ctx=ctx)
        assert n == g[name + '_n'][k] and np.array_equal(spots, g[name + '_spots'][k])
        assert np.array_equal(sizes, g[name + '_sizes'][k][:n])
        big = ops.largest_component(spots, n, ctx=ctx)
        assert (0 if big is None else big[0]) == g[name + '_label'][k]
        if big is None:
            continue
        total, count = ops.spot_take(im, spots, big[0], bg=bg, ctx=ctx)[3:]
        v = x[spots == big[0]]
        exact = math.fsum(v) / count
        err, bound = abs(total / count - exact), sum_bound(v) / count + 2.0 ** -53 * abs(exact)
        print('%s frame %d: mean error %.3e, bound %.3e' % (name, k, err, bound))
        assert err <= bound and abs(g[name + '_mx2'][k] - exact) <= bound
        means.append(total / count)
        bounds.append(bound)
    if means:
        # the same frame supplies mx, and the device's and numpy's mean of it each lie within its bound
        top = int(np.argmax(means))
        assert top == np.argmax(g[name + '_mx2'][g[name + '_label'] != 0])
        assert abs(means[top] - float(g[name + '_mx'])) <= 2 * bounds[top]
