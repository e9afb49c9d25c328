"""GPU: flat field calibration (csrc/flat.hip, camera/flatField/flatFieldFromCloseDistance.py,
camera/flatField/sensitivity.py) against the numpy restatement (tests/flat_ref.py), bit for bit, and
the reference's outputs (tests/golden/flat.npz).

The kernels run through the C ABI - rows with a pitch, guard-valued padding that must come back
untouched - and through ops, at the shapes where they can go wrong: one pixel, a pitched odd width,
more than one tile in both directions, rows aligned and not aligned for the multi-pixel lanes of
the stack mean; stacks of 1, 2, 5, 64 and 65 frames; all four element types; NaN and +-inf; a grid
of more than one workgroup of partial extrema; whole-block and fractional shrink factors.

Against the fixture: scene (a) is equal bit for bit; scene (b) - whose noise level function is
fitted on the host - is equal on the pixels the fixture's stable-decision mask covers, with the
reference's sort order.
"""
import ctypes as C

import numpy as np
import pytest

from .conftest import load_golden
from . import dark_cases as dc
from . import dark_ref
from . import flat_cases as fc
from . import flat_ref as ref
from .test_cpu_dark import same
from .test_cpu_flat import SUB
from .test_gpu_dark import DT_ID, ERR_BAD_ARG, ERR_UNSUPPORTED, GUARD, KINDS, dptr, padded, pitch_of, planes, unpad

pytestmark = pytest.mark.gpu

U8_GUARD = 77


@pytest.fixture(scope='module')
def ctx():
    import imgprocessor_amd
    return imgprocessor_amd.default_context(0)


@pytest.fixture(scope='module')
def g():
    return load_golden('flat.npz')


@pytest.fixture(scope='module')
def FF():
    from imgprocessor_amd.camera import flatField
    return flatField


def _ops():
    from imgprocessor_amd import ops
    return ops


def bg_args(ctx, bg, h, w, pitch):
    """a background as the C ABI takes it -> (device array kept alive, pointer, pitch, scalar)"""
    if bg is None or np.ndim(bg) == 0:
        return None, None, 0, 0.0 if bg is None else float(bg)
    d = ctx.to_device(padded(np.asarray(bg, np.float64), pitch, GUARD))
    return d, d.ptr, pitch, 0.0


# ------------------------------------------------------------------ stack_mean
@pytest.mark.parametrize('n', fc.MEAN_N)
def test_stack_mean(ctx, n):
    ops = _ops()
    for si, (h, w) in enumerate(dc.REGRESS_SHAPES):
        pitch = pitch_of(w)
        # (3, 67) and (5, 520): rows, frames and the result aligned for the lanes that own 4 or 2
        # adjacent pixels - one tile with a partial last lane, and three (uint8, uint16) or five
        # (float32) tiles along a row; the other shapes run one pixel per lane
        opitch = pitch + (4 if w in (67, 520) else 1)
        for di, dt in enumerate(dc.ALL_DTYPES):
            st = fc.stack(n, h, w, dt, 100 * n + 10 * si + di)
            want = ref.stack_mean(list(st))
            for gap in (0, 2):   # frames h * pitch apart, and further
                host = np.concatenate([padded(st, pitch), np.zeros((n, gap, pitch), st.dtype)], axis=1)
                d_out, = planes(ctx, 1, h, opitch)
                d_st = ctx.to_device(host)
                ctx._check(ctx._lib.ipa_stack_mean_dev(ctx.handle, d_st.ptr, DT_ID[st.dtype], n, h, w, pitch,
                                                       (h + gap) * pitch, d_out.ptr, opitch), 'stack_mean')
                assert same(unpad(d_out, w), want), (n, (h, w), dt, gap)
            assert same(ops.stack_mean(st), want) and same(ops.stack_mean(list(st)), want)
            d = ops.stack_mean(ctx.to_device(st))
            assert d.dtype == np.float64 and same(d.get(), want)


def test_stack_mean_colour_and_refusals(ctx):
    ops = _ops()
    for di, dt in enumerate(dc.ALL_DTYPES):
        st = fc.stack(5, 7, 3 * 11, dt, 900 + di).reshape(5, 7, 11, 3)
        want = ref.stack_mean(list(st))
        assert same(ops.stack_mean(st), want) and same(ops.stack_mean(list(st)), want)
        d = ops.stack_mean(ctx.to_device(st))
        assert d.shape == (7, 11, 3) and same(d.get(), want)
        d = ops.stack_mean([ctx.to_device(f) for f in st])      # a list of device colour frames
        assert d.shape == (7, 11, 3) and same(d.get(), want)
    d_st, (d_out,) = ctx.to_device(np.zeros((2, 4, 8), np.uint16)), planes(ctx, 1, 4, 8)
    call = ctx._lib.ipa_stack_mean_dev
    assert call(ctx.handle, d_st.ptr, 1, 0, 4, 8, 8, 32, d_out.ptr, 8) == ERR_BAD_ARG       # no frames
    assert call(ctx.handle, d_st.ptr, 1, 2, 4, 8, 7, 32, d_out.ptr, 8) == ERR_BAD_ARG       # pitch < w
    assert call(ctx.handle, d_st.ptr, 1, 2, 4, 8, 8, 16, d_out.ptr, 8) == ERR_BAD_ARG       # frames overlap
    assert call(ctx.handle, d_st.ptr, 7, 2, 4, 8, 8, 32, d_out.ptr, 8) == ERR_UNSUPPORTED   # dtype
    assert np.all(d_out.get() == GUARD)


# ------------------------------------------------------------------ luma
@pytest.mark.parametrize('shape', dc.SHAPES)
def test_luma(ctx, shape):
    ops = _ops()
    h, w = shape
    img = np.random.default_rng(31).uniform(-5.0, 3000.0, (h, w, 3))
    if h * w > 8:
        img[0, 1, 2], img[0, 2, 0], img[1, 3, 1] = np.nan, np.inf, -np.inf
    want = ref.luma(img)
    assert same(want, np.average(img, axis=-1, weights=ref.LUMA_WEIGHTS))
    pitch, opitch = 3 * w + 2, pitch_of(w) + 1
    d_img = ctx.to_device(padded(img.reshape(h, 3 * w), pitch, GUARD))
    d_out, = planes(ctx, 1, h, opitch)
    wgt = np.array(ref.LUMA_WEIGHTS)
    ctx._check(ctx._lib.ipa_luma_dev(ctx.handle, d_img.ptr, h, w, pitch, dptr(wgt), float(wgt.sum()), d_out.ptr,
                                     opitch), 'luma')
    assert same(unpad(d_out, w), want)
    assert same(ops.luma(img), want)
    d = ops.luma(ctx.to_device(img))
    assert d.shape == (h, w) and same(d.get(), want)
    assert ctx._lib.ipa_luma_dev(ctx.handle, d_img.ptr, h, w, 3 * w - 1, dptr(wgt), 1.0, d_out.ptr,
                                 opitch) == ERR_BAD_ARG


# ------------------------------------------------------------------ strided extremum
def extremum_abi(ctx, a, sy, sx, mode, pitch=None):
    h, w = a.shape
    pitch = pitch or pitch_of(w)
    fill = GUARD if a.dtype.kind == 'f' else U8_GUARD
    d = ctx.to_device(padded(a, pitch, fill))
    r = C.c_double(-1.0)
    rc = ctx._lib.ipa_strided_extremum_dev(ctx.handle, d.ptr, DT_ID[a.dtype], h, w, pitch, sy, sx, mode,
                                           C.byref(r))
    return rc, r.value


# (shape, step): one pixel, a pitched odd width, several tiles, a 5 x 257 grid - more than one
# workgroup of partial maxima -, and step 1
MEDIAN_CASES = [((1, 1), 10), ((3, 67), 10), ((33, 130), 10), ((41, 2570), 10), ((5, 7), 1)]


@pytest.mark.parametrize('shape,step', MEDIAN_CASES)
def test_strided_median_max(ctx, shape, step):
    ops = _ops()
    a = np.random.default_rng(41).uniform(0.0, 100.0, shape)
    gh, gw = -(-shape[0] // step), -(-shape[1] // step)
    # the maximum where the random field has it, then planted: at the first and at the last grid
    # point (a corner's window repeats its samples) and on a reflected edge
    plants = [()]
    if gh >= 2 and gw >= 3:
        plants += [((0, 0), (0, 1)), ((gh - 1, gw - 1), (gh - 1, gw - 2)),
                   ((0, gw // 2), (0, gw // 2 + 1), (1, gw // 2))]
    for k, pts in enumerate(plants):
        b = a.copy()
        for j, (gy, gx) in enumerate(pts):
            b[gy * step, gx * step] = 500.0 + 100.0 * k + j
        want = ref.strided_median_max(b, step)
        assert (want > 500.0) == bool(pts)
        rc, got = extremum_abi(ctx, b, step, step, 0)
        assert rc == 0 and got == want, (shape, step, pts)
        assert ops.strided_median_max(b, step) == want
        assert ops.strided_median_max(ctx.to_device(b), step) == want
    if a.size > 4:   # a NaN in a window is the maximum, as numpy's max has it
        b = a.copy()
        b[0, 0] = np.nan
        assert np.isnan(extremum_abi(ctx, b, step, step, 0)[1])


def test_strided_min_and_the_sort_key(ctx):
    ops = _ops()
    for si, (h, w) in enumerate([(1, 1), (3, 67), (33, 130), (41, 2570), (60, 80)]):
        for di, dt in enumerate(dc.ALL_DTYPES):
            a = fc.frame(h, w, dt, 50 + 10 * si + di, special=False)
            a = np.maximum(a, 3).astype(dt)
            for sy, sx in ((1, 1), (max(h // 10, 1), max(w // 10, 1)), (7, 3)):
                b = a.copy()
                b[(h - 1) // sy * sy, (w - 1) // sx * sx] = 2     # the minimum on the last grid point
                want = ref.strided_min(b, sy, sx)
                rc, got = extremum_abi(ctx, b, sy, sx, 1)
                assert rc == 0 and got == float(want) == 2.0, ((h, w), dt, sy, sx)
                got = ops.strided_min(b, sy, sx)
                assert got.dtype == b.dtype and got == want
                assert ops.strided_min(ctx.to_device(b), sy, sx) == want
            if h >= 10 and w >= 10:   # the key of the sort: the negation wraps for unsigned frames
                with np.errstate(over='ignore'):
                    key = np.negative(ops.strided_min(a, h // 10, w // 10))
                assert key.dtype == a.dtype and key == ref.sort_key(a)
                assert (key > 0) == (a.dtype.kind == 'u')
    a = np.array([[3.0, np.nan], [1.0, 2.0]], np.float32)
    assert np.isnan(ops.strided_min(a, 1, 1)) and ops.strided_min(a, 1, 2) == 1.0
    d = ctx.to_device(np.zeros((4, 4), np.float32))
    r = C.c_double()
    call = ctx._lib.ipa_strided_extremum_dev
    assert call(ctx.handle, d.ptr, 2, 4, 4, 4, 0, 1, 1, C.byref(r)) == ERR_BAD_ARG          # step 0
    assert call(ctx.handle, d.ptr, 2, 4, 4, 4, 1, 1, 2, C.byref(r)) == ERR_BAD_ARG          # mode
    assert call(ctx.handle, d.ptr, 2, 4, 4, 4, 1, 1, 0, C.byref(r)) == ERR_UNSUPPORTED      # median of float32


# ------------------------------------------------------------------ flat_scale
@pytest.mark.parametrize('shape', dc.SHAPES)
def test_flat_scale(ctx, shape):
    ops = _ops()
    h, w = shape
    pitch = pitch_of(w)
    img = fc.frame(h, w, np.float64, 61)
    bg_frame = fc.frame(h, w, np.float64, 62)
    if h * w > 8:
        bg_frame.ravel()[3] = np.inf      # inf - inf
    for bg in (None, 7.25, bg_frame):
        for div in (None, 3.7, 0.0):
            if bg is None and div is None:
                continue
            want = ref.flat_scale(img, bg, div)
            d_img = ctx.to_device(padded(img, pitch, GUARD))
            keep, bgp, bg_pitch, bgv = bg_args(ctx, bg, h, w, pitch + 2)
            d_out, = planes(ctx, 1, h, pitch + 1)
            args = (bgp, bg_pitch, bgv, int(bg is not None), 1.0 if div is None else div, int(div is not None))
            ctx._check(ctx._lib.ipa_flat_scale_dev(ctx.handle, d_img.ptr, h, w, pitch, *args, d_out.ptr, pitch + 1),
                       'flat_scale')
            assert same(unpad(d_out, w), want), (shape, np.ndim(bg), div)
            # in place
            ctx._check(ctx._lib.ipa_flat_scale_dev(ctx.handle, d_img.ptr, h, w, pitch, *args, d_img.ptr, pitch),
                       'flat_scale')
            assert same(unpad(d_img, w), want)
            assert same(ops.flat_scale(img, bg, div), want)
            d = ctx.to_device(img)
            assert ops.flat_scale(d, bg, div, out=d) is d and same(d.get(), want)
    # a result that overlaps the image without being it is refused (one pixel cannot)
    if w > 1:
        d_img = ctx.to_device(np.full((h + 1, pitch), GUARD))
        assert ctx._lib.ipa_flat_scale_dev(ctx.handle, d_img.ptr, h, w, pitch, None, 0, 0.0, 1, 1.0, 0,
                                           C.c_void_p(d_img.ptr.value + 8), pitch) == ERR_BAD_ARG
        assert np.all(d_img.get() == GUARD)


# ------------------------------------------------------------------ nlf_lower_mask
class _Fn(object):
    """a noise level function that carries its parameters as camera/NoiseLevelFunction's do"""

    def __init__(self, kind, params):
        setattr(self, ('triple', 'poly', 'constant')[kind], params if kind != 2 else params[0])
        self.kind, self.params = kind, params

    def __call__(self, x):
        return dark_ref.nlf_threshold(x, self.kind, self.params, 1.0)


@pytest.mark.parametrize('shape', dc.SHAPES)
def test_nlf_lower_mask(ctx, shape):
    ops = _ops()
    h, w = shape
    pitch = pitch_of(w)
    rng = np.random.default_rng(71)
    avg = rng.uniform(0.0, 200.0, (h, w))
    for kind, params in KINDS:
        for nstd in (6.0, 2.5):
            with np.errstate(invalid='ignore'):
                thr = avg - dark_ref.nlf_threshold(avg, kind, params, nstd)
            for dt in dc.ALL_DTYPES:
                # values around the threshold, exactly on it (every third pixel, where the type
                # holds the value), NaN in the frame and in the average
                f = thr + rng.choice([-1.0, 0.0, 1.0], (h, w)) * rng.uniform(0.0, 5.0, (h, w))
                f.ravel()[::3] = thr.ravel()[::3]
                a = avg.copy()
                if np.dtype(dt).kind == 'f':
                    f = f.astype(dt)
                    if h * w > 8:
                        f.ravel()[1] = np.nan
                        a.ravel()[2] = np.nan
                        f.ravel()[4] = np.inf
                else:
                    f = np.clip(np.round(f), 0, 255).astype(dt)
                want = ref.nlf_lower_mask(f, a, kind, params, nstd)
                if np.dtype(dt) == np.float64:
                    on = np.zeros(h * w, bool)
                    on[::3] = True
                    on &= ~np.isnan(f.ravel()) & ~np.isnan(a.ravel()) & ~np.isinf(f.ravel())
                    assert not want.ravel()[on].any()      # on the threshold is not above it
                d_f = ctx.to_device(padded(f, pitch))
                d_a = ctx.to_device(padded(a, pitch + 1, GUARD))
                d_m = ctx.to_device(np.full((h, pitch + 3), U8_GUARD, np.uint8))
                p = np.array(params, dtype=np.float64)
                ctx._check(ctx._lib.ipa_nlf_lower_mask_dev(ctx.handle, d_f.ptr, DT_ID[np.dtype(dt)], h, w, pitch,
                                                           d_a.ptr, pitch + 1, kind, dptr(p), nstd, d_m.ptr,
                                                           pitch + 3), 'nlf_lower_mask')
                m = d_m.get()
                assert np.all(m[:, w:] == U8_GUARD), 'the padding was written'
                assert np.array_equal(m[:, :w], want.astype(np.uint8)), (shape, kind, nstd, dt)
                fn = _Fn(kind, params)
                got = ops.nlf_lower_mask(f, a, fn, nstd)
                assert got.dtype == bool and np.array_equal(got, want)
                d = ops.nlf_lower_mask(ctx.to_device(f), ctx.to_device(a), fn, nstd)
                assert d.dtype == np.uint8 and np.array_equal(d.get(), want.astype(np.uint8))
    d_m = ctx.to_device(np.full((h, pitch), U8_GUARD, np.uint8))
    p = np.zeros(5)
    for kind in (-1, 3):
        assert ctx._lib.ipa_nlf_lower_mask_dev(ctx.handle, d_a.ptr, 3, h, w, pitch + 1, d_a.ptr, pitch + 1, kind,
                                               dptr(p), 3.0, d_m.ptr, pitch) == ERR_BAD_ARG
    assert np.all(d_m.get() == U8_GUARD)


# ------------------------------------------------------------------ sensitivity
# (shape, f): whole blocks - one fused kernel -, and fractional scales on both axes - the median
# frame through the workspace and the area tables
SENS_CASES = [((20, 30), 10), ((16, 24), 4), ((35, 67), 10)]


def composed(ctx, frames, bg, f):
    """sensitivity from the ops that were there before: nlf_signal -> fastMean on the device, the
    division and the sum on the host"""
    from imgprocessor_amd.filters.fastMean import fastMean
    ops = _ops()
    out = None
    d_bg = bg if bg is None or np.ndim(bg) == 0 else ctx.to_device(bg)
    for frame in frames:
        smooth = fastMean(ops.nlf_signal(ctx.to_device(frame), bg=d_bg), f).get()
        with np.errstate(invalid='ignore', divide='ignore'):
            q = ref.sens_signal(frame, bg) / smooth
        out = q if out is None else out + q
    return out / len(frames)


@pytest.mark.parametrize('shape,f', SENS_CASES)
def test_sens_kernels(ctx, shape, f):
    ops = _ops()
    h, w = shape
    pitch = pitch_of(w)
    dh, dw = ref.small_shape(shape, f)
    bg_frame = 20.0 + fc.frame(h, w, np.float64, 81, special=False) * 0.01
    for di, dt in enumerate(dc.ALL_DTYPES):
        frames = [fc.smooth_frame(h, w, dt, 82 + 10 * di + k) for k in range(3)]
        for bg in (None, 12.5, bg_frame):
            keep, bgp, bg_pitch, bgv = bg_args(ctx, bg, h, w, pitch + 2)
            d_acc, = planes(ctx, 1, h, pitch + 1)
            for n in (1, 3):
                for k in range(n):
                    want_small = ref.sens_shrink(frames[k], bg, f)
                    d_f = ctx.to_device(padded(frames[k], pitch))
                    d_small, = planes(ctx, 1, dh, dw + 3)
                    ctx._check(ctx._lib.ipa_sens_shrink_dev(ctx.handle, d_f.ptr, DT_ID[np.dtype(dt)], h, w, pitch, bgp,
                                                            bg_pitch, bgv, dh, dw, d_small.ptr, dw + 3), 'sens_shrink')
                    assert same(unpad(d_small, dw), want_small), (shape, f, dt, np.ndim(bg))
                    ctx._check(ctx._lib.ipa_sens_accumulate_dev(
                        ctx.handle, d_f.ptr, DT_ID[np.dtype(dt)], h, w, pitch, bgp, bg_pitch, bgv, d_small.ptr, dh, dw,
                        dw + 3, d_acc.ptr, pitch + 1, int(k == 0), n if k == n - 1 else 0), 'sens_accumulate')
                want = ref.sensitivity(frames[:n], bg, f)
                assert same(unpad(d_acc, w), want), (shape, f, dt, np.ndim(bg), n)
                assert same(want, composed(ctx, frames[:n], bg, f)), 'the composition of the merged ops differs'
            assert same(ops.sens_shrink(frames[0], bg, f), ref.sens_shrink(frames[0], bg, f))
            d = ops.sens_shrink(ctx.to_device(frames[0]), bg, f)
            assert d.shape == (dh, dw) and same(d.get(), ref.sens_shrink(frames[0], bg, f))


@pytest.mark.parametrize('shape,f', SENS_CASES)
def test_sens_special_values(ctx, FF, shape, f):
    """NaN, +inf and -inf in float frames: the median on the frame's own type (a scalar or no
    background) and the float64 one (a background frame) send them where the restatement and the
    merged ops do"""
    ops = _ops()
    h, w = shape
    bg_frame = 20.0 + fc.frame(h, w, np.float64, 85, special=False) * 0.01
    for di, dt in enumerate((np.float32, np.float64)):
        frames = [100.0 + fc.frame(h, w, dt, 86 + di), fc.smooth_frame(h, w, dt, 88 + di)]
        assert np.isnan(frames[0]).any() and np.isinf(frames[0]).sum() == 2
        for bg in (None, 12.5, bg_frame):
            want = ref.sens_shrink(frames[0], bg, f)
            assert np.isnan(want).any()
            assert same(ops.sens_shrink(frames[0], bg, f), want), (shape, dt, np.ndim(bg))
            want = ref.sensitivity(frames, bg, f)
            assert same(FF.sensitivity(frames, bg, f), want)
            assert same(want, composed(ctx, frames, bg, f))


def test_sens_refusals(ctx):
    d_f, (d_small, d_acc) = ctx.to_device(np.ones((20, 30), np.uint16)), planes(ctx, 2, 20, 30)
    shrink, acc = ctx._lib.ipa_sens_shrink_dev, ctx._lib.ipa_sens_accumulate_dev
    assert shrink(ctx.handle, d_f.ptr, 1, 20, 30, 30, None, 0, 0.0, 0, 3, d_small.ptr, 3) == ERR_BAD_ARG
    assert shrink(ctx.handle, d_f.ptr, 1, 20, 30, 30, None, 0, 0.0, 2, 3, d_small.ptr, 2) == ERR_BAD_ARG
    assert shrink(ctx.handle, d_f.ptr, 1, 20, 30, 30, None, 0, 0.0, 21, 3, d_small.ptr, 3) == ERR_UNSUPPORTED
    assert shrink(ctx.handle, d_f.ptr, 5, 20, 30, 30, None, 0, 0.0, 2, 3, d_small.ptr, 3) == ERR_UNSUPPORTED
    assert acc(ctx.handle, d_f.ptr, 1, 20, 30, 30, None, 0, 0.0, d_small.ptr, 2, 3, 3, d_acc.ptr, 29, 1,
               1) == ERR_BAD_ARG
    assert acc(ctx.handle, d_f.ptr, 1, 20, 30, 30, None, 0, 0.0, d_acc.ptr, 2, 3, 3, d_acc.ptr, 30, 1,
               1) == ERR_BAD_ARG                                                 # small inside the accumulator
    assert np.all(d_small.get() == GUARD) and np.all(d_acc.get() == GUARD)


# ------------------------------------------------------------------ the public functions
@pytest.mark.parametrize('shape,f', SENS_CASES)
def test_sensitivity(ctx, FF, shape, f):
    from imgprocessor_amd import DeviceArray
    h, w = shape
    frames = [fc.smooth_frame(h, w, np.uint16, 91 + k) for k in range(3)]
    bgs = [np.round(20.0 + fc.frame(h, w, np.float64, 95 + k, special=False) * 0.003).astype(np.uint16)
           for k in range(3)]
    for n in (1, 3):
        for bg in (None, bgs[0], bgs[:1]):
            b = None if bg is None else bgs[0].astype(np.float64)
            want = ref.sensitivity(frames[:n], b, f)
            got = FF.sensitivity(frames[:n], bg, f)
            assert isinstance(got, np.ndarray) and same(got, want), (shape, f, n)
            dev_bg = bg if bg is None else ctx.to_device(bgs[0])
            d = FF.sensitivity([ctx.to_device(fr) for fr in frames[:n]], dev_bg, f)
            assert isinstance(d, DeviceArray) and same(d.get(), want)
            d = FF.sensitivity(ctx.to_device(np.stack(frames[:n])), dev_bg, f)
            assert isinstance(d, DeviceArray) and same(d.get(), want)
    # several background frames: their single-time-effect-free average (DarkCurrentMap)
    from imgprocessor_amd.camera.DarkCurrentMap import averageSameExpTimes
    b = averageSameExpTimes(bgs)
    assert same(FF.sensitivity(frames, bgs, f), ref.sensitivity(frames, b, f))
    if f == 10:
        assert same(FF.sensitivity(frames), ref.sensitivity(frames, None, 10))   # the reference's signature


def test_img_average_and_backgrounds(ctx):
    from imgprocessor_amd import DeviceArray
    from imgprocessor_amd.transform import imgAverage
    from imgprocessor_amd.utils import getBackground, getBackground2
    for dt in dc.ALL_DTYPES:
        st = fc.stack(5, 33, 130, dt, 97)
        want = ref.stack_mean(list(st))
        assert same(imgAverage(list(st)), want) and same(imgAverage(st), want)
        d = imgAverage([ctx.to_device(f) for f in st])
        assert isinstance(d, DeviceArray) and same(d.get(), want)
        assert same(getBackground2(list(st)), want)
        assert same(getBackground2(ctx.to_device(st)).get(), want)
    frames = [f.astype(np.uint16) for f in fc.vignetting_scene()[1]]
    from imgprocessor_amd.camera.DarkCurrentMap import averageSameExpTimes
    assert same(getBackground(frames), averageSameExpTimes(frames))
    assert isinstance(getBackground(ctx.to_device(np.stack(frames))), DeviceArray)


def test_flat_field_1_equals_the_reference(ctx, FF, g):
    from imgprocessor_amd import DeviceArray
    for dtype in fc.ALL_DTYPES:
        frames, bgs = fc.colour_scene(dtype)
        p = 'a_%s_' % np.dtype(dtype).name
        got = FF.flatFieldFromCloseDistance(frames, bgs)
        assert isinstance(got, np.ndarray) and same(got, g[p + 'ff']), dtype
        assert same(FF.flatFieldFromCloseDistance(np.stack(frames), 9.5), g[p + 'ff_scalar_bg'])
        d = FF.flatFieldFromCloseDistance([ctx.to_device(f) for f in frames], [ctx.to_device(b) for b in bgs])
        assert isinstance(d, DeviceArray) and d.shape == fc.A_SHAPE[:2] and same(d.get(), g[p + 'ff'])
        d = FF.flatFieldFromCloseDistance(ctx.to_device(np.stack(frames)), 9.5)
        assert isinstance(d, DeviceArray) and same(d.get(), g[p + 'ff_scalar_bg'])
        # the documented extension: (h, w) frames skip the grey step
        grey, grey_bg = [f[..., 1].copy() for f in frames], [b[..., 1].copy() for b in bgs]
        assert same(FF.flatFieldFromCloseDistance(grey, grey_bg), ref.flat_field_1(grey, grey_bg))


def test_flat_field_2_equals_the_reference_on_the_stable_pixels(ctx, FF, g):
    from imgprocessor_amd import DeviceArray
    from imgprocessor_amd.camera.NoiseLevelFunction import BoundedNLF
    frames, bgs = fc.vignetting_scene()
    stable = g['b_stable']
    # the noise level function given: the reference's own parameters, every pixel is pinned
    tri = tuple(float(v) for v in g['b_nlf'])
    want, order = ref.flat_field_2(frames, bgs, dark_ref.NLF_BOUNDED_SQRT, tri, fc.B_NSTD)
    assert list(order) == list(g['b_order'])
    for nlf in (BoundedNLF(*tri), tri, lambda x: dark_ref.nlf_threshold(x, 0, tri, 1.0)):
        got = FF.flatFieldFromCloseDistance2(frames, bgs, nlf=nlf, nstd=fc.B_NSTD)
        assert isinstance(got, np.ndarray) and same(got, want)
    assert same(got[::SUB, ::SUB][stable], g['b_ff'][stable])
    # estimated here: the host fit differs in its last digits, the stable pixels do not
    got = FF.flatFieldFromCloseDistance2(frames, bgs)
    assert same(got[::SUB, ::SUB][stable], g['b_ff'][stable])
    d = FF.flatFieldFromCloseDistance2([ctx.to_device(f) for f in frames], ctx.to_device(np.stack(bgs)))
    assert isinstance(d, DeviceArray) and same(d.get()[::SUB, ::SUB][stable], g['b_ff'][stable])
    # a scalar background and the polynomial / constant functions, against the restatement
    for kind, params in ((dark_ref.NLF_CLIPPED_POLY, (1e-7, 0.005, 100.0, 5000.0, 30000.0)),
                         (dark_ref.NLF_CONSTANT, (250.0,))):
        want, _ = ref.flat_field_2(frames, 400.0, kind, params, 5)
        assert same(FF.flatFieldFromCloseDistance2(frames, 400.0, nlf=_Fn(kind, params), nstd=5), want), kind


def test_flat_field_feeds_camera_calibration(ctx, FF, capsys):
    from imgprocessor_amd.camera.CameraCalibration import CameraCalibration
    frames, bgs = fc.vignetting_scene()
    ff = FF.flatFieldFromCloseDistance2([ctx.to_device(f) for f in frames], [ctx.to_device(b) for b in bgs])
    cal = CameraCalibration()
    cal.addFlatField(ff.get(), date='03 Nov 15 - 10:00')
    raw = frames[2].astype(np.float64)
    out = cal.correct(raw, bgImages=[np.zeros(raw.shape)], threshold=0)
    capsys.readouterr()
    assert out.dtype == np.float64 and same(out, raw / ff.get())
