"""GPU: ops.nl_means (csrc/nlm.hip) against the float64 restatement tests/nlm_ref.py.

Tolerances, as fractions of the data range max|img|, set from the restatement's own arithmetic
error on the CPU over the fixture cases and the fresh 40 x 52 seeds below (pixels whose margin
min_t |D - 5| is under DELTA set aside, as here):
  float32 frames: nlm_ref run in float32 against the float64 restatement   1.73e-6  -> x 4
  float64 frames: nlm_ref run in float64 against the same in long double   2.67e-15 -> x 4
The factor 4 is headroom for the device exponential and the order of the sums.
Re-measured over the 24 cases of the geometry table (nlm_ref.GEO_CASES, patch sizes 3, 5, 9 and
11): 3.71e-7 and 7.61e-16, both under the figures above, which stay
(test_cpu_nlm.py::test_geometry_cases_denoise_and_stay_off_the_cut_off asserts it).
"""
import numpy as np
import pytest

from .conftest import load_golden, synth
from .gpu_helpers import same_bits
from . import nlm_ref as nr
from .nlm_ref import nlm_ref

pytestmark = pytest.mark.gpu

ERR32, ERR64 = 1.73e-6, 2.67e-15   # measured on the CPU (see above)
TOL = {np.float32: 4 * ERR32, np.float64: 4 * ERR64}
DELTA = 1e-4          # margin under which a rounding difference may switch a weight of exp(-5)
MAX_ASIDE = 0.02      # share of a case's pixels that may be set aside
ASIDE_TOL = 0.01      # of the data range, for the pixels set aside

G = load_golden('nlm.npz')
NAMES = [str(n) for n in G['names']]
_refs = {}


@pytest.fixture(scope='module')
def ctx():
    import imgprocessor_amd
    return imgprocessor_amd.default_context(0)


def ref_of(key, img, s, d, h, sigma=0.0):
    """float64 restatement of a case, computed once"""
    if key not in _refs:
        out, margin = nlm_ref(np.asarray(img, np.float64), s, d, h, sigma)
        out.setflags(write=False)
        margin.setflags(write=False)
        _refs[key] = (out, margin)
    return _refs[key]


def check(got, img, ref, margin, dtype, what):
    assert got.dtype == dtype and got.shape == ref.shape
    rng = float(np.abs(img).max())
    err = np.abs(got.astype(np.float64) - ref)
    aside = margin < DELTA
    worst = err[~aside].max() / rng
    worst_aside = err[aside].max() / rng if aside.any() else 0.0
    print('%s %s: %.2f %% set aside (worst %.2e), others worst %.2e of the range (tolerance %.2e)'
          % (what, np.dtype(dtype).name, 100 * aside.mean(), worst_aside, worst, TOL[dtype]))
    assert aside.mean() <= MAX_ASIDE, what
    assert worst_aside <= ASIDE_TOL, what
    assert worst <= TOL[dtype], what


def fixture_case(name):
    s, d, h, sigma = G[name + '_params']
    return G[name + '_img'], int(s), int(d), float(h), float(sigma)


@pytest.mark.parametrize('dtype', [np.float32, np.float64])
@pytest.mark.parametrize('name', NAMES)
def test_parity_fixture(ctx, name, dtype):
    from imgprocessor_amd import ops
    img, s, d, h, sigma = fixture_case(name)   # float32-exact values
    got = ops.nl_means(img.astype(dtype), s, d, h, sigma, ctx=ctx)
    check(got, img, G[name + '_ref'], G[name + '_margin'], dtype, name)


@pytest.mark.parametrize('dtype', [np.float32, np.float64])
@pytest.mark.parametrize('seed,d', [(11, 11), (12, 5)])
def test_parity_fresh_seed(ctx, seed, d, dtype):
    from imgprocessor_amd import ops
    img = synth((40, 52), seed, np.float32)
    ref, margin = ref_of(('seed', seed, d), img, 7, d, 0.1)
    got = ops.nl_means(img.astype(dtype), 7, d, 0.1, ctx=ctx)
    check(got, img, ref, margin, dtype, 'seed %d d %d' % (seed, d))


@pytest.mark.parametrize('dtype', [np.float32, np.float64])
def test_tiny_h_returns_the_input(ctx, dtype):
    """h = 1e-6: every distance is beyond the cut-off, only the self pair survives: 2 I / 2"""
    from imgprocessor_amd import ops
    img = synth((40, 52), 21, dtype)
    got = ops.nl_means(img, 7, 11, 1e-6, ctx=ctx)
    assert np.array_equal(got.view(np.uint8), img.view(np.uint8))


@pytest.mark.parametrize('dtype', [np.float32, np.float64])
def test_constant_image(ctx, dtype):
    from imgprocessor_amd import ops
    c = dtype(0.3)
    got = ops.nl_means(np.full((40, 52), c, dtype), ctx=ctx)
    assert np.abs(got - c).max() <= np.spacing(c)


@pytest.mark.parametrize('dtype', [np.float32, np.float64])
@pytest.mark.parametrize('shape,d', [((2, 2), 11), ((9, 50), 11), ((50, 3), 11), ((65, 129), 3),
                                     ((130, 70), 3), ((59, 64), 2), ((60, 65), 2)])
def test_geometry(ctx, shape, d, dtype):
    """pads larger than the image, tile edges of both kernels (59 columns x 64 / 32 rows at
    patch_size 7), more than one workgroup in both axes"""
    from imgprocessor_amd import ops
    img = synth(shape, 30 + shape[0], np.float32)
    ref, margin = ref_of(('geo', shape, d), img, 7, d, 0.1)
    got = ops.nl_means(img.astype(dtype), 7, d, 0.1, ctx=ctx)
    check(got, img, ref, margin, dtype, 'shape %s' % (shape,))


@pytest.mark.parametrize('dtype', [np.float32, np.float64])
def test_pitched_batch(ctx, dtype):
    """rows and frames of source and destination further apart than they are long: the same bits
    as the contiguous call, nothing written outside"""
    from imgprocessor_amd import ops
    from imgprocessor_amd.device import dtype_id
    n, h, w = 2, 37, 70
    src = np.stack([synth((h, w), 40 + i, dtype) for i in range(n)])
    want = ops.nl_means(ctx.to_device(src), 7, 4, 0.1).get()
    sp, dp = w + 9, w + 5
    sbig = np.full((n, h + 3, sp), 7.0, dtype)
    sbig[:, :h, :w] = src
    dbig = ctx.to_device(np.full((n, h + 2, dp), -5.0, dtype))
    ctx._check(ctx._lib.ipa_nl_means_dev(ctx.handle, ctx.to_device(sbig).ptr, dtype_id(dtype), n, h, w, sp,
                                         (h + 3) * sp, 7, 4, 0.1, 0.0, dbig.ptr, dp, (h + 2) * dp), 'nl_means')
    got = dbig.get()
    assert np.array_equal(got[:, :h, :w], want)
    assert (got[:, h:, :] == -5.0).all() and (got[:, :, w:] == -5.0).all(), 'wrote outside'


@pytest.mark.parametrize('dtype', [np.float32, np.float64])
def test_batch_equals_single_calls(ctx, dtype):
    from imgprocessor_amd import ops
    src = np.stack([synth((33, 61), 50 + i, np.float32) for i in range(3)]).astype(dtype)
    got = ops.nl_means(src, 7, 5, 0.1, ctx=ctx)
    assert got.shape == src.shape
    for i in range(3):
        one = ops.nl_means(src[i], 7, 5, 0.1, ctx=ctx)
        assert np.array_equal(got[i].view(np.uint8), one.view(np.uint8)), i
    ref, margin = ref_of(('batch', 1), src[1], 7, 5, 0.1)
    check(got[1], src[1], ref, margin, dtype, 'frame 1 of the batch')


def test_out_and_aliasing(ctx):
    from imgprocessor_amd import ops
    from imgprocessor_amd.device import dtype_id
    img = synth((20, 30), 60)
    d_img = ctx.to_device(img)
    d_out = ctx.empty((20, 30), np.float32)
    assert ops.nl_means(d_img, 5, 3, 0.1, out=d_out) is d_out
    assert np.array_equal(d_out.get(), ops.nl_means(img, 5, 3, 0.1, ctx=ctx))
    with pytest.raises(ValueError):
        ops.nl_means(d_img, out=d_img)
    with pytest.raises(ValueError):   # the C ABI: a destination that overlaps the source
        ctx._check(ctx._lib.ipa_nl_means_dev(ctx.handle, d_img.ptr, dtype_id(np.float32), 1, 20, 30, 30, 600,
                                             7, 3, 0.1, 0.0, d_img.ptr, 30, 600), 'nl_means')
    assert np.array_equal(d_img.get(), img)


def test_filter_wrapper(ctx):
    from imgprocessor_amd import ops
    from imgprocessor_amd.filters import denoiseNLMeans
    img = synth((20, 30), 61)
    got = denoiseNLMeans(img, patch_size=5, patch_distance=3, h=0.2)
    assert isinstance(got, np.ndarray)
    assert np.array_equal(got, ops.nl_means(img, 5, 3, 0.2, ctx=ctx))


def lds_bytes(dtype, s, d):
    """the bound stated in include/imgproc_hip.h"""
    rows = 64 if dtype == np.float32 else 32
    return (rows + s - 2 + 2 * d) * (64 + 2 * d) * np.dtype(dtype).itemsize


@pytest.mark.parametrize('dtype', [np.float32, np.float64])
def test_largest_documented_patch(ctx, dtype):
    """patch_size 11 with patch_distance 16 must run"""
    from imgprocessor_amd import ops
    img = synth((24, 30), 70, np.float32)
    ref, margin = ref_of(('big', 1), img, 11, 16, 0.1)
    got = ops.nl_means(img.astype(dtype), 11, 16, 0.1, ctx=ctx)
    check(got, img, ref, margin, dtype, 's 11 d 16')


@pytest.mark.parametrize('dtype,s', [(np.float32, 7), (np.float64, 7), (np.float32, 11), (np.float64, 11)])
def test_one_step_beyond_the_bound(ctx, dtype, s):
    from imgprocessor_amd import ops
    d = 0
    while lds_bytes(dtype, s, d + 1) <= 65536:
        d += 1
    assert d >= 16
    img = ctx.to_device(synth((8, 8), 71, dtype))
    out = ctx.to_device(np.full((8, 8), -5.0, dtype))
    with pytest.raises(ValueError):
        ops.nl_means(img, s, d + 1, 0.1, out=out)
    with pytest.raises(ValueError):
        ops.nl_means(img, 12, 3, 0.1, out=out)
    ctx.synchronize()
    assert (out.get() == -5.0).all(), 'something was launched'
    ops.nl_means(img, s, d, 0.1, out=out)   # the bound itself runs
    assert np.isfinite(out.get()).all() and (out.get() != -5.0).all()


@pytest.mark.parametrize('dtype', [np.float32, np.float64])
def test_calibration_denoise(ctx, dtype):
    from imgprocessor_amd import ops
    from imgprocessor_amd.camera.CameraCalibration import CameraCalibration
    from imgprocessor_amd.camera.LensDistortion import LensDistortion
    h, w = 40, 52
    img = (synth((h, w), 80, np.float64) * 1000).astype(dtype)
    img[5, 7] = img[20, 30] = img[0, 0] = np.nan
    cal = CameraCalibration(ctx=ctx)
    ld = LensDistortion(newCameraMatrix='same', ctx=ctx)
    ld.setCameraParams(60.0, 60.0, (w - 1) / 2.0, (h - 1) / 2.0, -0.1, 0.02, 0.0, 1e-3, -5e-4)
    cal.addLens(ld)
    cal.addDarkCurrent(np.full((h, w), 3.0))
    plain = cal.correct(img, dtype=dtype, threshold=0.0)
    got = cal.correct(img, dtype=dtype, threshold=0.0, denoise=True, denoise_h=40.0)
    assert got.dtype == dtype
    want = ops.nl_means(np.where(np.isnan(plain), 0, plain).astype(dtype), 7, 11, 40.0, ctx=ctx)
    assert np.array_equal(got.view(np.uint8), want.view(np.uint8))
    assert np.abs(got - np.nan_to_num(plain)).max() > 1.0, 'nothing was denoised'
    # the reference's fixed h = 0.1 on a frame in counts: every distance beyond the cut-off
    same = cal.correct(img, dtype=dtype, threshold=0.0, denoise=True)
    assert np.array_equal(same, np.where(np.isnan(plain), 0, plain))
    d_got = cal.correct(ctx.to_device(img), threshold=0.0, denoise=True, denoise_h=40.0)
    assert np.array_equal(d_got.get().view(np.uint8), want.view(np.uint8))
    with pytest.raises(NotImplementedError):
        cal.correct(img, deblur=True)
    with pytest.raises(NotImplementedError):
        cal.correct(img, deblur=True, denoise=True)


def test_nan_to_zero(ctx):
    from imgprocessor_amd import ops
    a = np.stack([synth((9, 70), 90 + i) for i in range(3)])
    a[0, 0, 0] = a[2, 8, 69] = a[1, 4, 64] = np.nan
    d = ctx.to_device(a)
    assert ops.nan_to_zero(d) is d
    assert np.array_equal(d.get(), np.where(np.isnan(a), 0, a))


# ------------------------------------------------- every instantiation at its tile edges ----
@pytest.mark.parametrize('dtype', [np.float32, np.float64])
@pytest.mark.parametrize('s,shape_no,sigma', nr.GEO_CASES)
def test_instantiation_geometry(ctx, s, shape_no, sigma, dtype):
    """nlm_kernel<T, 2 | 4 | 8 | 10> one row past its 64- and 32-row tiles and one column past its
    column tile of 63 | 61 | 57 | 55, more than one workgroup in x and in y (test_cpu_nlm.py
    proves it); the even patch size below gives the same bits"""
    from imgprocessor_amd import ops
    img, ref, margin = nr.geo_case(s, shape_no, sigma)
    got = ops.nl_means(img.astype(dtype), s, nr.GEO_D, nr.GEO_H, sigma, ctx=ctx)
    check(got, img, ref, margin, dtype, 's %d %s sigma %g' % (s, img.shape, sigma))
    even = ops.nl_means(img.astype(dtype), s - 1, nr.GEO_D, nr.GEO_H, sigma, ctx=ctx)
    assert np.array_equal(even.view(np.uint8), got.view(np.uint8)), 'patch size %d' % (s - 1)


@pytest.mark.parametrize('dtype', [np.float32, np.float64])
def test_cutoff_is_strict(ctx, dtype):
    """an image of 0 and 4 at patch_size 5, h 0.8: every distance is an integer, computed exactly
    in both types on both sides, and most pixels have one equal to 5 - which keeps its weight
    exp(-5).  Nothing is set aside: there is no rounding that could switch a weight."""
    from imgprocessor_amd import ops
    img = nr.knife_image()
    ref, margin = nlm_ref(img, **nr.KNIFE)
    assert (margin == 0).any() and margin[margin > 0].min() >= 1.0
    got = ops.nl_means(img.astype(dtype), nr.KNIFE['patch_size'], nr.KNIFE['patch_distance'], nr.KNIFE['h'],
                       ctx=ctx)
    worst = np.abs(got - ref).max() / img.max()
    print('knife edge %s: worst %.2e of the range (tolerance %.2e)' % (np.dtype(dtype).name, worst, TOL[dtype]))
    assert worst <= TOL[dtype]


@pytest.mark.parametrize('dtype', [np.float32, np.float64])
@pytest.mark.parametrize('s', [3, 7, 10])
def test_patch_distance_0_and_1(ctx, s, dtype):
    from imgprocessor_amd import ops
    img = synth((37, 70), 95, np.float32)
    got = ops.nl_means(img.astype(dtype), s, 0, 0.1, ctx=ctx)   # the self pair alone: the input
    assert np.array_equal(got.view(np.uint8), img.astype(dtype).view(np.uint8))
    ref, margin = ref_of(('d1', s), img, s, 1, 0.1)
    got = ops.nl_means(img.astype(dtype), s, 1, 0.1, ctx=ctx)
    check(got, img, ref, margin, dtype, 's %d d 1' % s)


@pytest.mark.parametrize('dtype', [np.float32, np.float64])
@pytest.mark.parametrize('s', [3, 11])
def test_pitched_batch_small_and_large_patch(ctx, s, dtype):
    """test_pitched_batch at the two ends of the patch sizes, on frames of two column tiles"""
    from imgprocessor_amd import ops
    from imgprocessor_amd.device import dtype_id
    n, h, w = 2, 37, 70
    src = np.stack([synth((h, w), 40 + i, np.float32) for i in range(n)]).astype(dtype)   # float32-exact
    want = ops.nl_means(ctx.to_device(src), s, 3, 0.1).get()
    sp, dp = w + 9, w + 5
    sbig = np.full((n, h + 3, sp), 7.0, dtype)
    sbig[:, :h, :w] = src
    dbig = ctx.to_device(np.full((n, h + 2, dp), -5.0, dtype))
    ctx._check(ctx._lib.ipa_nl_means_dev(ctx.handle, ctx.to_device(sbig).ptr, dtype_id(dtype), n, h, w, sp,
                                         (h + 3) * sp, s, 3, 0.1, 0.0, dbig.ptr, dp, (h + 2) * dp), 'nl_means')
    got = dbig.get()
    assert np.array_equal(got[:, :h, :w].view(np.uint8), want.view(np.uint8))
    assert (got[:, h:, :] == -5.0).all() and (got[:, :, w:] == -5.0).all(), 'wrote outside'
    ref, margin = ref_of(('pitched', s), src[1].astype(np.float64), s, 3, 0.1)
    check(got[1, :h, :w], src[1], ref, margin, dtype, 'pitched frame 1, s %d' % s)


def _with_nans(shape, dtype, seed):
    rng = np.random.default_rng(seed)
    a = rng.standard_normal(shape).astype(dtype)
    a[rng.random(shape) < 0.2] = np.nan
    a.flat[0] = a.flat[-1] = np.nan
    a[..., -1, :] = np.where(np.arange(shape[-1]) % 2, np.nan, a[..., -1, :])
    return a


@pytest.mark.parametrize('dtype', [np.float32, np.float64])
@pytest.mark.parametrize('shape', [(1, 1), (4, 64), (5, 65), (9, 129), (3, 9, 70)])
def test_nan_to_zero_shapes(ctx, shape, dtype):
    from imgprocessor_amd import ops
    a = _with_nans(shape, dtype, sum(shape))
    a.flat[a.size // 2] = -0.0 if a.size > 2 else a.flat[a.size // 2]
    d = ctx.to_device(a)
    assert ops.nan_to_zero(d) is d
    want = np.where(np.isnan(a), dtype(0), a)
    assert np.array_equal(d.get().view(np.uint8), want.view(np.uint8))   # everything else keeps its bits


@pytest.mark.parametrize('dtype', [np.float32, np.float64])
def test_nan_to_zero_pitched(ctx, dtype):
    """two frames in a buffer whose rows and frames are further apart than they are long: the
    NaNs of the padding stay"""
    from imgprocessor_amd.device import dtype_id
    n, h, w, pitch, rows = 2, 9, 129, 140, 11
    big = np.full((n, rows, pitch), np.nan, dtype)
    a = _with_nans((n, h, w), dtype, 7)
    big[:, :h, :w] = a
    d = ctx.to_device(big)
    ctx._check(ctx._lib.ipa_nan_to_zero_dev(ctx.handle, d.ptr, dtype_id(dtype), n, h, w, pitch, rows * pitch),
               'nan_to_zero')
    got = d.get()
    assert np.array_equal(got[:, :h, :w].view(np.uint8), np.where(np.isnan(a), dtype(0), a).view(np.uint8))
    assert np.isnan(got[:, h:, :]).all() and np.isnan(got[:, :, w:]).all(), 'the padding was touched'
