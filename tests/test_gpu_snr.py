"""GPU: signal-to-noise maps (csrc/nlf.hip, measure/SNR/SNR.py) against the reference's maps
(tests/golden/nlf.npz) and the numpy restatement (tests/nlf_ref.py): bit for bit for a given
noise level function and background (chains of single IEEE operations), within 1e-12 where the
noise is one float64 mean over the frame, within the fit's 1e-6 where the NLF is estimated.
"""
import numpy as np
import pytest

from .conftest import load_golden
from . import nlf_cases as nc
from . import nlf_ref as ref
from .test_cpu_nlf import rel_err

pytestmark = pytest.mark.gpu


@pytest.fixture(scope='module')
def ctx():
    import imgprocessor_amd
    return imgprocessor_amd.default_context(0)


@pytest.fixture(scope='module')
def g():
    return load_golden('nlf.npz')


def _snr():
    from imgprocessor_amd.measure.SNR import SNR, getBackgroundLevel
    return SNR, getBackgroundLevel


def same(a, b):
    return np.array_equal(np.asarray(a), np.asarray(b), equal_nan=True)


def check_map(got, want, constant, what):
    if constant:
        e = rel_err(got, want)
        print('%-40s rel err %.1e' % (what, e))
        assert e <= 1e-12, (what, e)
    else:
        assert same(got, want), what


@pytest.mark.parametrize('form', list(nc.SNR_FORMS))
def test_snr_golden(ctx, g, form):
    SNR, _ = _snr()
    f1, f2 = nc.snr_frames(nc.SNR_SHAPE)
    pair, kw = nc.snr_kwargs(form, nc.SNR_TRIPLE)
    got = SNR(f1, f2 if pair else None, **kw)
    assert isinstance(got, np.ndarray) and got.dtype == np.float64
    check_map(got, g['snr_' + form], kw.get('constant_noise_level'), form)


@pytest.mark.parametrize('shape', [(37, 53), (96, 160)])
@pytest.mark.parametrize('form', list(nc.SNR_FORMS))
def test_snr_forms(ctx, form, shape):
    """every form on host and device frames, uint16 and float32"""
    SNR, _ = _snr()
    from imgprocessor_amd import DeviceArray
    for dt in (np.uint16, np.float32):
        f1, f2 = nc.snr_frames(shape, seed=600, dtype=dt)
        pair, kw = nc.snr_kwargs(form, nc.SNR_TRIPLE)
        want = ref.snr(f1, f2 if pair else None, **kw)
        const = kw.get('constant_noise_level')
        what = '%s %dx%d %s' % (form, shape[0], shape[1], np.dtype(dt).name)
        check_map(SNR(f1, f2 if pair else None, **kw), want, const, what)
        d = SNR(ctx.to_device(f1), ctx.to_device(f2) if pair else None, **kw)
        assert isinstance(d, DeviceArray)
        check_map(d.get(), want, const, what + ' (device)')


def test_bg_array_and_bounded_nlf_object(ctx):
    SNR, _ = _snr()
    from imgprocessor_amd.camera.NoiseLevelFunction import BoundedNLF
    f1, f2 = nc.snr_frames((37, 53), seed=610)
    bg = np.random.default_rng(3).uniform(50, 150, (37, 53))
    want = ref.snr(f1, f2, bg, nc.SNR_TRIPLE)
    assert same(SNR(f1, f2, bg, nc.SNR_TRIPLE), want)
    assert same(SNR(f1, f2, bg, BoundedNLF(*nc.SNR_TRIPLE)), want)
    assert same(SNR(ctx.to_device(f1), ctx.to_device(f2), ctx.to_device(bg), nc.SNR_TRIPLE).get(), want)


def test_background_level(ctx, g):
    _, getBackgroundLevel = _snr()
    f1, _ = nc.snr_frames(nc.SNR_SHAPE)
    g1, g2 = nc.snr_frames(nc.SNR_NLF_SHAPE, seed=84)
    assert np.array_equal([getBackgroundLevel(f1), getBackgroundLevel(ctx.to_device(g1)),
                           getBackgroundLevel(g2.astype(np.float64))], g['bg_level'])
    from imgprocessor_amd import ops
    for shape in ((21, 21), (31, 32), (150, 260)):
        a = nc.gradient(shape[0], shape[1], 620, np.float32)
        assert same(ops.snr_bg_median(a), ref.median3(a.astype(np.float64)[10:-10:10, 10:-10:10])), shape
    with pytest.raises(ValueError):
        ops.snr_bg_median(np.zeros((20, 40)))


def test_nan_pixels_stay_nan(ctx):
    from imgprocessor_amd import ops
    SNR, _ = _snr()
    rng = np.random.default_rng(8)
    sig = rng.uniform(0, 3000, (37, 53))
    sig[rng.random(sig.shape) < 0.05] = np.nan
    noise = rng.uniform(0.2, 30, sig.shape)
    noise[5, 5] = np.nan
    for kw, n in (({'nlf': nc.SNR_TRIPLE}, np.maximum(ref.bounded_nlf(sig, *nc.SNR_TRIPLE), 1.0)),
                  ({'noise': noise}, np.where(noise < 1, 1.0, noise)),
                  ({'constant_noise': 0.25}, 0.25)):
        with np.errstate(invalid='ignore'):
            want = (sig - 40.0) / (n * 0.5 ** 0.5)
            want = np.where(want < 1, 1.0, want)
        got = ops.snr_map(sig, noise_factor=0.5 ** 0.5, bg_level=40.0, **kw)
        assert same(got, want), sorted(kw)
        assert np.isnan(got[np.isnan(sig)]).all()
    # through SNR: a NaN pixel makes its 3x3 neighbourhood NaN, every other pixel is unchanged
    f = nc.gradient(37, 53, 630, np.float64)
    want = ref.snr(f, bg=50.0, noise_level_function=nc.SNR_TRIPLE)
    f[7, 9] = f[20, 0] = np.nan
    got = SNR(f, bg=50.0, noise_level_function=nc.SNR_TRIPLE)
    hit = np.zeros(f.shape, bool)
    hit[6:9, 8:11] = hit[19:22, 0:2] = True
    assert np.isnan(got[hit]).all() and same(got[~hit], want[~hit])


def test_snr_with_an_estimated_nlf(ctx, g):
    SNR, _ = _snr()
    g1, g2 = nc.snr_frames(nc.SNR_NLF_SHAPE, seed=84)
    assert np.array_equal([g1.sum(dtype=np.float64), g2.sum(dtype=np.float64)], g['snr_nlf_in_sum'])
    for key, args in (('snr_nlf_one', (g1,)), ('snr_nlf_pair', (g1, g2, 100.0))):
        e = rel_err(SNR(*args)[::nc.SNR_NLF_STEP, ::nc.SNR_NLF_STEP], g[key])
        print('%s: rel err %.1e' % (key, e))
        assert e <= 1e-6
