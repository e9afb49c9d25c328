"""GPU: noise level function estimation (csrc/nlf.hip, camera/NoiseLevelFunction.py) against
the reference's outputs (tests/golden/nlf.npz) and the numpy restatement (tests/nlf_ref.py):
the signal bit for bit, the counts exactly, x / y / moments within 1e-12 (float64 sums over
<= 1e7 terms: eps * log2 N is 3e-15), fitted function values within 1e-6 (curve_fit's xtol).
The measured margins are printed.  test_cpu_nlf.py proves on the CPU which defect each boundary
scene sees.
"""
import ctypes as C

import numpy as np
import pytest

from .conftest import load_golden
from . import nlf_cases as nc
from . import nlf_ref as ref
from .test_cpu_nlf import check_nlf, rel_err

pytestmark = pytest.mark.gpu

SHAPES = [(1, 1), (1, 57), (41, 1), (2, 2), (37, 53), (150, 260)]


@pytest.fixture(scope='module')
def ctx():
    import imgprocessor_amd
    return imgprocessor_amd.default_context(0)


@pytest.fixture(scope='module')
def g():
    return load_golden('nlf.npz')


@pytest.fixture(scope='module')
def N():
    from imgprocessor_amd.camera import NoiseLevelFunction
    return NoiseLevelFunction


def _ops():
    from imgprocessor_amd import ops
    return ops


def same(a, b):
    return np.array_equal(np.asarray(a), np.asarray(b), equal_nan=True)


def check_bins(got, want, what):
    (c, s), (c0, s0) = got, want
    assert np.array_equal(c, c0), what + ': counts'
    e = rel_err(np.where(c0 > 0, s, 0.0), np.where(c0 > 0, s0, 0.0))
    print('%-36s sums rel err %.1e' % (what, e))
    assert e <= 1e-12, (what, e)
    assert np.all(s[c0 == 0] == 0.0), what + ': an empty bin has a sum'


# ------------------------------------------------------------------ signal
@pytest.mark.parametrize('shape', SHAPES)
def test_signal_is_scipys_median(ctx, shape):
    ops = _ops()
    for i, dt in enumerate(nc.DTYPES):
        a, b = nc.gradient(shape[0], shape[1], 200 + i, dt), nc.gradient(shape[0], shape[1], 210 + i, dt)
        assert same(ops.nlf_signal(a), ref.signal_of(a)), (shape, dt)
        assert same(ops.nlf_signal(a, b), ref.signal_of(a, b)), (shape, dt, 'pair')
        assert same(ops.nlf_signal(a, b, bg=17.0), ref.signal_of(a, b, 17.0)), (shape, dt, 'bg')
        bg = np.random.default_rng(5).uniform(0, 30, shape)
        d = ops.nlf_signal(ctx.to_device(a), bg=ctx.to_device(bg))
        assert d.dtype == np.float64 and same(d.get(), ref.signal_of(a, None, bg)), (shape, dt, 'device')
        assert same(ops.nlf_signal(a, bg=bg), ref.signal_of(a, None, bg)), (shape, dt, 'host bg array')


def test_pitched_rows(ctx):
    """frames, signal and outputs with pitches wider than the row, through the C ABI"""
    lib, h, w, pitch, spitch = ctx._lib, 37, 53, 64, 71
    rng = np.random.default_rng(7)
    wide = rng.integers(0, 4000, (h, pitch)).astype(np.uint16)
    wide2 = rng.integers(0, 4000, (h, pitch + 3)).astype(np.uint16)
    a, b = wide[:, :w], wide2[:, :w]
    d1, d2 = ctx.to_device(wide), ctx.to_device(wide2)
    d_sig = ctx.to_device(np.full((h, spitch), -7.0))
    ctx._check(lib.ipa_nlf_signal_dev(ctx.handle, d1.ptr, 1, d2.ptr, h, w, pitch, pitch + 3, None, 0, 0.0,
                                      d_sig.ptr, spitch), 'signal')
    sig = d_sig.get()
    assert same(sig[:, :w], ref.signal_of(a, b)) and np.all(sig[:, w:] == -7.0)
    m = np.empty(5)
    ctx._check(lib.ipa_nlf_moments_dev(ctx.handle, d_sig.ptr, 3, h, w, spitch, m.ctypes.data_as(C.POINTER(C.c_double))),
               'moments')
    want = ref.moments(sig[:, :w])
    assert m[0] == want[0] and m[1] == want[1] and m[4] == 0
    assert rel_err(m[2:4], want[2:4]) <= 1e-12
    e = nc.edge_table(want[0], (want[1] - want[0]) / 9, 9)
    cnt, sm = np.zeros(9, np.uint64), np.zeros(9)
    ctx._check(lib.ipa_nlf_bins_dev(ctx.handle, d1.ptr, 1, d2.ptr, h, w, pitch, pitch + 3, None, 0, 0.0,
                                    d_sig.ptr, spitch, e.ctypes.data_as(C.POINTER(C.c_double)), 9,
                                    (want[1] - want[0]) / 9, 2 ** 0.5, 0, cnt.ctypes.data_as(C.c_void_p),
                                    sm.ctypes.data_as(C.POINTER(C.c_double))), 'bins')
    d = ref.diff_of(a, sig[:, :w], b)
    check_bins((cnt.astype(np.int64), sm), ref.loop_bins(sig[:, :w], np.abs(d), e), 'pitched pair')


# ------------------------------------------------------------------ calcNLF
@pytest.mark.parametrize('name', list(nc.GOLDEN_NLF))
def test_calc_nlf_golden(ctx, g, N, name):
    img, img2, kw = nc.nlf_inputs(name)
    p = 'nlf_%s_' % name
    got = N.calcNLF(img, img2, **kw)
    check_nlf(got, g, p, name)
    assert isinstance(got[3], np.ndarray) and same(got[3], ref.signal_of(img, img2))
    # device frames: the same numbers, the signal stays on the device
    d = N.calcNLF(ctx.to_device(img), None if img2 is None else ctx.to_device(img2), **kw)
    check_nlf(d, g, p, name + ' (device)')
    assert same(d[3].get(), got[3]) and all(isinstance(v, np.ndarray) for v in d[:3])


def test_callers_signal_and_x_reuse(ctx, g, N):
    img, img2, _ = nc.nlf_inputs('pair_uint16')
    sig = ref.signal_of(img)
    got = N.calcNLF(img, img2, signal=sig)
    check_nlf(got, g, 'nlf_signal_', 'caller signal (host)')
    assert got[3] is sig
    got = N.calcNLF(ctx.to_device(img), ctx.to_device(img2), signal=ctx.to_device(sig))
    check_nlf(got, g, 'nlf_signal_', 'caller signal (device)')
    # mn_mx_nbins with the x of an earlier call: left as it is
    img, _, kw = nc.nlf_inputs('given_uint16')
    x0 = N.calcNLF(img, **kw)[0]
    x1, y1, w1, _ = N.calcNLF(nc.gradient(64, 96, 133, np.uint16), x=x0, **kw)
    assert x1 is x0 and len(y1) == len(x0)


@pytest.mark.parametrize('shape', SHAPES + [(5, 7), (3, 63), (3, 65), (2, 513)])
def test_bins_on_ragged_shapes(ctx, shape):
    """every shape of the signal tests, widths one more and one less than a multiple of the
    lane's run of 8, in all call forms"""
    ops = _ops()
    h, w = shape
    for i, dt in enumerate(nc.DTYPES):
        a, b = nc.gradient(h, w, 300 + i, dt), nc.gradient(h, w, 310 + i, dt)
        lo, span = nc.RANGE[dt]
        mn, mx, nbins = lo - 5, lo + span + 5, 17
        step = (mx - mn) / nbins
        e = ref.edges_of(mn, step, nbins)
        sig = ref.signal_of(a)
        for form, img2, factor, rms in (('one', None, ref.F_NOISE_WITH_MEDIAN, False), ('multi', None, 1.0, False),
                                        ('pair', b, 2 ** 0.5, False), ('rms', None, ref.F_NOISE_WITH_MEDIAN, True)):
            d = ref.diff_of(a, sig, img2, multiple=form == 'multi')
            got = ops.nlf_bins(a, sig, e, step, img2=img2, factor=factor, rms=rms)
            check_bins(got, ref.loop_bins(sig, d * d if rms else np.abs(d), e),
                       '%dx%d %s %s' % (h, w, np.dtype(dt).name, form))
        bg = np.random.default_rng(6).uniform(0, 3, shape)     # a host background array
        sig = ref.signal_of(a, None, bg)
        check_bins(ops.nlf_bins(a, sig, e, step, bg=bg, factor=ref.F_NOISE_WITH_MEDIAN),
                   ref.loop_bins(sig, np.abs(ref.diff_of(a, sig, None, bg)), e),
                   '%dx%d %s host bg' % (h, w, np.dtype(dt).name))


def test_idle_workgroups_write_zeros(ctx, N):
    """5 x 7 pixels on 512 workgroups: 511 slabs and 511 moment partials must be zero"""
    ops = _ops()
    a = nc.gradient(5, 7, 77, np.float64)
    sig = ref.signal_of(a)
    e = ref.edges_of(150.0, 400.0, 8)
    old = ctx.set_tuning(nlf_grid=512)
    try:
        got = ops.nlf_bins(a, sig, e, 400.0, factor=1.0)
        m = ops.nlf_moments(sig)
    finally:
        ctx.set_tuning(**old)
    check_bins(got, ref.loop_bins(sig, np.abs(a - sig), e), '5x7 on 512 workgroups')
    want = ref.moments(sig)
    assert m[:2] == want[:2] and m[4] == 0 and rel_err(m[2:4], want[2:4]) <= 1e-12


@pytest.mark.parametrize('scene', ['planted_edges', 'accumulated_edges'])
def test_pixels_on_the_edges(ctx, scene):
    ops = _ops()
    img, sig, (mn, mx, nbins) = getattr(nc, scene)()
    step = (mx - mn) / nbins
    e = ref.edges_of(mn, step, nbins)
    got = ops.nlf_bins(img, sig, e, step, factor=1.0)
    check_bins(got, ref.loop_bins(sig, np.abs(img - sig), e), scene)


def test_integer_frames_with_step_one(ctx, N):
    """every pixel on an edge: in two bins, but for those on e[0] and e[nbins]"""
    for img in (nc.nlf_inputs('step1_uint8')[0], nc.uniform_int(41, 57, 140, np.uint16, 1050, 1090)):
        x, y, w, sig = N.calcNLF(img)
        x0, y0, w0, _ = ref.calc_nlf(img)
        assert np.array_equal(w, w0) and rel_err(y, y0) <= 1e-12 and rel_err(x, x0) <= 1e-12
        mn, mx = ref.min_max(sig)
        assert (mx - mn) / len(w) == 1.0
        counts, _ = _ops().nlf_bins(img, sig, ref.edges_of(mn, 1.0, len(w)), 1.0)
        assert counts.sum() == 2 * sig.size - (sig == mn).sum() - (sig == mx).sum()


def test_bin_count_limits(ctx):
    ops = _ops()
    rng = np.random.default_rng(11)
    sig = rng.uniform(-3.0, 2051.0, (150, 260))     # some pixels outside either end
    img = sig + rng.standard_normal(sig.shape)
    for nbins in (1, 2, 1300, 1800, 2048):      # workgroups of 4, 4, 3, 2 and 1 waves
        step = 2048.0 / nbins
        e = ref.edges_of(0.0, step, nbins)
        check_bins(ops.nlf_bins(img, sig, e, step), ref.loop_bins(sig, np.abs(img - sig), e), '%d bins' % nbins)
    # one bin of no width: the pixels equal to its edge
    flat_sig = np.full((37, 53), 5.0)
    flat_sig[3, 4] = 6.0
    c, s = ops.nlf_bins(flat_sig + 1.0, flat_sig, [5.0, 5.0], 0.0)
    assert c[0] == flat_sig.size - 1 and s[0] == c[0]
    # 2049: refused, outputs untouched
    with pytest.raises(NotImplementedError):
        ops.nlf_bins(img, sig, ref.edges_of(0.0, 1.0, 2049), 1.0)
    d_img, d_sig = ctx.to_device(img), ctx.to_device(sig)
    e = ref.edges_of(0.0, 1.0, 2049)
    cnt, sm = np.full(2049, 123, np.uint64), np.full(2049, -4.5)
    rc = ctx._lib.ipa_nlf_bins_dev(ctx.handle, d_img.ptr, 3, None, 150, 260, 260, 0, None, 0, 0.0, d_sig.ptr, 260,
                                   e.ctypes.data_as(C.POINTER(C.c_double)), 2049, 1.0, 1.0, 0,
                                   cnt.ctypes.data_as(C.c_void_p), sm.ctypes.data_as(C.POINTER(C.c_double)))
    assert rc == -2 and np.all(cnt == 123) and np.all(sm == -4.5)
    with pytest.raises(ValueError):
        ops.nlf_bins(img, sig, [0.0, 0.0, 0.0], 0.0)    # no width and more than one bin


def test_flat_frame_in_one_or_two_bins(ctx):
    """worst contention: every pixel of 150 x 260 in the same bin, or on the edge between two"""
    ops = _ops()
    sig = np.full((150, 260), 5.0)
    img = sig + np.random.default_rng(12).standard_normal(sig.shape)
    for e in ([4.0, 5.0, 6.0], [4.5, 5.5, 6.5]):
        check_bins(ops.nlf_bins(img, sig, e, 1.0), ref.loop_bins(sig, np.abs(img - sig), np.array(e)),
                   'flat frame, edges %s' % e)


def test_min_len_is_inclusive(ctx, N):
    img, sig, (keep, drop) = nc.min_len_scene()
    x, y, w, _ = N.calcNLF(img, signal=sig)
    x0, y0, w0, _ = ref.calc_nlf(img, signal=sig)
    assert np.array_equal(w, w0) and rel_err(y, y0) <= 1e-12 and rel_err(x, x0) <= 1e-12
    assert 12 in w and 11 not in w


# ------------------------------------------------------------------ moments
def test_moments_of_a_narrow_frame(ctx):
    ops = _ops()
    f = nc.moments_frame()
    mn, mx, mean, std, n_nan = ops.nlf_moments(f)
    assert (mn, mx, n_nan) == (f.min(), f.max(), 0)
    em, es = abs(mean - np.mean(f)) / np.mean(f), abs(std - np.std(f)) / np.std(f)
    print('moments, mean 60000 std 2: rel err mean %.1e std %.1e' % (em, es))
    assert em <= 1e-12 and es <= 1e-12
    for shape in SHAPES:
        a = nc.gradient(shape[0], shape[1], 400, np.float64)
        m = ops.nlf_moments(ctx.to_device(a))
        want = ref.moments(a)
        assert m[:2] == want[:2] and rel_err(m[2:4], want[2:4]) <= 1e-12, shape
    # raw frames of every type, host and device (what estimateFromImages hands to _getMinMax)
    for i, dt in enumerate(nc.DTYPES):
        f = nc.gradient(37, 53, 410 + i, dt)
        want = ref.moments(f.astype(np.float64))
        for m in (ops.nlf_moments(f), ops.nlf_moments(ctx.to_device(f))):
            assert m[:2] == want[:2] and m[4] == 0 and rel_err(m[2:4], want[2:4]) <= 1e-12, dt
    a[3, 5] = a[100, 200] = np.nan
    m = ops.nlf_moments(a)
    assert m[4] == 2 and m[0] == np.nanmin(a) and m[1] == np.nanmax(a)
    assert rel_err(m[2:4], [np.nanmean(a), np.nanstd(a)]) <= 1e-12


def test_nan_and_constant_frames(ctx, N):
    a = nc.gradient(37, 53, 401, np.float64)
    a[10, 10] = np.nan
    with pytest.raises(ValueError):
        N.calcNLF(a)                                    # the median carries the NaN
    with pytest.raises(ValueError):
        N.calcNLF(nc.gradient(37, 53, 402, np.uint16), signal=a)
    with pytest.raises(ValueError):
        N._getMinMax(a)
    # given a range, a NaN pixel counts in no bin
    x, y, w, _ = N.calcNLF(np.nan_to_num(a), signal=a, mn_mx_nbins=(0.0, 4000.0, 10))
    assert w.sum() == a.size - 1
    x, y, w, sig = N.calcNLF(np.full((20, 20), 7, np.uint8))
    assert x.shape == y.shape == w.shape == (0,) and np.all(sig == 7.0)


# ------------------------------------------------------------------ end to end
def test_one_image_nlf_fit(ctx, g, N):
    f = nc.fit_frame()
    assert f.sum(dtype=np.float64) == g['fit_in_sum'][0]
    x, y, w, _ = N.calcNLF(f)
    check_nlf((x, y, w), g, 'fit_', 'fit frame')
    fn, sig = N.oneImageNLF(ctx.to_device(f))
    e = rel_err(fn(g['fit_grid']), g['fit_values'])
    print('oneImageNLF: function values rel err %.1e' % e)
    assert e <= 1e-6 and len(fn.triple) == 3 and same(sig.get(), ref.signal_of(f))


@pytest.mark.parametrize('dev', [False, True], ids=['host', 'device'])
def test_estimate_from_images(ctx, g, N, dev):
    imgs1, imgs2 = nc.estimate_pairs()
    assert np.array_equal([a.sum(dtype=np.float64) for a in imgs1 + imgs2], g['est_in_sum'])
    if dev:     # uint16 DeviceArrays: the range comes from the raw frames' moments
        imgs1, imgs2 = [ctx.to_device(a) for a in imgs1], [ctx.to_device(a) for a in imgs2]
    x, fn, y_avg, y_vals, w_vals, params, i = N.estimateFromImages(imgs1, imgs2)
    assert np.array_equal(x, g['est_x']) and params is not None
    ey, ew = rel_err(y_avg, g['est_y_avg']), rel_err(w_vals, g['est_w_vals'])
    ev = rel_err(y_vals, g['est_y_vals'])
    ef = rel_err(fn(g['est_grid']), g['est_values'])
    print('estimateFromImages: rel err y_avg %.1e y_vals %.1e w_vals %.1e function %.1e' % (ey, ev, ew, ef))
    assert ey <= 1e-12 and ev <= 1e-12 and ew <= 1e-12 and ef <= 1e-6


def test_get_min_max_of_raw_device_frames(ctx, N):
    for i, dt in enumerate(nc.DTYPES):
        f = nc.gradient(37, 53, 420 + i, dt)
        want = ref.min_max(f.astype(np.float64))
        for got in (N._getMinMax(f), N._getMinMax(ctx.to_device(f))):
            assert rel_err(got, want) <= 1e-12, dt


def test_frames_of_different_types(ctx, N):
    """two host frames of different types are both float64, as np.asfarray of each: a float second
    exposure is never cast to the first frame's integers; DeviceArrays of different types raise"""
    from imgprocessor_amd.measure.SNR import SNR
    a = nc.gradient(64, 96, 430, np.uint16)
    b = nc.gradient(64, 96, 431, np.float64) - 250.5        # fractions, and negative values
    assert (b < 0).any()
    for first, second in ((a, b), (b, a), (a.astype(np.uint8), a.astype(np.float32) + 0.25)):
        x, y, w, sig = N.calcNLF(first, second)
        x0, y0, w0, sig0 = ref.calc_nlf(first, second)
        assert same(sig, sig0) and np.array_equal(w, w0) and rel_err(y, y0) <= 1e-12
        assert same(_ops().nlf_signal(first, second), sig0)
    assert same(SNR(a, b, 10.0, nc.SNR_TRIPLE), ref.snr(a, b, 10.0, nc.SNR_TRIPLE))
    for first, second in ((ctx.to_device(a), ctx.to_device(b)), (ctx.to_device(a), b), (a, ctx.to_device(b))):
        with pytest.raises(ValueError):
            N.calcNLF(first, second)


def test_ste_with_an_estimated_nlf(ctx, N):
    """an estimated NLF takes the device path: the same bits as its .triple, and as the host
    round trip of a plain callable"""
    from imgprocessor_amd.features import SingleTimeEffectDetection as S
    fr = np.stack([nc.gradient(96, 160, 500 + i, np.uint16) for i in range(3)])
    fr[2, 40:42, 50:52] += 900
    fn = N.oneImageNLF(np.minimum(fr[0], fr[1]))[0]
    s_fn, s_tri = S(list(fr), fn), S(list(fr), fn.triple)
    s_host = S(list(fr), lambda v: fn(v))
    for s in (s_tri, s_host):
        assert same(s_fn.threshold, s.threshold) and same(s_fn.noSTE, s.noSTE)
        assert np.array_equal(s_fn.mask_clean, s.mask_clean)
    assert not s_fn.mask_clean[40, 50]
