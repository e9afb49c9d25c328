"""GPU: every kernel of the secondary stencils (csrc/stencils.hip, csrc/stencils_ydep.hip) on
both sides of the window at which its launcher switches to the next one, against the plain
references of tests/stencil_ref.py and the C oracle.

Which kernel a case runs is asked of the library (ipa_stencil_path, the launchers' own
arithmetic), and every boundary pair is asserted to land on two different paths.  Frames are
small and ragged (one pixel, one row, one column, widths around 64 and 256, windows larger than
the frame); data has both signs, ties, +-0, +-inf and NaNs where the operation defines them.

Tolerances: selections and integer outputs bit-equal; float64 reductions at the bound of the
existing GPU test of the same operation; float32 outputs within close32.
"""
import os

import numpy as np
import pytest

from . import stencil_ref as ref
from . import stencil_cases as sc
from .conftest import assert_close

pytestmark = pytest.mark.gpu

RT = 1e-5
F32, F64 = np.float32, np.float64
TINY = ((1, 1), (1, 70), (70, 1), (5, 63), (9, 64), (13, 65))
MASKED_SHAPES = ((1, 1), (1, 70), (70, 1), (13, 65), (37, 130))
MEAN_SHAPES = MASKED_SHAPES + ((5, 63), (9, 64))


@pytest.fixture(scope='module')
def ia():
    import imgprocessor_amd
    imgprocessor_amd.default_context(0)
    return imgprocessor_amd


@pytest.fixture(scope='module')
def orc(oracle):
    try:
        n = len(os.sched_getaffinity(0))
    except AttributeError:
        n = os.cpu_count() or 1
    oracle.set_threads(max(1, min(n, oracle.max_threads(), 32)))
    yield oracle
    oracle.set_threads(1)


def close32(got, want, what=''):
    """1e-5 relative plus 1e-5 of the largest FINITE reference value (an inf in the reference
    must be met by an inf, and does not widen the bound of the other pixels)"""
    assert got.dtype == F32, what
    want = np.asarray(want, dtype=np.float64)
    fin = np.abs(want[np.isfinite(want)])
    assert_close(got, want, RT, RT * (fin.max() if fin.size else 1.0), what)


def same(got, want, what=''):
    assert got.dtype == want.dtype and got.shape == want.shape, what
    assert np.array_equal(got, want, equal_nan=True), '%s: %d of %d differ' % (
        what, (~((got == want) | (np.isnan(got) & np.isnan(want)))).sum(), got.size)


def close_nan0(got, want, tol, what=''):
    """pos_intensity_unc as tests/test_gpu_parity.py compares it"""
    assert got.dtype == F64, what
    assert np.array_equal(np.isnan(got), np.isnan(want)), what
    assert_close(np.nan_to_num(got), np.nan_to_num(want), tol, tol, what)


def worst(got, want):
    """largest absolute and relative difference over the finite pixels, for the printed figures"""
    got, want = np.asarray(got, F64), np.asarray(want, F64)
    ok = np.isfinite(got) & np.isfinite(want)
    if not ok.any():
        return 0.0, 0.0
    d = np.abs(got[ok] - want[ok])
    return float(d.max()), float((d / np.maximum(np.abs(want[ok]), 1e-300)).max())


# ------------------------------------------------------------- local_std ----
def _std_path(dt, ks):
    return sc.path('local_std', dt, ks[0], ks[1])


@sc.cached
def std_inputs(shape, dt):
    return sc.frame('signed', shape, dt), sc.frame('signed', shape, dt, 8) * dt(0.5)


@sc.cached
def std_ref(shape, dt, ks):
    img, blurred = std_inputs(shape, dt)
    return ref.local_std(img, blurred, ks)


def _std_tile_last(dt):
    k = 12
    while _std_path(dt, (k + 1, k + 1)) == sc.STD_TILE:
        k += 1
    return k


STD_SQUARES = (2, 3, 4, 6, 7, 8, 9, 10, 11, 12, 13, 31)
STD_RECTS = ((3, 9), (9, 3), (2, 40))


@pytest.mark.parametrize('ks', [(k, k) for k in STD_SQUARES] + list(STD_RECTS),
                         ids=lambda k: '%dx%d' % k)
def test_local_std_wave_and_tile(ia, orc, ks):
    square = ks[0] == ks[1]
    for dt in sc.DTYPES:
        want_path = sc.STD_WAVE if square and ks[0] <= 11 else sc.STD_TILE
        assert _std_path(dt, ks) == want_path
        for shape in sc.SMALL + sc.WIDE:
            img, blurred = std_inputs(shape, dt)
            got = ia.ops.local_std(img, blurred, ks)
            wants = [('ref', std_ref(shape, dt, ks))]
            if square:
                wants.append(('oracle', orc.standardDeviation2d(img, ks[0], blurred)))
            for name, want in wants:
                what = 'local_std %s %s %s vs %s' % (ks, shape, dt.__name__, name)
                if dt is F64:
                    assert got.dtype == F64
                    assert_close(got, want, 1e-10, 1e-13, what)
                else:
                    close32(got, want, what)
    # the boundary pair 11 | 12 stands on two kernels
    assert _std_path(F32, (11, 11)) != _std_path(F32, (12, 12))
    assert _std_path(F64, (11, 11)) != _std_path(F64, (12, 12))


@pytest.mark.parametrize('dt', sc.DTYPES, ids=lambda d: d.__name__)
def test_local_std_tile_to_generic(ia, orc, dt):
    """the last window of the LDS tile kernel and the first of the generic one (48 KiB), and
    101: on the smallest frames, every window larger than the frame"""
    last = _std_tile_last(dt)
    assert _std_path(dt, (last, last)) == sc.STD_TILE
    assert _std_path(dt, (last + 1, last + 1)) == sc.STD_GENERIC
    assert _std_path(dt, (101, 101)) == sc.STD_GENERIC
    for k in (last, last + 1, 101):
        for shape in TINY:
            img, blurred = std_inputs(shape, dt)
            got = ia.ops.local_std(img, blurred, (k, k))
            for name, want in (('ref', std_ref(shape, dt, (k, k))),
                               ('oracle', orc.standardDeviation2d(img, k, blurred))):
                what = 'local_std %d %s %s vs %s' % (k, shape, dt.__name__, name)
                if dt is F64:
                    assert_close(got, want, 1e-10, 1e-13, what)
                else:
                    close32(got, want, what)


# ----------------------------------------------------------- masked mean ----
def _mean_fill_out_of_place(ia, a, m, ks):
    """ipa_masked_mean_dev with fill_mask and d_out != d_arr (the plain kernel); the Python layer
    always fills in place"""
    from imgprocessor_amd.device import dtype_id
    ctx = ia.default_context(0)
    d_a, d_m, d_o = ctx.to_device(a), ctx.to_device(m.astype(np.uint8)), ctx.to_device(a)
    h, w = a.shape
    ctx._check(ctx._lib.ipa_masked_mean_dev(ctx.handle, d_a.ptr, dtype_id(a.dtype), d_m.ptr, h, w,
                                            w, w, int(ks), 1, d_o.ptr, w), 'masked_mean')
    return d_o.get()


@sc.cached
def mean_ref(shape, dt, kind, mk, ks, fill):
    return ref.masked_mean(sc.frame(kind, shape, dt), sc.mask(mk, shape, ks // 2), ks, fill)


@pytest.mark.parametrize('ks', [64, 65, 66, 67, 130])
def test_masked_mean_cols_and_wave(ia, orc, ks):
    """in place: the column-sum kernel up to ksize / 2 = 32 (its LDS columns exactly full), the
    wave kernel beyond, with its three branches by clipped window width: two rows per pass
    (<= 32: the one-column frames), one row (<= 64: (5, 63), (9, 64), the rim of (37, 130) at
    66 and 67) and the flat index (> 64: the wide frames); fill_mask=False and the out-of-place
    fill run the plain kernel.

    Bound: assert_close(1e-13, 1e-15) of tests/test_gpu_parity.py::test_masked_filter_and_nan_max
    is kept for every path.  The wave kernel sums in another order than the reference's loop
    (64 lane-strided partial sums, then a butterfly); that order, replayed in numpy on the
    (37, 130) frames at ksize 130, stays within 1.2e-16 of the extended-precision reference, 2e-3
    of the bound.  The float64 errors of the GPU and of the oracle against the reference are
    printed per frame on every run.
    """
    from imgprocessor_amd.filters import maskedFilter
    assert sc.path('masked_mean_fill', F64, 65) == sc.MEAN_COLS
    assert sc.path('masked_mean_fill', F64, 66) == sc.MEAN_WAVE
    figures = {}
    widths = {min(j + ks // 2, w) - max(j - ks // 2, 0) for _, w in MEAN_SHAPES for j in range(w)}
    assert ks <= 65 or {0, 1, 2} == {(ww > 32) + (ww > 64) for ww in widths}
    for dt in sc.DTYPES:
        assert sc.path('masked_mean_fill', dt, ks) == (sc.MEAN_COLS if ks <= 65 else sc.MEAN_WAVE)
        for shape in MEAN_SHAPES:
            for mk in ('block', 'single'):
                m = sc.mask(mk, shape, ks // 2)
                for kind in ('signed', 'quantised'):
                    a = sc.frame(kind, shape, dt)
                    what = 'masked mean k%d %s %s %s %s' % (ks, shape, dt.__name__, mk, kind)
                    inplace = a.copy()
                    assert maskedFilter(inplace, m, ks, fn='mean') is inplace
                    outplace = _mean_fill_out_of_place(ia, a, m, ks)
                    nofill = maskedFilter(a.copy(), m, ks, fill_mask=False, fn='mean')
                    assert inplace.dtype == outplace.dtype == nofill.dtype == dt
                    w_fill, w_nofill = (mean_ref(shape, dt, kind, mk, ks, f) for f in (True, False))
                    o_fill = orc.maskedFilter(a.copy(), m, ks, True, 'mean')
                    o_nofill = orc.maskedFilter(a.copy(), m, ks, False, 'mean')
                    # untouched pixels keep their bits; a window without unmasked pixel writes none
                    assert np.array_equal(inplace[~m], a[~m]) and np.array_equal(outplace[~m], a[~m])
                    assert np.array_equal(np.isnan(nofill), np.isnan(w_nofill)), what
                    if dt is F64:
                        f = figures.setdefault(shape, {'gpu': (0, 0), 'oracle': (0, 0)})
                        f['gpu'] = tuple(np.maximum(f['gpu'], np.maximum(
                            worst(inplace, w_fill), worst(nofill, w_nofill))))
                        f['oracle'] = tuple(np.maximum(f['oracle'], np.maximum(
                            worst(o_fill, w_fill), worst(o_nofill, w_nofill))))
                    checks = ((inplace, w_fill, 'in place vs ref'), (inplace, o_fill, 'in place vs oracle'),
                              (outplace, w_fill, 'out of place vs ref'),
                              (inplace, outplace, 'in place vs out of place'),
                              (nofill, w_nofill, 'nofill vs ref'), (nofill, o_nofill, 'nofill vs oracle'))
                    for got, want, name in checks:
                        if dt is F64:
                            assert_close(got, want, 1e-13, 1e-15, what + ' ' + name)
                        else:
                            close32(got, want, what + ' ' + name)
    for shape, f in figures.items():
        print('masked mean k%d %s float64: GPU vs ref abs %.3g rel %.3g | oracle vs ref abs %.3g '
              'rel %.3g' % ((ks, shape) + f['gpu'] + f['oracle']))


# --------------------------------------------------------- masked median ----
@sc.cached
def median_ref(shape, dt, kind, mk, ks, fill):
    return ref.masked_median(sc.frame(kind, shape, dt), sc.mask(mk, shape, ks // 2), ks, fill)


def _median_last(dt):
    return sc.boundary('masked_median', dt)[0]


@pytest.mark.parametrize('dt,ks', [(F32, 2), (F32, 3), (F32, 45), (F64, 2), (F64, 3), (F64, 33)],
                         ids=lambda v: getattr(v, '__name__', str(v)))
def test_masked_median(ia, orc, dt, ks):
    """pure selection: bit-equal.  45 / 33 are the largest windows the per-wave LDS buffers take
    (float64 33: exactly 64 KiB of dynamic LDS); negative, tied, +-0 and +-inf values, odd and
    even counts, windows with one unmasked pixel and with none, NaN in the window -> NaN"""
    from imgprocessor_amd.filters import maskedFilter
    assert sc.path('masked_median', dt, ks) == sc.MEDIAN_WAVE
    if ks > 3:
        assert ks == _median_last(dt)
    counts, nans = set(), 0
    for shape in MASKED_SHAPES + ((5, 63),):
        for mk in ('block', 'single'):
            m = sc.mask(mk, shape, ks // 2)
            for kind in ('special', 'nans', 'signed'):
                a = sc.frame(kind, shape, dt)
                what = 'masked median k%d %s %s %s %s' % (ks, shape, dt.__name__, mk, kind)
                fill = a.copy()
                assert maskedFilter(fill, m, ks, fn='median') is fill
                nofill = maskedFilter(a.copy(), m, ks, fill_mask=False, fn='median')
                for got, f in ((fill, True), (nofill, False)):
                    same(got, median_ref(shape, dt, kind, mk, ks, f), what + ' vs ref')
                    same(got, orc.maskedFilter(a.copy(), m, ks, f, 'median'), what + ' vs oracle')
                if kind == 'nans':   # a NaN among the window values, none at the pixel itself
                    nans += int((np.isnan(nofill) & ~m & ~np.isnan(a)).sum())
            counts |= set(np.unique(sc.window_counts(m, ks // 2)).tolist())
    # windows with no unmasked pixel, with exactly one, with odd and with even counts; NaN medians
    assert {0, 1} <= counts and any(c % 2 == 0 and c > 1 for c in counts) and \
        any(c % 2 and c > 1 for c in counts) and nans


@pytest.mark.parametrize('dt', sc.DTYPES, ids=lambda d: d.__name__)
def test_masked_median_first_refused_window(ia, dt):
    from imgprocessor_amd.filters import maskedFilter
    ks = _median_last(dt) + 1
    assert ks == {F32: 46, F64: 34}[dt]
    assert sc.path('masked_median', dt, ks - 1) == sc.MEDIAN_WAVE
    assert sc.path('masked_median', dt, ks) == sc.REFUSED
    shape = (13, 65)
    a, m = sc.frame('signed', shape, dt), sc.mask('block', shape, ks // 2)
    for fill in (True, False):
        b = a.copy()
        with pytest.raises(NotImplementedError):
            maskedFilter(b, m, ks, fill_mask=fill, fn='median')
        assert np.array_equal(b, a)
    ctx = ia.default_context(0)
    d, dm = ctx.to_device(a), ctx.to_device(m.astype(np.uint8))
    with pytest.raises(NotImplementedError):
        maskedFilter(d, dm, ks, fn='median')
    assert np.array_equal(d.get(), a)


# --------------------------------------------------------------- nan_max ----
@pytest.mark.parametrize('dt', sc.DTYPES, ids=lambda d: d.__name__)
def test_nan_max_separable_and_generic(ia, orc, dt):
    from imgprocessor_amd.filters import nan_maximum_filter
    last, first = sc.boundary('nan_max', dt)
    assert (last, first) == {F32: (53, 54), F64: (19, 20)}[dt]
    assert sc.path('nan_max', dt, 2) == sc.path('nan_max', dt, last) == sc.NANMAX_SEP
    assert sc.path('nan_max', dt, first) == sc.NANMAX_GENERIC
    all_nan = lone_inf = 0
    for ks in (2, last, first):
        for shape in sc.SMALL:
            a = sc.nan_max_frame(shape, ks // 2, dt)
            got = nan_maximum_filter(a, ks)
            want = ref.nan_max(a, ks)
            what = 'nan_max k%d %s %s' % (ks, shape, dt.__name__)
            same(got, want, what + ' vs ref')
            same(got, orc.nan_maximum_filter(a, ks), what + ' vs oracle')
            all_nan += int(np.isnan(want).sum())
            lone_inf += int(np.isneginf(want).sum())
    assert all_nan and lone_inf


# ------------------------------------------------------ closest_distance ----
@sc.cached
def closest_ref(shape, name, ks):
    return ref.closest_distance(sc.closest_frames(shape)[name], ks, np.float64)


@pytest.mark.parametrize('ks', [1, 253, 254, 255, 300])
def test_closest_distance_two_pass_and_direct(ia, orc, ks):
    """254 is the largest row distance a byte of the two-pass kernel holds beside its sentinel
    255; from 255 on the direct kernel runs.  Set pixels exactly 254 and 255 columns from a probe,
    diagonal neighbours just inside and just outside the window, a frame without a set pixel"""
    from imgprocessor_amd.render import closestDirectDistance
    assert sc.path('closest_distance', F64, 254) == sc.CDD_TWO_PASS
    assert sc.path('closest_distance', F64, 255) == sc.CDD_DIRECT
    assert sc.path('closest_distance', F64, ks) == (sc.CDD_TWO_PASS if ks <= 254 else sc.CDD_DIRECT)
    n_orc = 0
    for shape, name, k, dt, with_orc in sc.closest_cases():
        if k != ks:
            continue
        a = sc.closest_frames(shape)[name]
        got = closestDirectDistance(a, ks, dt)
        want = closest_ref(shape, name, ks)
        what = 'closest k%d %s %s %s' % (ks, shape, name, np.dtype(dt).name)
        same(got, want if dt is np.float64 else np.floor(want).astype(np.uint16), what + ' vs ref')
        if with_orc:
            same(got, orc.closestDirectDistance(a, ks, dt), what + ' vs oracle')
            n_orc += 1
        if name == 'empty':
            assert (got == 2 * ks).all()
    assert n_orc or ks in (253, 300)


# ----------------------------------------------------- pos_intensity_unc ----
@pytest.mark.parametrize('k', [1, 14, 15, 16])
def test_pos_intensity_unc_separable_and_generic(ia, orc, k):
    """half window 14 is the last whose column factors fit the 60 KiB of the separable kernel"""
    assert sc.boundary('pos_intensity_unc', F64, lo=1) == (14, 15)
    for dt in sc.DTYPES:
        assert sc.path('pos_intensity_unc', dt, k) == (sc.PIU_SEP if k <= 14 else sc.PIU_GENERIC)
        for shape in ((2 * k + 2, 2 * k + 3), (2 * k, 2 * k + 3), (37, 130)):
            img = sc.piu_frame(shape, dt)
            sx, sy = sc.piu_sigma_maps(shape)
            for s0, s1 in ((3.0, 1.25), (sx, sy)):
                got = ia.ops.pos_intensity_unc(img, s0, s1, k)
                want = ref.pos_intensity_unc(img, s0, s1, k)
                what = 'piu k%d %s %s %s' % (k, shape, dt.__name__, 'maps' if s0 is sx else 'const')
                close_nan0(got, want, 1e-12, what + ' vs ref')
                close_nan0(got, orc.positionToIntensityUncertainty(img, s0, s1, 2 * k + 1), 1e-12,
                           what + ' vs oracle')
                if shape[0] <= 2 * k:
                    assert not got.any(), what   # no pixel is k away from the rim
                elif shape[0] == 2 * k + 2:
                    # the 2 x 3 interior: the NaN centre stays 0, its neighbours are NaN
                    assert np.isnan(got).sum() == 5 and np.count_nonzero(got) == 5
                else:
                    assert np.isnan(got).any() and got[shape[0] // 2, shape[1] // 2] == 0


def test_pos_intensity_unc_default_kernel_size(ia, orc):
    """positionToIntensityUncertainty(img, 8, 8): kernelSize 4 std + 1 = 33, half window 16 -
    the generic kernel through the default public call"""
    from imgprocessor_amd.uncertainty import positionToIntensityUncertainty
    assert sc.path('pos_intensity_unc', F64, 33 // 2) == sc.PIU_GENERIC
    for dt in sc.DTYPES:
        img = sc.piu_frame((37, 130), dt)
        got = positionToIntensityUncertainty(img, 8.0, 8.0)
        close_nan0(got, ref.pos_intensity_unc(img, 8.0, 8.0, 16), 1e-12, 'default vs ref')
        close_nan0(got, orc.positionToIntensityUncertainty(img, 8.0, 8.0), 1e-12, 'default vs oracle')
        assert np.count_nonzero(np.nan_to_num(got, nan=1.0)) == 5 * 98 - 1


# ------------------------------------------------------- median_threshold ----
@pytest.mark.parametrize('size', [2, 3, 4, 5, 9])
def test_median_threshold_small_frames(ia, orc, size):
    """frames smaller than the window: the edge-repeating index folds more than once; medians
    that are exactly zero (the relative difference divides by them)"""
    assert sc.path('median_threshold', F32, size) == (sc.MT_NETWORK if size == 3 else sc.MT_COUNTING)
    assert sc.path('median_threshold', F32, 3) != sc.path('median_threshold', F32, 4)
    hits = zero_blur = 0
    for shape in ((1, 1), (1, 70), (70, 1), (2, 3), (5, 63)):
        for dt in sc.DTYPES:
            for kind in ('zeros', 'spiky'):
                img = sc.median_threshold_frame(kind, shape, dt)
                for cond in '><':
                    out, hit = ia.ops.median_threshold(img, 0.2, cond, size=size)
                    what = 'median_threshold s%d %s %s %s %s' % (size, shape, dt.__name__, kind, cond)
                    w_out, w_hit = ref.median_threshold(img, 0.2, size, cond)
                    same(out, w_out, what + ' vs ref')
                    same(hit, w_hit, what + ' vs ref (indices)')
                    o_out, o_hit = orc.medianThreshold(img, 0.2, size, cond)
                    same(out, o_out, what + ' vs oracle')
                    same(hit, o_hit, what + ' vs oracle (indices)')
                    hits += int(w_hit.sum())
                    zero_blur += int((w_out[w_hit] == 0).sum())
    assert hits and zero_blur


# ----------------------------------------------------------- var_y_gauss ----
@pytest.mark.parametrize('kx,stdx', [(1, 0), (3, 1), (5, 2), (7, 3)], ids=lambda v: str(v))
@pytest.mark.parametrize('dt', sc.DTYPES, ids=lambda d: d.__name__)
def test_var_y_gauss_tiled_and_expanded(ia, orc, dt, kx, stdx):
    """the last ky the tiled kernel takes and the first that goes through the expanded table, as
    the library reports them for this kx and dtype; kx 1, 3, 5 are the unrolled templates, 7
    the generic one; a NaN run is skipped without renormalisation"""
    from imgprocessor_amd.filters import varYSizeGaussianFilter
    last, first = sc.var_y_boundary(dt, kx)
    assert sc.path('var_y_gauss', dt, kx, last) == sc.VYG_TILED
    assert sc.path('var_y_gauss', dt, kx, first) in (sc.VYG_EXPANDED_TILE, sc.VYG_EXPANDED_GENERIC)
    tol = 1e-12 if dt is F64 else 2e-6
    for ky in (last, first):
        rng = (0.5, sc.stdy_for(ky))
        assert ref.var_y_sizes(rng, stdx)[2:] == (ky, kx)
        for shape in ((50, 257), (37, 130)):
            a = sc.var_y_frame(shape, dt)
            for modex in ('wrap', 'reflect'):
                got = varYSizeGaussianFilter(a, rng, stdx, modex=modex)
                assert got.dtype == dt and got.shape == shape
                what = 'var_y_gauss ky%d kx%d %s %s %s' % (ky, kx, shape, dt.__name__, modex)
                assert_close(got, ref.var_y_gauss(a, rng, stdx, modex), tol, tol, what + ' vs ref')
                assert_close(got, orc.varYSizeGaussianFilter(a, rng, stdx, modex), tol, tol,
                             what + ' vs oracle')
