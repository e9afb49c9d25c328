"""CPU: the plain references of tests/stencil_ref.py against the reference's own fixtures and
against the C oracle at the shapes and data of the GPU module, and the kernel-selection table of
the secondary stencils through ipa_stencil_path - so that a difference on the GPU is a kernel
against two references that already agree, standing on a boundary that is known to be one.

Selections and integer results bit-equal; float64 reductions within the bounds
tests/test_oracle_golden.py uses for the same operation.
"""
import numpy as np
import pytest

from . import stencil_ref as ref
from . import stencil_cases as sc
from .conftest import load_golden, assert_close

F32, F64 = np.float32, np.float64


@pytest.fixture(scope='module')
def orc(oracle):
    """the oracle on every CPU this process may use (its window loops are OpenMP-parallel)"""
    import os
    try:
        n = len(os.sched_getaffinity(0))
    except AttributeError:
        n = os.cpu_count() or 1
    oracle.set_threads(max(1, min(n, oracle.max_threads(), 32)))
    yield oracle
    oracle.set_threads(1)


def same(got, want, what=''):
    assert got.dtype == want.dtype and np.array_equal(got, want, equal_nan=True), what


# ------------------------------------------------------------- goldens ----
def test_local_std_golden():
    import scipy.ndimage as ndi
    g = load_golden('std2d.npz')
    for k in (5, 11):
        blurred = ndi.gaussian_filter(g['img'], (k, k))
        assert_close(ref.local_std(g['img'], blurred, (k, k)), g['std_k%d' % k], 1e-11, 1e-14)
    blurred = ndi.gaussian_filter(g['img32'], (5, 5))
    assert_close(ref.local_std(g['img32'], blurred, (5, 5)), g['std32_k5'], 2e-6, 1e-7)


def test_masked_filter_and_nan_max_golden():
    g = load_golden('masked_filter.npz')
    for ks in (6, 11, 30):
        assert_close(ref.masked_mean(g['arr'], g['mask'], ks), g['mean_fill_k%d' % ks],
                     1e-13, 1e-15)
        got, want = ref.masked_mean(g['arr'], g['mask'], ks, False), g['mean_nofill_k%d' % ks]
        assert np.array_equal(np.isnan(got), np.isnan(want))
        assert_close(np.nan_to_num(got), np.nan_to_num(want), 1e-13, 1e-15)
    assert_close(ref.masked_mean(g['arr'].astype(F32), g['mask'], 6), g['mean32_fill_k6'],
                 1e-6, 1e-7)
    for ks in (6, 11):
        same(ref.masked_median(g['arr'], g['mask'], ks), g['median_fill_k%d' % ks])
        same(ref.masked_median(g['arr'], g['mask'], ks, False), g['median_nofill_k%d' % ks])
    same(ref.masked_median(g['arr'].astype(F32), g['mask'], 6), g['median32_fill_k6'])
    for ks in (3, 6, 9):
        same(ref.nan_max(g['arr_nan'], ks), g['nanmax_k%d' % ks])


def test_closest_distance_and_position_uncertainty_golden():
    g = load_golden('render_uncertainty.npz')
    for ks in (4, 9):
        same(ref.closest_distance(g['cdd_arr'], ks), g['cdd_k%d' % ks])

    def close(got, want):
        assert np.array_equal(np.isnan(got), np.isnan(want))
        assert_close(np.nan_to_num(got), np.nan_to_num(want), 1e-12, 1e-12)
    close(ref.pos_intensity_unc(g['piu_img'], 1.5, 0.7, 3), g['piu_const_1p5_0p7_k7'])
    close(ref.pos_intensity_unc(g['piu_img'], 2, 2, 2), g['piu_const_2_2_k5'])
    close(ref.pos_intensity_unc(g['piu_img'], g['piu_sx'], g['piu_sy'], 3), g['piu_vari_k7'])
    close(ref.pos_intensity_unc(g['piu_u16'], 1, 1, 2), g['piu_u16_const_1_1_k5'])


def test_median_threshold_golden():
    g = load_golden('median_threshold.npz')
    for key, thr, cond in (('thr0p1_gt', 0.1, '>'), ('thr0p5_gt', 0.5, '>'),
                           ('thr0p05_lt', 0.05, '<')):
        out, ind = ref.median_threshold(g['img'], thr, 3, cond)
        same(out, g['out_' + key], key)
        same(ind, g['ind_' + key], key)
    out, ind = ref.median_threshold(g['img'].astype(F32), 0.1)
    same(out, g['out32_thr0p1_gt'])
    same(ind, g['ind32_thr0p1_gt'])
    out, ind = ref.median_threshold(g['img_zero'], 0.1)
    same(out, g['out_zero'])
    same(ind, g['ind_zero'])
    for size in (5, 4, 2, 7, 9):
        out, ind = ref.median_threshold(g['img'], 0.1, size)
        same(out, g['out_s%d' % size], size)
        same(ind, g['ind_s%d' % size], size)
    out, ind = ref.median_threshold(g['img'].astype(F32), 0.1, 5)
    same(out, g['out32_s5'])
    same(ind, g['ind32_s5'])


def test_var_y_gauss_golden():
    g = load_golden('var_y_gauss.npz')
    assert_close(ref.var_y_gauss(g['arr'], (0, 4), 1), g['out_0_4_1'], 1e-12, 1e-15)
    assert_close(ref.var_y_gauss(g['arr'], 3, 0), g['out_3_0'], 1e-12, 1e-15)
    assert_close(ref.var_y_gauss(g['arr_nan'], (0, 4), 1), g['out_nan_0_4_1'], 1e-12, 1e-15)
    assert_close(ref.var_y_gauss(g['arr'], (1, 3), 2, 'reflect'), g['out_1_3_2_reflect'],
                 1e-12, 1e-15)


# ------------------------------------------- the oracle at the GPU shapes ----
def test_local_std_oracle(oracle):
    """square windows: the oracle's standardDeviation2d takes no others"""
    for shape in sc.SMALL + sc.WIDE[1:]:
        for dt in sc.DTYPES:
            img = sc.frame('signed', shape, dt)
            blurred = sc.frame('signed', shape, dt, seed=8) * dt(0.5)
            for ks in (2, 3, 7, 11, 12, 31, 101) if shape in sc.SMALL else (4, 10):
                want = oracle.standardDeviation2d(img, ks, blurred)
                got = ref.local_std(img, blurred, (ks, ks))
                if dt is F64:
                    assert_close(got, want, 1e-11, 1e-14, '%s k%d' % (shape, ks))
                else:
                    assert_close(got, want, 2e-6, 1e-7, '%s k%d f32' % (shape, ks))


@pytest.mark.parametrize('fn', ['mean', 'median'])
def test_masked_filter_oracle(oracle, fn):
    windows = (2, 3, 64, 65, 66, 130) if fn == 'mean' else (2, 3, 33, 45)
    kinds = ('signed', 'quantised') if fn == 'mean' else ('special', 'nans')
    for shape in ((1, 1), (1, 70), (70, 1), (5, 63), (9, 64), (13, 65), (37, 130)):
        for dt in sc.DTYPES:
            for ks in windows:
                for mk in ('block', 'single'):
                    m = sc.mask(mk, shape, ks // 2)
                    for kind in kinds:
                        a = sc.frame(kind, shape, dt)
                        what = '%s %s k%d %s %s' % (fn, shape, ks, mk, kind)
                        for fill in (True, False):
                            want = oracle.maskedFilter(a.copy(), m, ks, fill, fn)
                            if fn == 'median':
                                same(ref.masked_median(a, m, ks, fill), want, what)
                            elif dt is F64:
                                assert_close(ref.masked_mean(a, m, ks, fill), want, 1e-13, 1e-15,
                                             what)
                            else:
                                assert_close(ref.masked_mean(a, m, ks, fill), want, 1e-6, 1e-7,
                                             what)


def test_nan_max_oracle(oracle):
    for shape in sc.SMALL:
        for dt in sc.DTYPES:
            for ks in (2, 19, 20, 53, 54):
                a = sc.nan_max_frame(shape, ks // 2, dt)
                same(ref.nan_max(a, ks), oracle.nan_maximum_filter(a, ks), '%s k%d' % (shape, ks))


def test_closest_distance_oracle(orc):
    n = 0
    for shape, name, ks, dt, with_orc in sc.closest_cases():
        if with_orc:
            a = sc.closest_frames(shape)[name]
            same(ref.closest_distance(a, ks, dt), orc.closestDirectDistance(a, ks, dt),
                 '%s %s k%d' % (shape, name, ks))
            n += 1
    assert n >= 20
    # what the frames are for: distances 254 and 255 along a row, and a diagonal neighbour just
    # inside the window (further than ksize, closer than 2 ksize) and just outside
    two = sc.closest_frames((5, 600))['two']
    assert two[2, 10] and two[0, 590]
    for ks, d254, d255 in ((254, 254, 508), (255, 254, 255), (253, 506, 506)):
        d = ref.closest_distance(two, ks, np.float64)
        assert d[2, 264] == d254 and d[2, 265] == d255
        assert d[4, 590 - ks] == np.sqrt(16 + ks * ks) and d[4, 590 - ks - 1] == 2 * ks


def test_pos_intensity_unc_oracle(oracle):
    for k in (1, 14, 15, 16):
        for shape in ((2 * k + 2, 2 * k + 3), (2 * k, 2 * k + 3), (37, 130)):
            for dt in sc.DTYPES:
                img = sc.piu_frame(shape, dt)
                sx, sy = sc.piu_sigma_maps(shape)
                for args in ((3.0, 1.25), (sx, sy)):
                    got = ref.pos_intensity_unc(img, args[0], args[1], k)
                    want = oracle.positionToIntensityUncertainty(img, args[0], args[1], 2 * k + 1)
                    assert np.array_equal(np.isnan(got), np.isnan(want))
                    assert_close(np.nan_to_num(got), np.nan_to_num(want), 1e-12, 1e-12,
                                 '%s k%d' % (shape, k))
                    if shape[0] <= 2 * k:
                        assert not got.any()


def test_median_threshold_oracle(oracle):
    for shape in ((1, 1), (1, 70), (70, 1), (2, 3), (5, 63)):
        for dt in sc.DTYPES:
            for kind in ('zeros', 'spiky'):
                img = sc.median_threshold_frame(kind, shape, dt)
                for size in (2, 3, 4, 5, 9):
                    for cond in '><':
                        out, hit = ref.median_threshold(img, 0.2, size, cond)
                        want, whit = oracle.medianThreshold(img, 0.2, size, cond)
                        what = '%s %s s%d %s' % (shape, kind, size, cond)
                        same(out, want, what)
                        same(hit, whit, what)


def test_var_y_gauss_oracle(oracle):
    for shape in ((37, 130), (50, 257)):
        for dt in sc.DTYPES:
            a = sc.var_y_frame(shape, dt)
            for ky, stdx, modex in ((27, 1, 'wrap'), (29, 0, 'reflect'), (59, 3, 'wrap')):
                rng = (0.5, sc.stdy_for(ky))
                assert ref.var_y_sizes(rng, stdx)[2] == ky
                got = ref.var_y_gauss(a, rng, stdx, modex)
                want = oracle.varYSizeGaussianFilter(a, rng, stdx, modex)
                tol = 1e-12 if dt is F64 else 2e-6
                assert_close(got, want, tol, tol, '%s ky%d' % (shape, ky))


# ------------------------------------------------- the selection table ----
def test_path_table():
    """the last window of a path and the first of the next, per entry point and dtype, as the
    launchers decide them (the query is the code they call)"""
    P = sc.path
    for dt in sc.DTYPES:
        # local_std: square half windows 1..5 -> wave kernel; then the 48 KiB tile; then generic
        assert [P('local_std', dt, k, k) for k in (2, 3, 11, 12, 13)] == [1, 1, 1, 2, 2]
        assert [P('local_std', dt, *k) for k in ((3, 9), (9, 3), (2, 40))] == [2, 2, 2]
        assert P('local_std', dt, 1, 5) == sc.REFUSED
        assert sc.boundary('masked_mean_fill', dt) == (65, 66)     # ksize / 2 == 32 | 33
        assert sc.boundary('closest_distance', dt, lo=1) == (254, 255)
        assert sc.boundary('pos_intensity_unc', dt, lo=1) == (14, 15)   # half windows
        assert [P('median_threshold', dt, s) for s in (1, 2, 3, 4, 9)] == [2, 2, 1, 2, 2]
    es = {F32: 4, F64: 8}
    for dt, tile_last, med_last, nanmax_last in ((F32, 81, 45, 53), (F64, 49, 33, 19)):
        assert [P('local_std', dt, k, k) for k in (tile_last, tile_last + 1)] == [2, 3]
        hk = tile_last // 2
        assert (64 + 2 * hk) * (4 + 2 * hk) * es[dt] <= 48 * 1024 < \
            (64 + 2 * hk + 2) * (4 + 2 * hk + 2) * es[dt]
        assert sc.boundary('masked_median', dt) == (med_last, med_last + 1)
        assert P('masked_median', dt, med_last + 1) == sc.REFUSED
        assert sc.boundary('nan_max', dt) == (nanmax_last, nanmax_last + 1)
    assert 4 * 2 * 4 * 16 * 16 * 8 == 64 * 1024   # float64 ksize 33: the LDS limit exactly
    assert P('local_std', F32, 101, 101) == sc.STD_GENERIC
    # var_y_gauss: tiled below, expanded table above; the boundary moves with kx and dtype
    for dt in sc.DTYPES:
        last = [sc.var_y_boundary(dt, kx) for kx in (1, 3, 5, 7)]
        for (a, b), kx in zip(last, (1, 3, 5, 7)):
            assert P('var_y_gauss', dt, kx, a) == sc.VYG_TILED
            assert P('var_y_gauss', dt, kx, b) in (sc.VYG_EXPANDED_TILE, sc.VYG_EXPANDED_GENERIC)
            assert P('var_y_gauss', dt, kx, b) == 1 + P('conv_ydep', dt, kx, b)
        assert all(x[0] >= y[0] for x, y in zip(last, last[1:]))
    assert sc.var_y_boundary(F32, 3)[0] > sc.var_y_boundary(F64, 3)[0]
    # the comment of tests/test_gpu_configs.py::test_var_y_gauss_large_window: ky > 57 / > 27
    assert sc.var_y_boundary(F32, 3) == (57, 59) and sc.var_y_boundary(F64, 3) == (27, 29)
    assert P('var_y_gauss', F32, 4, 9) == sc.REFUSED and P('var_y_gauss', F32, 3, 8) == sc.REFUSED
    from imgprocessor_amd import _lib
    assert _lib.lib().ipa_stencil_path(99, _lib.F32, 3, 3) == -1
    assert P('nan_max', np.float32, 1) == sc.REFUSED
