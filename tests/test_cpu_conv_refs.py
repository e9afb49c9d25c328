"""CPU: the plain reference of tests/conv_ref.py against scipy.ndimage, the C oracle and the
reference's own fixtures, at the cases and data of tests/test_gpu_conv_paths.py, and the
kernel-selection table of ipa_conv2d_dev / ipa_sepconv2d_dev through ipa_conv_path - so that a
difference on the GPU is a kernel against references that already agree, standing on a boundary
that is known to be one.

Every comparison is held to conv_ref.bound: (n + 2) u sum |k| |img|, the most any summation
order in the image's precision can be off.
"""
import numpy as np
import pytest

from . import conv_ref as ref
from . import conv_cases as cc
from .conftest import load_golden

F32, F64 = np.float32, np.float64


def _q(v, dt):
    return np.asarray(v, dtype=F64).astype(dt).astype(F64)


# ------------------------------------------ the oracle at the GPU cases ----
@pytest.mark.parametrize('case', cc.CONV_CASES, ids=cc.conv_id)
def test_conv2d_oracle(oracle, case):
    worst = 0.0
    for shape, (mode, mode_y) in cc.conv_runs(case):
        img, k, m = cc.conv_inputs(case, shape)
        want = ref.ref_conv2d(img, k, mode, cc.CVAL, mode_y, m)
        bnd = ref.bound(img, k, mode, cc.CVAL, mode_y, m)
        got = oracle.conv2d(img, k, mode, cc.CVAL, m, mode_y)
        assert got.dtype == img.dtype
        worst = max(worst, cc.compare(got, want, bnd, 'oracle %s %s %s/%s' % (
            cc.conv_id(case), shape, mode, mode_y)))
    print('conv2d %s: oracle at %.3f of the bound' % (cc.conv_id(case), worst))


@pytest.mark.parametrize('case', cc.SEP_CASES, ids=cc.sep_id)
def test_sepconv2d_oracle(oracle, case):
    dt, nky, nkx = case[:3]
    ky, kx = cc.sep_taps(nky, nkx)
    worst = 0.0
    for shape, (mode, mode_y) in cc.sep_runs(case):
        if mode_y is not None:
            continue   # the oracle takes one mode for both passes: scipy has the mixed pairs
        img = cc.frame(shape, dt)
        want = ref.ref_sepconv2d(img, ky, kx, mode, cc.CVAL)
        bnd = ref.bound(img, (ky, kx), mode, cc.CVAL)
        got = oracle.sepconv2d(img, ky, kx, mode, cc.CVAL)
        worst = max(worst, cc.compare(got, want, bnd, 'oracle %s %s %s' % (
            cc.sep_id(case), shape, mode)))
    print('sepconv2d %s: oracle at %.3f of the bound' % (cc.sep_id(case), worst))


# ------------------------------------------------ scipy at the GPU cases ----
@pytest.mark.parametrize('case', cc.CONV_CASES, ids=cc.conv_id)
def test_conv2d_scipy(case):
    """scipy.ndimage.correlate takes one mode: the mixed pairs are the oracle's to confirm"""
    ndi = pytest.importorskip('scipy.ndimage')
    dt = case[0]
    for shape, (mode, mode_y) in cc.conv_runs(case):
        if mode_y is not None:
            continue
        img, k, m = cc.conv_inputs(case, shape)
        got = ndi.correlate(img, _q(k, dt), mode=mode, cval=float(_q(cc.CVAL, dt)))
        if m is not None:
            got = np.where(m != 0, got, dt(0))
        assert got.dtype == img.dtype
        cc.compare(got, ref.ref_conv2d(img, k, mode, cc.CVAL, None, m),
                   ref.bound(img, k, mode, cc.CVAL, None, m),
                   'scipy %s %s %s' % (cc.conv_id(case), shape, mode))


@pytest.mark.parametrize('case', cc.SEP_CASES, ids=cc.sep_id)
def test_sepconv2d_scipy(case):
    """correlate1d per axis, the intermediate an array of the image dtype (gaussian_filter's
    own structure), one mode per axis"""
    ndi = pytest.importorskip('scipy.ndimage')
    dt, nky, nkx = case[:3]
    ky, kx = cc.sep_taps(nky, nkx)
    cv = float(_q(cc.CVAL, dt))
    for shape, (mode, mode_y) in cc.sep_runs(case):
        img = cc.frame(shape, dt)
        got = img
        if ky is not None:
            got = ndi.correlate1d(got, _q(ky, dt), axis=0, mode=mode_y or mode, cval=cv)
        if kx is not None:
            got = ndi.correlate1d(got, _q(kx, dt), axis=1, mode=mode, cval=cv)
        assert got.dtype == img.dtype
        cc.compare(got, ref.ref_sepconv2d(img, ky, kx, mode, cc.CVAL, mode_y),
                   ref.bound(img, (ky, kx), mode, cc.CVAL, mode_y),
                   'scipy %s %s %s/%s' % (cc.sep_id(case), shape, mode, mode_y))


def test_even_and_tiny_exact_in_float64():
    """float64, frames below the radius, even and odd kernels, every mode: the reference and
    scipy sum the same products - what differs is the order at most"""
    ndi = pytest.importorskip('scipy.ndimage')
    for shape in ((1, 1), (1, 7), (2, 3), (3, 2), (5, 4), (33, 17)):
        img = cc.frame(shape, F64)
        for kh, kw in ((3, 3), (7, 7), (13, 13), (6, 4), (3, 7), (1, 9), (9, 1), (4, 4)):
            k = cc.kernel2d(kh, kw)
            for mode in cc.MODES:
                want = ndi.correlate(img, k, mode=mode, cval=cc.CVAL)
                cc.compare(ref.ref_conv2d(img, k, mode, cc.CVAL), want,
                           ref.bound(img, k, mode, cc.CVAL), '%s %dx%d %s' % (shape, kh, kw, mode))


def test_nonfinite_pattern(oracle):
    """IEEE: 0 x inf is NaN, so an exact-zero tap over an inf gives NaN - in the reference and
    in the oracle.  (scipy's N-D correlate drops zero weights from its footprint and is no
    yardstick here; its correlate1d keeps them.)"""
    for dt in cc.DTYPES:
        img = cc.nonfinite_frame((33, 129), dt, 13)
        assert np.isnan(img).sum() == 2 and np.isinf(img).sum() == 2
        k = cc.kernel2d(13, 13)
        want = ref.ref_conv2d(img, k, 'constant', cc.CVAL)
        # the pixel whose zero tap k[0, 12] lies on the +inf at (16, 18)
        assert np.isposinf(img[16, 18]) and k[0, 12] == 0.0 and np.isnan(want[22, 12])
        assert np.isnan(want).sum() > 13 * 13 and np.isinf(want).any()
        cc.compare(oracle.conv2d(img, k, 'constant', cc.CVAL), want,
                   ref.bound(img, k, 'constant', cc.CVAL), 'non-finite %s' % dt)
        ky, kx = cc.sep_taps(11, 11)
        cc.compare(oracle.sepconv2d(img, ky, kx, 'constant', cc.CVAL),
                   ref.ref_sepconv2d(img, ky, kx, 'constant', cc.CVAL),
                   ref.bound(img, (ky, kx), 'constant', cc.CVAL), 'non-finite sep %s' % dt)


# ------------------------------------------------------------- goldens ----
def test_goldens():
    """scipy's own outputs (float64 weights, float32 store): the rounding of the weights and
    the store are the + 2 of the bound"""
    from imgprocessor_amd.ops import gaussian_kernel1d
    g = load_golden('remap_scipy.npz')
    img = g['img']

    def dense(k, key, mode='reflect', cval=0.0):
        cc.compare(g[key], ref.ref_conv2d(img, k, mode, cval), ref.bound(img, k, mode, cval), key)
    dense(g['k7'], 'corr_k7')
    dense(g['k11'], 'corr_k11')
    dense(g['k7'][:3, :], 'corr_k3x7')
    dense(g['k7'][:6, :4], 'corr_k6x4')
    for mode in ('nearest', 'mirror', 'wrap', 'constant'):
        dense(g['k7'], 'corr_k7_' + mode, mode, 0.25)

    def gauss(a, sig, key):
        ky, kx = gaussian_kernel1d(sig[0]), gaussian_kernel1d(sig[1])
        cc.compare(g[key], ref.ref_sepconv2d(a, ky, kx), ref.bound(a, (ky, kx)), key)
    for s in (0.5, 1.0, 1.25, 2.0):
        gauss(img, (s, s), 'gauss_s%s' % str(s).replace('.', 'p'))
    gauss(img, (1.0, 2.5), 'gauss_s1_2p5')
    gauss(img.astype(F64), (1.0, 1.0), 'gauss64_s1')


# ------------------------------------------------- the selection table ----
def test_path_table():
    """every case of the GPU module on the path it claims, every boundary pair on two, as the
    launchers decide them (the query is the code they call)"""
    for c in cc.CONV_CASES:
        assert cc.path('conv2d', *c[:4]) == c[4], cc.conv_id(c)
    for c in cc.SEP_CASES:
        assert cc.path('sepconv2d', *c[:3]) == c[3], cc.sep_id(c)
    for a, b in cc.CONV_BOUNDARIES:
        pa, pb = cc.path('conv2d', *a), cc.path('conv2d', *b)
        assert pa != pb and pa != cc.REFUSED and pb != cc.REFUSED, (a, b)
    for a, b in cc.SEP_BOUNDARIES:
        pa, pb = cc.path('sepconv2d', *a), cc.path('sepconv2d', *b)
        assert pa != pb and pa != cc.REFUSED and pb != cc.REFUSED, (a, b)
    # big_wave == 0 moves 9 and 11 only; a mask moves every size
    assert [cc.path('conv2d', F32, K, K, cc.BIG_WAVE_OFF) for K in (3, 5, 7)] == [cc.WAVE] * 3
    assert cc.path('conv2d', F64, 9, 9, cc.BIG_WAVE_OFF) == cc.GENERIC
    # refusals, and the end of the generic kernel (65536 taps)
    from imgprocessor_amd import _lib
    L = _lib.lib()
    assert L.ipa_conv_path(99, _lib.F32, 3, 3, 0) == -1
    for dt in (_lib.U8, _lib.U16):
        assert L.ipa_conv_path(_lib.CONV_CONV2D, dt, 3, 3, 0) == cc.REFUSED
        assert L.ipa_conv_path(_lib.CONV_SEPCONV2D, dt, 3, 3, 0) == cc.REFUSED
    assert cc.path('conv2d', F32, 0, 3) == cc.REFUSED
    assert [cc.path('conv2d', F64, 256, k) for k in (256, 257)] == [cc.GENERIC, cc.REFUSED]
    # even tap counts: refused where they are short, accepted where the generic kernel runs them
    for dt in cc.DTYPES:
        assert [cc.path('sepconv2d', dt, *t) for t in ((4, 4), (4, 0), (3, 4), (62, 3))] == \
            [cc.REFUSED] * 4
        assert cc.path('sepconv2d', dt, 64, 0) == cc.SEP_ONE_GENERIC
        assert cc.path('sepconv2d', dt, 0, 64) == cc.SEP_ONE_GENERIC
        assert cc.path('sepconv2d', dt, 64, 64) == cc.SEP_TWO_GENERIC
        assert cc.path('sepconv2d', dt, 0, 0) == cc.SEP_LDS


def test_lds_boundaries():
    """the boundaries of the LDS-separable kernel recomputed from the library's byte formula:
    float32 equal taps opt in to more than 64 KiB between 33 and 35 and leave at 65 (the tap
    table, not the 150 KiB); float64 opts in always and leaves between 45 and 47"""
    OPT_IN, GIVE_UP, MAX_TAPS = 64 * 1024, 150 * 1024, 63
    odd = range(3, 200, 2)
    lds = {dt: {n: cc.sep_lds_bytes(dt, n, n) for n in odd} for dt in cc.DTYPES}
    for dt in cc.DTYPES:
        assert all(lds[dt][n] < lds[dt][n + 4] for n in odd if n + 4 in lds[dt])
    assert cc.sep_lds_bytes(F64, 3, 3) == 71808
    assert all(2 * lds[F32][n] == lds[F64][n] for n in odd)

    def expected(dt, n):
        if n > MAX_TAPS or lds[dt][n] > GIVE_UP:
            return cc.SEP_TWO_GENERIC
        if dt is F32 and n <= 9:
            return cc.SEP_WAVE
        return cc.SEP_LDS if lds[dt][n] <= OPT_IN else cc.SEP_LDS_BIG
    for dt in cc.DTYPES:
        for n in odd:
            assert cc.path('sepconv2d', dt, n, n) == expected(dt, n), (dt, n)
    last = {dt: {lim: max((n for n in odd if lds[dt][n] <= lim), default=None) for lim in (OPT_IN, GIVE_UP)}
            for dt in cc.DTYPES}
    assert last[F32][OPT_IN] == 33
    assert last[F32][GIVE_UP] > MAX_TAPS           # float32 leaves by the tap table: 63 | 65
    assert [expected(F32, n) for n in (33, 35, 63, 65)] == [
        cc.SEP_LDS, cc.SEP_LDS_BIG, cc.SEP_LDS_BIG, cc.SEP_TWO_GENERIC]
    assert last[F64][OPT_IN] is None and min(lds[F64].values()) > OPT_IN         # float64: every 2-D call opts in
    assert last[F64][GIVE_UP] == 45
    assert [expected(F64, n) for n in (45, 47)] == [cc.SEP_LDS_BIG, cc.SEP_TWO_GENERIC]
    assert all(cc.path('sepconv2d', F64, n, n) >= cc.SEP_LDS_BIG for n in odd)
    # unequal taps: (45, 3) has the tallest tile, (3, 45) the widest; both within 150 KiB
    for t in ((45, 3), (3, 45)):
        assert OPT_IN < cc.sep_lds_bytes(F64, *t) <= GIVE_UP
    # the largest accepted configurations fill most of a CU's 160 KiB
    assert lds[F64][45] > 140 * 1024
