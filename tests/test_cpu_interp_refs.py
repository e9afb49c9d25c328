"""CPU: the plain references of tests/interp_ref.py against the reference project's own
fixtures and against the C oracle on every case of tests/test_gpu_interp_paths.py, the table of
ipa_interp_path with every boundary pair on two sides, and the multiply-shift that replaces
t / ny checked exhaustively - so that a difference on the GPU is a kernel against references
that already agree, standing on a boundary that is known to be one.

The oracle sums in raster order in float64: it is held to the same bound as the kernels
(interp_ref.bound_rel with the window as ONE lane's share, n additions instead of n / 64).
"""
import numpy as np
import pytest

from . import interp_ref as ref
from . import interp_cases as ic
from .conftest import load_golden, assert_close

F32, F64 = np.float32, np.float64
RES = {'linear': 1, 'cubic': 2, 'area': 3, 'lanczos4': 4}


def seq_bound(n, c, dt):
    """a raster-order float64 sum of n terms: n roundings per sum"""
    return (2.0 * (np.asarray(n, dtype=F64) + 1) + c) * ref.U64 + ref.u_of(dt)


# ------------------------------------------------------------------ fixtures ----
def test_fixtures_interp_more():
    g = load_golden('interp_more.npz')
    gx, gy = g['u_shape']
    for tag, (x, y, v) in (('int', (g['u_xi'], g['u_yi'], g['u_vi'])), ('flt', (g['u_xf'], g['u_yf'], g['u_vf']))):
        for p in (1, 2, 3):
            assert_close(ref.unstructured_idw(x, y, v, (gx, gy), p), g['u_%s_p%d' % (tag, p)], 1e-12, 0, tag)
    assert np.array_equal(ref.unstructured_idw_seq(g['u_xf'], g['u_yf'], g['u_vf'], (gx, gy), 2), g['u_flt_p2'])
    for name in ('sq', 'wide'):
        gr, m = g['c_grid_' + name], g['c_mask_' + name]
        cx, cy = g['c_centre_' + name]
        for kern, power, fr, fphi in ((5, 2, 1, 0.2), (15, 2, 1, 1), (7, 1, 2, 0.5)):
            key = 'c_%s_k%d_p%d_fr%g_fphi%g' % (name, kern, power, fr, fphi)
            out = ref.circular_idw(gr, m, kern, power, fr, fphi, float(cx), float(cy))[0]
            assert_close(out, g[key], 1e-12, 1e-15, key)
    for name, kern in (('sq', 5), ('tall', 4), ('wide', 6)):
        for power in (2, 1):
            key = 'x_%s_k%d_p%d' % (name, kern, power)
            out = ref.cross_avg(g['x_grid_' + name], g['x_mask_' + name], kern, power)[0]
            assert_close(out, g[key], 1e-12, 0, key)


def test_fixtures_point_spread():
    g = load_golden('point_spread.npz')
    for name in ('sq', 'wide'):
        for kern, power in ((5, 2), (3, 1), (8, 3)):
            out, m = ref.point_spread(g['ps_grid_' + name], g['ps_mask_' + name], kern, power, 10 ** 5)[:2]
            assert_close(out, g['ps_%s_k%d_p%d' % (name, kern, power)], 1e-11, 0, name)
            assert not m.any()
    out = ref.point_spread(g['ps_grid_edge'], g['ps_mask_edge'], 4, 2, 10 ** 5)[0]
    assert_close(out, g['ps_edge_k4_p2'], 1e-11, 0, 'edge')
    out = ref.point_spread(g['ps_grid_sq'].astype(F32), g['ps_mask_sq'], 5, 2, 10 ** 5)[0]
    assert_close(out, g['ps32_sq_k5_p2'], 2e-6, 0, 'float32')


def test_fixtures_fast_filter():
    g = load_golden('fast_filter.npz')
    n = 0
    for key in g:
        if not key.startswith('ff_') or 'smooth' in key:
            continue
        _, src, k, e, fn = key.split('_')
        ksize = int(k[1:])
        every = max(ksize // 3, 1) if e == 'eNone' else int(e[1:])
        img = g['img_nan' if src == 'nan' else 'img']
        # fastFilter itself replaces `every` by shape[0] // (shape[0] // every) before it forms
        # the windows, and returns the grid without its last row and column (it uses the loops'
        # last INDICES as sizes): the fixture is that crop
        every = img.shape[0] // (img.shape[0] // every)
        out = ref.fast_stat(img, ksize, every)[fn]
        want = g[key]
        assert want.shape == (out.shape[0] - 1, out.shape[1] - 1), key
        assert_close(out[:-1, :-1], want, 1e-13, 0, key)
        n += 1
    assert n == 20


def test_fixtures_resize():
    g = load_golden('cv_resize.npz')
    n = 0
    for key in g:
        parts = key.split('_')
        if parts[0] in ('img', 'aimg'):
            continue
        kind, tag, (dh, dw) = parts[0], parts[-2], map(int, parts[-1].split('x'))
        src = g[('aimg_' if kind == 'area' else 'img_') + tag]
        assert np.array_equal(ref.resize(src, (dh, dw), kind), g[key]), key
        n += 1
    assert n == 34


# ------------------------------------------------- the oracle at the GPU cases ----
@pytest.mark.parametrize('case', ic.U_CASES, ids=ic.u_id)
def test_unstructured_oracle(oracle, case):
    h, w, n, power = case
    x, y, v = ic.points(h, w, n)
    want = ic.u_ref(case)
    for dt in ic.DTYPES:
        got = oracle.interpolate2dUnstructuredIDW(x, y, v, np.zeros((h, w), dt), power)
        ic.check_rel(got, want, seq_bound(n, ref.c_ops('unstructured', power), dt), ic.u_id(case))
    if power == 2:
        got = oracle.interpolate2dUnstructuredIDW(x, y, v, np.zeros((h, w)), 2)
        assert np.array_equal(got, ref.unstructured_idw_seq(x, y, v, (h, w), 2))


def circular_vs_oracle(oracle, case, defect=None):
    g, w, k, power, fr, fphi, where, kind = case
    cx, cy = ic.c_centre(g, where)
    m = ic.c_mask(g, w, kind)
    for dt in ic.DTYPES:
        src = ic.grid((g, w)).astype(dt)
        want, written, nn, cang = ic.c_ref(case, dt) if defect is None else \
            ref.circular_idw(src, m, k, power, fr, fphi, cx, cy, defect)
        got = oracle.interpolateCircular2dStructuredIDW(src.copy(), m, k, power, fr, fphi, cx, cy)
        assert np.array_equal(got != src, written) or np.array_equal(got[~written], src[~written])
        assert np.array_equal(got[:, g:], src[:, g:]) and not written[:, g:].any()
        ic.check_rel(got, want, seq_bound(nn, ref.c_ops('circular', power) + cang, dt), ic.c_id(case))
        assert written.any() and (m[:g, :g] & ~written[:g, :g]).any() == (kind == 'dense')


@pytest.mark.parametrize('case', ic.C_CASES, ids=ic.c_id)
def test_circular_oracle(oracle, case):
    circular_vs_oracle(oracle, case)


def cross_vs_oracle(oracle, case, defect=None):
    h, w, k, power, kind = case
    m = ic.x_mask(h, w, kind)
    for dt in ic.DTYPES:
        src = ic.grid((h, w)).astype(dt)
        want, nmax = ic.x_ref(case, dt) if defect is None else ref.cross_avg(src, m, k, power, defect)
        got = oracle.interpolate2dStructuredCrossAvg(src.copy(), m, k, power)
        assert np.array_equal(got[~m], src[~m])
        ic.check_rel(got, want, seq_bound(nmax, ref.c_ops('cross', power), dt), ic.x_id(case))


@pytest.mark.parametrize('case', ic.X_CASES, ids=ic.x_id)
def test_cross_oracle(oracle, case):
    cross_vs_oracle(oracle, case)


def point_spread_vs_oracle(oracle, case, defect=None):
    h, w, k, power, it, kind = case
    for dt in ic.DTYPES:
        want, wm, nmax, sweeps, depth = ic.p_ref(case, dt) if defect is None else \
            ref.point_spread(ic.grid((h, w)).astype(dt), ic.p_mask(h, w, kind), k, power, it, defect)
        gg, mm = ic.grid((h, w)).astype(dt), ic.p_mask(h, w, kind).copy()
        oracle.interpolate2dStructuredPointSpreadIDW(gg, mm, k, power, it, copy=False)
        assert np.array_equal(mm, wm), 'the mask left behind differs'
        bnd = ic.p_bound(case, dt, nmax, depth) if it == 1 else ic.P_END_TOL[dt]
        if it == 1:   # the oracle's sums are sequential
            bnd = np.maximum(depth, 1) * (seq_bound(nmax, ref.c_ops('point_spread', power), dt) - ref.u_of(dt)) + ref.u_of(dt)
        ic.check_rel(gg, want, bnd, ic.p_id(case))
        if k == 0:
            assert np.array_equal(gg, ic.grid((h, w)).astype(dt)) and sweeps == 2


@pytest.mark.parametrize('case', ic.P_CASES, ids=ic.p_id)
def test_point_spread_oracle(oracle, case):
    point_spread_vs_oracle(oracle, case)


def stat_vs_oracle(oracle, case, defect=None):
    import ctypes as C
    h, w, k, every = case
    assert ic.q('stat_samples', k, every) == 64
    for dt in ic.DTYPES:
        img = ic.s_image(h, w, dt)
        want = ic.s_ref(case, dt) if defect is None else ref.fast_stat(img, k, every, defect)
        for f, fn in enumerate(ref.FNS):
            out = np.empty(want[fn].shape)
            rc = oracle.lib().orc_fast_filter_stat(oracle._p(img), oracle._dt(img), C.c_long(h), C.c_long(w),
                                                   C.c_long(k), C.c_long(every), C.c_int(f), oracle._p(out))
            assert rc == 0
            if fn.endswith('median'):
                assert np.array_equal(out, want[fn], equal_nan=True), fn
            else:
                ic.check_rel(out, want[fn], seq_bound(4096, ref.c_ops('stat', 2), F64), fn)
        assert np.isfinite(want['median']).any() and np.isnan(want['median']).any()


@pytest.mark.parametrize('case', ic.S_CASES, ids=lambda c: '%dx%d-k%d-e%d' % c)
def test_stat_oracle(oracle, case):
    stat_vs_oracle(oracle, case)


# ------------------------------------------------ the cases see the defects ----
@pytest.mark.parametrize('defect', sorted(ref.DEFECTS))
def test_defects_are_seen(oracle, defect):
    """interp_ref.DEFECTS: each subtly wrong variant of the reference, held against the oracle
    over the case list with the bounds of the tests above, must fail at least one case - were
    the kernel wrong in that way, the GPU module would say so"""
    what = ref.DEFECTS[defect]
    run, cases = {'circular': (circular_vs_oracle, ic.C_CASES), 'cross average': (cross_vs_oracle, ic.X_CASES),
                  'point spread': (point_spread_vs_oracle, ic.P_CASES),
                  'statistics': (stat_vs_oracle, ic.S_CASES)}[what.split(':')[0]]
    for case in cases[::-1]:      # (the special cases stand at the end of the lists)
        try:
            run(oracle, case, defect)
        except AssertionError:
            return
    raise AssertionError('no case notices: ' + what)


@pytest.mark.parametrize('case', ic.R_CASES, ids=ic.r_id)
def test_resize_oracle(oracle, case):
    kind, ss, ds = case
    for dt in ic.DTYPES:
        got = oracle.resize(ic.r_image(ss, dt), ds, RES[kind])
        assert np.array_equal(got, ic.r_ref(case, dt)), '%s %s' % (ic.r_id(case), np.dtype(dt).name)


# -------------------------------------------------------------- the table ----
def test_query_table():
    assert ic.const('cross_seg') == 16 and ic.const('cross_ballot_steps') == 8
    assert ic.const('cross_search_pass') == 64 and ic.const('fastdiv_shift') == 20
    assert ic.const('ps_waves') == 16 and ic.const('ps_max_rows') == 16000
    assert ic.const('stat_max') == 4096 == 64 * 64
    for what, a, b in ic.boundary_table():
        assert a != b and a >= 0 and b >= 0, (what, a, b)
    assert [ic.q('power', p) for p in (2, 1, 1.5, 3)] == [2, 1, 0, 0]
    assert [ic.q('stat_samples', *c[2:]) for c in ic.S_CASES] == [64, 64]
    assert [ic.q('stat_samples', *c[2:]) for c in ic.S_REFUSED] == [0, 0]
    assert ic.q('stat_samples', 30, 10) == 6
    f32 = ic.dt_id(F32)
    for dw, pad, off in ic.R_VEC:
        for dt in ic.DTYPES:
            es = np.dtype(dt).itemsize
            want = 1 if pad % 4 == 0 and (off * es) % (4 * es) == 0 else 2
            assert ic.q('resize_vec4', ic.dt_id(dt), dw, dw + pad, 4096 + off * es) == want
    assert ic.q('resize_vec4', 0, 256, 256, 0) == 0
    for kind, ss, ds in ic.R_AREA:
        assert ic.q('resize_area', ss[0], ss[1], ds[0], ds[1]) == 2
    for kind, ss, ds in ic.R_AREA_INT + ic.R_LIN_AREA:
        assert ic.q('resize_area', ss[0], ss[1], ds[0], ds[1]) == 1
    assert ic.q('resize_linear', 12, 514, 6, 257) == 1
    assert all(ic.q('resize_linear', c[1][0], c[1][1], c[2][0], c[2][1]) == 2 for c in ic.R_SEP)
    assert ic.q('const', 99) == -1
    from imgprocessor_amd import _lib
    assert _lib.lib().ipa_interp_path(99, 0.0, 0.0, 0.0, 0.0) == -1
    assert ic.q('cross_fastdiv', 0.5, 3) == -1
    # the whole windows of the k = 50 | 51 cases stand on the switch, in both kernels
    assert [ic.q('cross_fastdiv', (2 * k + 1) ** 2, 2 * k + 1) for k in (6, 50, 51, 70)] == [1, 1, 0, 0]
    assert [ic.q('circular_fastdiv', 2 * k, 2 * k) for k in (2, 50, 51, 65)] == [1, 1, 0, 0]
    assert ic.q('circular_fastdiv', 5, 0) == 0


def test_multiply_shift_is_exact():
    """for every ny up to 2048 - the widest window of the cases is 2 * 70 + 1 = 141 - and every t
    with t * ny < 2^20: (t * M) >> 20 == t // ny.  The kernels use it for t < nt under the
    predicate nt * ny < 2^20, so every t they form satisfies t * ny < 2^20.

    The first t beyond the limit, t0 = ceil(2^20 / ny): the quotient is still right there for
    every ny but one, 1025 (t0 = 1024) - a window 1025 columns wide, k >= 512.  For the windows
    of the cases, and for any window below that width, the limit is therefore merely
    conservative AT ITS FIRST STEP; further out it is not: the nearest wrong quotient for a window
    width that occurs lies a few dozen positions beyond t0 (printed)."""
    sh = ic.const('fastdiv_shift')
    widest = 2 * max(c[2] for c in ic.X_CASES + ic.C_CASES) + 1
    first_wrong, nearest = [], []
    for ny in range(1, 2049):
        M = ic.q('fastdiv_mul', ny)
        assert M == -(-(1 << sh) // ny)
        tmax = ((1 << sh) - 1) // ny            # the largest t with t * ny < 2^20
        t = np.arange(0, tmax + 1, dtype=np.uint64)
        assert np.array_equal((t * np.uint64(M)) >> np.uint64(sh), t // np.uint64(ny)), ny
        t2 = np.arange(tmax + 1, tmax + 1 + 4 * ny, dtype=np.uint64)
        bad = np.flatnonzero(((t2 * np.uint64(M)) >> np.uint64(sh)) != t2 // np.uint64(ny))
        if bad.size and bad[0] == 0:
            first_wrong.append(ny)
        if bad.size and ny <= widest:
            nearest.append((int(bad[0]) + 1, ny))
    assert first_wrong == [1025]
    assert all(ny > widest for ny in first_wrong)
    assert nearest, 'no window width of the cases ever gets a wrong quotient within 4 rows of the limit'
    print('first wrong quotient for the window widths of the cases (<= %d): %d positions beyond '
          'the limit, at ny = %d' % ((widest,) + min(nearest)))
