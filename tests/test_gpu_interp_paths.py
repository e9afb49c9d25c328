"""GPU: every kernel of csrc/interp_more.hip and csrc/resize.hip on both sides of each of its
boundaries, against the plain references of tests/interp_ref.py (which tests/
test_cpu_interp_refs.py holds against the C oracle and the reference project's fixtures first).
Cases and data: tests/interp_cases.py; every boundary is read from ipa_interp_path.  The cases
run through the package's own functions (imgprocessor_amd.interpolate, ops.resize,
ops.fast_filter_stat) on host arrays; the C ABI is called directly where those do not reach: row
pitches, a destination pointer off its alignment.

Bounds.  Integer decisions are exact: masks, which pixels are written, medians, refusals.
Resize is bit for bit.  A weighted mean sum(w v) / sum(w) over n window positions with positive
terms is within (2 (ceil(n / 64) + 6) + c) u64 + u_T of the reference, relative: two sums, each
ceil(n / 64) additions per lane and 6 for the butterfly, c roundings in one term on both sides,
u_T the store into the grid's type.  Counted c (interp_ref.c_ops; pow within 2 ulp = 4 u):
  scattered points  2 (5 + w + 1): two differences, two squares, their sum, the weight, w v
  point spread      2 (w + 1): the squared distance is an exact integer
  circular          2 (10 power + w + 1) + c_angle: radii are the same correctly rounded
                    operations on both sides; the angles are not (atan2, 3 ulp between the two),
                    and |PHI - nphi| cancels: c_angle is that error carried to the mean, first
                    order, per pixel (interp_ref.circular_idw)
  cross average     15: the window sum and its division, then 3 products, 2 sums and a pow of
                    the blend, which runs in the grid's type on both sides
  window mean       1
with w = 1 (power 2), 2 (power 1), 5 (pow).  A single point-spread sweep feeds fills into later
windows: a pixel that rests on a chain of L fills gets L times the double part.  Runs to the
end keep the 1e-10 / 3e-6 of tests/test_gpu_interp_more.py.  float64 scattered points at power 2
are the reference's own arithmetic: array_equal against the sequential restatement.

The worst err / bound per kernel is printed by the last test of the module.
"""
import ctypes as C

import numpy as np
import pytest

from . import interp_ref as ref
from . import interp_cases as ic

pytestmark = pytest.mark.gpu

F32, F64 = np.float32, np.float64
WORST = {}
RES = {'linear': 1, 'cubic': 2, 'area': 3, 'lanczos4': 4}


@pytest.fixture(scope='module')
def ctx():
    import imgprocessor_amd
    return imgprocessor_amd.default_context(0)   # raises without a gfx950 device: no fallback


@pytest.fixture(scope='module')
def fills(ctx):
    from imgprocessor_amd import interpolate
    return interpolate


def note(name, dt, ratio):
    key = '%s %s' % (name, np.dtype(dt).name)
    WORST[key] = max(WORST.get(key, 0.0), ratio)
    return ratio


def bits(a):
    a = np.ascontiguousarray(a)
    return a.view(np.uint32 if a.dtype == F32 else np.uint64)


def embed(a, pitch, fill=ic.GUARD):
    """(h, w) -> (h + 2, pitch): a in the top-left corner, the guard value everywhere else"""
    h, w = a.shape
    big = np.full((h + 2, pitch), fill, a.dtype)
    big[:h, :w] = a
    return big


def guard_ok(big, h, w, fill=ic.GUARD):
    return (big[h:, :] == fill).all() and (big[:, w:] == fill).all()


def _dp(v):
    v = np.ascontiguousarray(v, dtype=F64)
    return v, v.ctypes.data_as(C.POINTER(C.c_double))


# the six *_dev entry points: grid `a` (h, w) inside a buffer of row pitch `pitch`
def run_unstructured(ctx, a, pitch, x, y, v, power):
    h, w = a.shape
    d = ctx.to_device(embed(a, pitch))
    (x, px), (y, py), (v, pv) = _dp(x), _dp(y), _dp(v)
    ctx._check(ctx._lib.ipa_unstructured_idw_dev(ctx.handle, d.ptr, ic.dt_id(a.dtype), h, w, pitch, px, py,
                                                 pv, v.size, float(power)), 'unstructured')
    return d.get()


def run_circular(ctx, a, pitch, m, k, power, fr, fphi, cx, cy):
    h, w = a.shape
    d, dm = ctx.to_device(embed(a, pitch)), ctx.to_device(np.ascontiguousarray(m, dtype=np.uint8))
    ctx._check(ctx._lib.ipa_circular_idw_fill_dev(ctx.handle, d.ptr, ic.dt_id(a.dtype), dm.ptr, h, w, pitch,
                                                  k, float(power), fr, fphi, cx, cy), 'circular')
    assert np.array_equal(dm.get(), m.astype(np.uint8))
    return d.get()


def run_cross(ctx, a, pitch, m, k, power):
    h, w = a.shape
    d, dm = ctx.to_device(embed(a, pitch)), ctx.to_device(np.ascontiguousarray(m, dtype=np.uint8))
    ctx._check(ctx._lib.ipa_cross_avg_fill_dev(ctx.handle, d.ptr, ic.dt_id(a.dtype), dm.ptr, h, w, pitch, k,
                                               float(power)), 'cross')
    assert np.array_equal(dm.get(), m.astype(np.uint8))
    return d.get()


def run_point_spread(ctx, a, pitch, m, k, power, it, status=False):
    h, w = a.shape
    d, dm = ctx.to_device(embed(a, pitch)), ctx.to_device(np.ascontiguousarray(m, dtype=np.uint8))
    rc = ctx._lib.ipa_point_spread_idw_dev(ctx.handle, d.ptr, ic.dt_id(a.dtype), dm.ptr, h, w, pitch, k,
                                           float(power), int(it))
    if status:
        return rc, d.get(), dm.get()
    ctx._check(rc, 'point spread')
    return d.get(), dm.get().astype(bool)


def run_stat(ctx, a, pitch, k, every, fn, status=False):
    h, w = a.shape
    n0, n1 = -(-h // every), -(-w // every)
    d, do = ctx.to_device(embed(a, pitch)), ctx.to_device(np.full((n0 + 1, n1), ic.GUARD))
    rc = ctx._lib.ipa_fast_filter_stat_dev(ctx.handle, d.ptr, ic.dt_id(a.dtype), h, w, pitch, k, every, fn,
                                           do.ptr)
    if status:
        return rc, do.get()
    ctx._check(rc, 'stat')
    out = do.get()
    assert (out[n0:] == ic.GUARD).all(), 'wrote outside'
    return out[:n0]


def run_resize(ctx, a, sp, ds, dp, kind, off=0):
    """-> the destination buffer (dh + 2, dp) as a flat array from element `off` on"""
    (sh, sw), (dh, dw) = a.shape, ds
    d = ctx.to_device(embed(a, sp, 1e30))
    do = ctx.to_device(np.full((dh + 2) * dp + off, ic.GUARD, a.dtype))
    ptr = C.cast(do.ptr, C.c_void_p).value + off * a.dtype.itemsize
    ctx._check(ctx._lib.ipa_resize_dev(ctx.handle, d.ptr, ic.dt_id(a.dtype), sh, sw, sp, C.c_void_p(ptr),
                                       dh, dw, dp, RES[kind]), 'resize')
    flat = do.get()
    assert (flat[:off] == ic.GUARD).all(), 'wrote before the destination'
    return flat[off:].reshape(dh + 2, dp), ptr


# ---------------------------------------------------------- scattered points ----
@pytest.mark.parametrize('case', ic.U_CASES, ids=ic.u_id)
def test_unstructured(fills, case):
    h, w, n, power = case
    assert ic.q('power', power) == ref.pick(power)
    x, y, v = ic.points(h, w, n)
    want = ic.u_ref(case)
    for dt in ic.DTYPES:
        got = np.zeros((h, w), dt)
        assert fills.interpolate2dUnstructuredIDW(x, y, v, got, power) is got
        note('unstructured_idw p%s' % ref.pick(power), dt,
             ic.check_rel(got, want, ref.bound_rel(n, ref.c_ops('unstructured', power), dt), ic.u_id(case)))
        if dt is F64 and power == 2:
            assert np.array_equal(got, ref.unstructured_idw_seq(x, y, v, (h, w), 2))


# ------------------------------------------------------------------ circular ----
@pytest.mark.parametrize('case', ic.C_CASES, ids=ic.c_id)
def test_circular(fills, case):
    g, w, k, power, fr, fphi, where, kind = case
    cx, cy = ic.c_centre(g, where)
    m = ic.c_mask(g, w, kind)
    fast = ic.q('circular_fastdiv', min(2 * k, g), min(2 * k, g))
    for dt in ic.DTYPES:
        src = ic.grid((g, w)).astype(dt)
        want, written, nn, cang = ic.c_ref(case, dt)
        got = fills.interpolateCircular2dStructuredIDW(src.copy(), m, k, power, fr, fphi, cx, cy)
        assert np.array_equal(bits(got[~written]), bits(src[~written])), 'a pixel that must stay was written'
        note('circular_idw %s p%s' % ('mul-shift' if fast else 'division', ref.pick(power)), dt,
             ic.check_rel(got, want, ref.bound_rel(nn, ref.c_ops('circular', power) + cang, dt), ic.c_id(case)))


# ------------------------------------------------------------- cross average ----
@pytest.mark.parametrize('case', ic.X_CASES, ids=ic.x_id)
def test_cross(fills, case):
    h, w, k, power, kind = case
    m = ic.x_mask(h, w, kind)
    fast = ic.q('cross_fastdiv', min(2 * k + 1, h) * min(2 * k + 1, w), min(2 * k + 1, w))
    for dt in ic.DTYPES:
        src = ic.grid((h, w)).astype(dt)
        want, nmax = ic.x_ref(case, dt)
        got = fills.interpolate2dStructuredCrossAvg(src.copy(), m, k, power)
        assert np.array_equal(bits(got[~m]), bits(src[~m])), 'an unmasked pixel was written'
        note('cross_avg %s' % ('mul-shift' if fast else 'division'), dt,
             ic.check_rel(got, want, ref.bound_rel(nmax, ref.c_ops('cross', power), dt), ic.x_id(case)))


# --------------------------------------------------------------- point spread ----
@pytest.mark.parametrize('case', ic.P_CASES, ids=ic.p_id)
def test_point_spread(fills, case):
    h, w, k, power, it, kind = case
    for dt in ic.DTYPES:
        src = ic.grid((h, w)).astype(dt)
        want, wm, nmax, sweeps, depth = ic.p_ref(case, dt)
        got, gm = src.copy(), ic.p_mask(h, w, kind).copy()
        assert fills.interpolate2dStructuredPointSpreadIDW(got, gm, k, power, maxIter=it, copy=False) is got
        assert np.array_equal(gm, wm), 'the mask left behind differs at %d pixels' % (gm != wm).sum()
        note('ps_sweep %s p%s' % ('one sweep' if it == 1 else 'run', ref.pick(power)), dt,
             ic.check_rel(got, want, ic.p_bound(case, dt, nmax, depth), ic.p_id(case)))
        if k == 0:
            assert np.array_equal(bits(got), bits(src))


def test_point_spread_row_limit(ctx, fills):
    """16000 x 2 runs (one LDS word per row: 64000 bytes), 16001 x 1 is refused before any launch"""
    from imgprocessor_amd import _lib
    lim = ic.const('ps_max_rows')
    assert ic.q('point_spread_rows', lim) == 1 and ic.q('point_spread_rows', lim + 1) == 0
    src = ic.grid((lim, 2))
    m = np.zeros((lim, 2), bool)
    for r in (0, 1, 15, 16, 17, 8000, lim - 2, lim - 1):
        m[r, r % 2] = True
    want, wm = ref.point_spread(src, m, 2, 2, ic.END)[:2]
    got, gm = src.copy(), m.copy()
    fills.interpolate2dStructuredPointSpreadIDW(got, gm, 2, 2, copy=False)
    assert np.array_equal(gm, wm) and not gm.any()
    note('ps_sweep run p2', F64, ic.check_rel(got, want, ic.P_END_TOL[F64], 'row limit'))
    src = ic.grid((lim + 1, 1))
    m = np.zeros((lim + 1, 1), bool)
    m[5] = True
    rc, g2, m2 = run_point_spread(ctx, src, 1, m, 2, 2, ic.END, status=True)
    assert rc == _lib.ERR_BAD_ARG
    assert np.array_equal(g2[:lim + 1], src) and np.array_equal(m2.astype(bool), m)
    got, gm = src.copy(), m.copy()
    with pytest.raises(ValueError):
        fills.interpolate2dStructuredPointSpreadIDW(got, gm, 2, 2, copy=False)
    assert np.array_equal(got, src) and np.array_equal(gm, m)


# ---------------------------------------------------------- window statistics ----
@pytest.mark.parametrize('case', ic.S_CASES, ids=lambda c: '%dx%d-k%d-e%d' % c)
def test_stat_at_the_lds_limit(ctx, case):
    from imgprocessor_amd import ops
    h, w, k, every = case
    assert ic.q('stat_samples', k, every) ** 2 == ic.const('stat_max')
    for dt in ic.DTYPES:
        img = ic.s_image(h, w, dt)
        want = ic.s_ref(case, dt)
        for f, fn in enumerate(ref.FNS):
            got = ops.fast_filter_stat(img, k, every, fn)
            if fn.endswith('median'):
                assert np.array_equal(got, want[fn], equal_nan=True), fn
            else:
                note('fast_filter_stat mean', dt, ic.check_rel(
                    got, want[fn], ref.bound_rel(ic.const('stat_max'), ref.c_ops('stat', 2), F64), fn))


@pytest.mark.parametrize('case', ic.S_REFUSED, ids=lambda c: '%dx%d-k%d-e%d' % c)
def test_stat_beyond_the_lds_limit(ctx, case):
    from imgprocessor_amd import _lib, ops
    h, w, k, every = case
    assert ic.q('stat_samples', k, every) == 0
    for dt in ic.DTYPES:
        rc, out = run_stat(ctx, ic.s_image(h, w, dt), w, k, every, 0, status=True)
        assert rc == _lib.ERR_UNSUPPORTED and (out == ic.GUARD).all()
        with pytest.raises(NotImplementedError):
            ops.fast_filter_stat(ic.s_image(h, w, dt), k, every, 'median')


# --------------------------------------------------------------------- resize ----
@pytest.mark.parametrize('case', ic.R_CASES, ids=ic.r_id)
def test_resize(ctx, case):
    from imgprocessor_amd import ops
    kind, ss, ds = case
    for dt in ic.DTYPES:
        got = ops.resize(ic.r_image(ss, dt), ds, kind)
        want = ic.r_ref(case, dt)
        assert got.dtype == want.dtype and got.shape == want.shape
        assert np.array_equal(bits(got), bits(want)), '%d values differ' % (bits(got) != bits(want)).sum()


@pytest.mark.parametrize('dw,pad,off', ic.R_VEC)
def test_resize_vertical_pass_choice(ctx, dw, pad, off):
    """dw % 4 == 0: vresize4_kernel | vresize_kernel by the destination's pitch and by its
    pointer, which kernel asked of the library with the pointer the call gets"""
    for kind in ('linear', 'lanczos4'):
        case = (kind, (5, 101), (7, dw))
        for dt in ic.DTYPES:
            got, ptr = run_resize(ctx, ic.r_image((5, 101), dt), 101 + 2, (7, dw), dw + pad, kind, off)
            es = np.dtype(dt).itemsize
            want_path = 1 if pad % 4 == 0 and (off * es) % (4 * es) == 0 else 2
            assert ic.q('resize_vec4', ic.dt_id(dt), dw, dw + pad, ptr) == want_path
            assert np.array_equal(bits(got[:7, :dw]), bits(ic.r_ref(case, dt)))
            assert guard_ok(got, 7, dw), 'wrote outside'


# ---------------------------------------------------------------------- pitch ----
@pytest.mark.parametrize('pad', [3, 8])
@pytest.mark.parametrize('op', ['unstructured', 'circular', 'cross', 'cross_division', 'point_spread',
                                'stat', 'resize_lanczos4', 'resize_area', 'resize_area_int'])
def test_pitch(ctx, op, pad):
    """every *_dev entry point with the grid inside a larger buffer: the bits of the contiguous
    call, the guard untouched (the mask, and the output of the statistics, have no pitch)"""
    for dt in ic.DTYPES:
        if op == 'unstructured':
            h, w = 9, 65
            x, y, v = ic.points(h, w, 257)
            f = lambda p: run_unstructured(ctx, np.zeros((h, w), dt), p, x, y, v, 1.5)
        elif op == 'circular':
            h, w = 65, 70
            a, m = ic.grid((h, w)).astype(dt), ic.c_mask(h, w, 'dense')
            f = lambda p: run_circular(ctx, a, p, m, 2, 2, 1.0, 0.2, 33.0, 33.0)
        elif op in ('cross', 'cross_division'):
            h, w, k, kind = (65, 33, 5, 'rand') if op == 'cross' else (103, 104, 51, 'few')
            a, m = ic.grid((h, w)).astype(dt), ic.x_mask(h, w, kind)
            f = lambda p: run_cross(ctx, a, p, m, k, 2)
        elif op == 'point_spread':
            h, w = 33, 65
            a, m = ic.grid((h, w)).astype(dt), ic.p_mask(h, w, 'rand')
            left = []

            def f(p):
                g, gm = run_point_spread(ctx, a, p, m, 3, 2, ic.END)
                left.append(gm)
                return g
        elif op == 'stat':
            h, w = 66, 68
            a = ic.s_image(h, w, dt)
            plain = run_stat(ctx, a, w, 32, 1, 3)
            assert np.array_equal(bits(run_stat(ctx, a, w + pad, 32, 1, 3)), bits(plain))
            continue
        else:
            kind, ss, ds = {'resize_lanczos4': ('lanczos4', (5, 101), (7, 260)),
                            'resize_area': ic.R_AREA[3], 'resize_area_int': ic.R_AREA_INT[3]}[op]
            a = ic.r_image(ss, dt)
            h, w = ds
            f = lambda p: run_resize(ctx, a, ss[1] + (p - w), ds, p, kind)[0]
        plain, got = f(w), f(w + pad)
        assert np.array_equal(bits(got[:h, :w]), bits(plain[:h, :w])), '%d values differ' % (
            bits(got[:h, :w]) != bits(plain[:h, :w])).sum()
        assert guard_ok(got, h, w) and guard_ok(plain, h, w), 'wrote outside'
        if op == 'point_spread':
            want_mask = ic.p_ref((h, w, 3, 2, ic.END, 'rand'), dt)[1]
            assert np.array_equal(left[0], want_mask) and np.array_equal(left[1], want_mask), \
                'the mask left behind differs'


def test_zz_report():
    """the figures of this run (reported values, not thresholds)"""
    print()
    for key in sorted(WORST):
        print('worst err / bound  %-40s %.3f' % (key, WORST[key]))
    assert all(v <= 1.0 for v in WORST.values())
