"""Grids, masks, points and case lists shared by tests/test_cpu_interp_refs.py (tests/interp_ref.py
against the C oracle, no GPU) and tests/test_gpu_interp_paths.py (every kernel of
csrc/interp_more.hip and csrc/resize.hip against interp_ref), and the query of the library
(ipa_interp_path: the constants and predicates the kernels and launchers call, no device needed).

Grids are small and ragged, values lie in [5, 11] (every bound is purely relative), masks reach
every edge.  Every boundary a case stands on is read from the query; BOUNDARIES pairs them.
"""
import functools

import numpy as np

from .stencil_cases import cached

F32, F64 = np.float32, np.float64
DTYPES = (F32, F64)
GUARD = -77.0        # what a pitched buffer holds outside the grid


def q(op, a=0, b=0, c=0, d=0):
    """ipa_interp_path for the op NAME ('cross_fastdiv', 'stat_samples', ...)"""
    from imgprocessor_amd import _lib
    return _lib.lib().ipa_interp_path(getattr(_lib, 'INTERP_' + op.upper()), float(a), float(b),
                                      float(c), float(d))


def const(name):
    from imgprocessor_amd import _lib
    return q('const', getattr(_lib, 'INTERP_K_' + name.upper()))


def dt_id(dt):
    from imgprocessor_amd.device import dtype_id
    return dtype_id(np.dtype(dt))


@cached
def grid(shape, seed=0):
    """float64 in [5, 11]; the float32 cases take its rounding"""
    h, w = shape
    return 5.0 + 6.0 * np.random.default_rng(300 + 17 * h + w + seed).random(shape)


def rmask(shape, dens, seed=0):
    h, w = shape
    return np.random.default_rng(500 + 13 * h + w + seed).random(shape) < dens


# ---------------------------------------------------------- scattered points ----
POWERS = (2, 1, 1.5, 3)
U_SHAPES = tuple((h, w) for w in (63, 64, 65) for h in (3, 4, 5, 9))     # the block is 64 x 4
U_CASES = tuple((h, w, n, POWERS[(3 * si + ni) % 4])
                for si, (h, w) in enumerate(U_SHAPES) for ni, n in enumerate((1, 2, 257)))


def u_id(c):
    return '%dx%d-n%d-p%g' % c


@cached
def points(h, w, n):
    """x (rows), y, v.  n = 1: one point on the last pixel.  n = 2: two points on ONE pixel, the
    first one's value counts.  n = 257: the first point on a pixel (the last of row 0), the
    second a duplicate of it, the last on a pixel (the first of the last row); a third of the
    rest on pixels, a third at fractional positions, a third outside the grid"""
    rng = np.random.default_rng(40 + 7 * h + w + n)
    v = 5.0 + 6.0 * rng.random(n)
    if n == 1:
        return np.array([h - 1.0]), np.array([w - 1.0]), v
    if n == 2:
        return np.array([1.0, 1.0]), np.array([2.0, 2.0]), v
    x = rng.integers(0, h, n).astype(F64)
    y = rng.integers(0, w, n).astype(F64)
    x[2::3] += rng.random(x[2::3].size) * 0.9 + 0.05
    y[2::3] += rng.random(y[2::3].size) * 0.9 + 0.05
    x[3::3] = np.where(rng.random(x[3::3].size) < 0.5, -1.0 - 3 * rng.random(x[3::3].size),
                       h + 3 * rng.random(x[3::3].size))
    y[3::6] = w + 2.5
    x[0], y[0] = 0.0, w - 1.0
    x[1], y[1] = x[0], y[0]
    x[-1], y[-1] = h - 1.0, 0.0
    return x, y, v


# ------------------------------------------------------------------ circular ----
# (g, w, k, power, fr, fphi, centre 'in' / 'out', mask 'dense' / 'sparse')
def _circ():
    out = []
    for gi, g in enumerate((63, 64, 65, 129)):
        for wi, extra in enumerate((0, 5)):
            out.append((g, g + extra, 1, 2, 1.0, 0.2, 'in' if wi else 'out', 'dense'))
            out.append((g, g + extra, 2, (1, 3)[(gi + wi) % 2], 0.5, 2.0, 'out' if wi else 'in', 'dense'))
    out += [(129, 129, 50, 2, 1.0, 1.0, 'in', 'sparse'), (129, 129, 51, 2, 1.0, 1.0, 'in', 'sparse'),
            (129, 134, 50, 1, 1.0, 0.3, 'out', 'sparse'), (129, 134, 51, 3, 2.0, 0.5, 'in', 'sparse'),
            (63, 63, 65, 2, 1.0, 0.2, 'in', 'sparse'), (64, 69, 70, 3, 1.0, 1.0, 'out', 'sparse'),
            (65, 65, 65, 1, 0.5, 1.0, 'in', 'sparse')]
    return tuple(out)


C_CASES = _circ()


def c_id(c):
    return 'g%d-w%d-k%d-p%g-%s-%s' % (c[0], c[1], c[2], c[3], c[6], c[7])


def c_centre(g, where):
    return (g // 2 + 1.0, g // 2 + 1.0) if where == 'in' else (-7.5, g + 3.25)


@cached
def c_mask(g, w, kind):
    """dense: 30 % to every edge and a 7 x 7 block (its middle sees nothing at k <= 2); sparse:
    a few dozen pixels - the interior pixel (g // 2, g // 2) whose window is whole at k = 50 / 51
    on the 129 grid, its neighbours, the corners and edge pixels.  Both: the pixel AT the centre
    (g // 2 + 1, g // 2 + 1), the ones next to it, and pixels on both sides of the +-pi cut of the
    angle (rows above the centre, the centre's column and the two beside it).  Columns >= g:
    every other one masked - they must stay as they are"""
    m = rmask((g, w), 0.3) if kind == 'dense' else np.zeros((g, w), bool)
    c = g // 2 + 1
    if kind == 'dense':
        m[10:17, 20:27] = True
        m[c - 6:c + 3, c - 3:c + 4] = False
    else:
        rng = np.random.default_rng(g + w)
        m[rng.integers(0, g, 24), rng.integers(0, g, 24)] = True
        for p in ((g // 2, g // 2), (g // 2, g // 2 + 1), (0, 0), (0, g - 1), (g - 1, 0), (g - 1, g - 1),
                  (0, g // 2), (g - 1, g // 3), (g // 3, 0), (g // 2, g - 1), (g - 1, g - 2)):
            m[p] = True
    for p in ((c, c), (c, c + 1), (c + 1, c), (c - 3, c), (c - 3, c - 1), (c - 3, c + 1), (c - 5, c - 1),
              (c - 5, c), (c - 4, c + 1)):
        m[p] = True
    m[c - 1, c] = m[c, c - 1] = False
    m[:, g:] = False
    m[:, g::2] = True
    return m


# ------------------------------------------------------------- cross average ----
# (h, w, k, power, mask kind)
def _cross():
    out = []
    ks = (0, 3, 4, 5, 6)
    n = 0
    for w in (15, 16, 17, 33, 65):
        for h in (1, 2, 65, 130):
            out.append((h, w, ks[n % 5], (2, 3)[n % 2], 'rand'))
            n += 1
    out += [(130, 132, 3, 2, 'steps'), (130, 132, 3, 3, 'steps'), (130, 132, 4, 3, 'stale'),
            (130, 132, 5, 2, 'stale'), (103, 104, 50, 2, 'few'), (103, 104, 51, 2, 'few'),
            (104, 103, 51, 3, 'few'), (65, 33, 70, 2, 'rand'), (130, 33, 6, 2, 'tall'),
            (1, 65, 32, 2, 'rand'), (2, 65, 32, 3, 'rand'), (3, 65, 21, 2, 'rand'),
            (5, 33, 6, 2, 'rand'), (9, 16, 7, 2, 'rand')]
    return tuple(out)


X_CASES = _cross()


def x_id(c):
    return '%dx%d-k%d-p%g-%s' % c


@cached
def x_mask(h, w, kind):
    """rand: 30 %, blocks that touch each edge and each corner (searches with nothing to find),
    a fully masked row, a row that starts masked (the stale slot).
    tall (h > w): rand, and the rows >= w - 1 half masked (the search towards the last column is
    skipped there).
    steps: a 65 x 65 hole - every distance 1 .. 65 in each of the four directions, 8 | 9 and
    64 | 65 among them - and blocks on every edge.
    stale: rows that start masked, with the last row that has a masked pixel right of an unmasked
    one 1, 17, 67 and 97 rows further up (the 64-row chunks of cross_prev_row_kernel and their
    carry), rows before any such row (no stale value: the slot is left out), rows whose first
    unmasked column is 70 (beyond one 64-column chunk of cross_row_last_kernel), a fully masked
    row.
    few: a dozen pixels around the middle, so that the pixels their searches find have whole
    windows at k = 50 / 51."""
    m = np.zeros((h, w), bool)
    if kind in ('rand', 'tall'):
        m = rmask((h, w), 0.3)
        if h > 4 and w > 8:
            m[:3, 2:5] = True
            m[h - 3:, w - 6:w - 3] = True
            m[h // 2:h // 2 + 3, :2] = True
            m[h // 3:h // 3 + 2, w - 2:] = True
            m[0, 0] = m[h - 1, w - 1] = True
            m[min(h // 2 + 6, h - 2), :] = True
            m[h // 4, :w // 3] = True
        if kind == 'tall':
            m[w - 1:, ::2] = True
        if not (~m).any():
            m[0, w // 2] = False
    elif kind == 'steps':
        m[32:97, 33:98] = True
        m[:9, 5:8] = True
        m[h - 9:, 110:113] = True
        m[100:103, :9] = True
        m[10:13, w - 9:] = True
    elif kind == 'stale':
        m[1, :3] = True            # no row before it has a value for the slot
        m[2, 0] = True
        m[3, 10] = True            # row 3: the value every stale slot below takes
        for r in (4, 20, 70, 100):
            m[r, :5] = True
        m[101, :70] = True         # first unmasked column 70, a masked pixel further right:
        m[101, 80] = True          # ITS search is the value of the rows below
        m[102, :3] = True
        m[110, :] = True           # a fully masked row
        m[111, :2] = True
        m[129, :4] = True          # last row: nothing below, the slot is not raised
    elif kind == 'few':
        r, c = h // 2, w // 2
        for p in ((r, c), (r, c + 1), (r + 1, c), (r + 3, c - 2), (r - 2, c + 3), (0, 0), (h - 1, w - 1),
                  (r, 0), (r, 1), (0, c), (h - 1, c)):
            m[p] = True
    return m


# --------------------------------------------------------------- point spread ----
# (h, w, k, power, max_iter, mask kind)
END = 10 ** 5


def _ps():
    out = []
    ks, ps = (1, 2, 3, 5), (2, 1, 2.5)
    n = 0
    for h in (15, 16, 17, 33):
        for w in (63, 64, 65, 129):
            out.append((h, w, ks[n % 4], ps[n % 3], (1, END)[n % 2], 'rand'))
            n += 1
    out += [(129, 17, 3, 2, 1, 'rand'), (100, 63, 2, 1, END, 'rand'), (65, 33, 5, 2.5, 1, 'rand'),
            (81, 65, 1, 2, 1, 'clusters'), (81, 65, 63, 2, 1, 'clusters'),
            (81, 65, 64, 1, 1, 'clusters'), (81, 65, 65, 2, 1, 'clusters'),
            (96, 129, 63, 2, END, 'clusters'), (96, 129, 64, 2, END, 'clusters'),
            (96, 129, 65, 3, END, 'clusters'), (130, 70, 64, 2, 1, 'clusters'),
            (33, 65, 0, 2, 2, 'rand'), (17, 65, 2, 2, END, 'one'), (16, 64, 3, 1, 1, 'one')]
    return tuple(out)


P_CASES = _ps()


def p_id(c):
    return '%dx%d-k%d-p%g-%s-%s' % (c[0], c[1], c[2], c[3], 'end' if c[4] == END else 'it%d' % c[4], c[5])


@cached
def p_mask(h, w, kind):
    """rand: 40 %, a hole, the first pixel unmasked, half of the last row and column masked (the
    -1 index of the border pass).  clusters: 5 x 9 blocks every 9 rows from top to bottom - border
    pixels in many consecutive rows, so that rows wait on rows - and a partly masked last row
    and column.  one: everything masked but ONE pixel"""
    if kind == 'one':
        m = np.ones((h, w), bool)
        m[h // 2, w // 3] = False
        return m
    rng = np.random.default_rng(900 + 3 * h + w)
    if kind == 'rand':
        m = rmask((h, w), 0.4, 3)
        m[h // 4:3 * h // 4, w // 4:3 * w // 4] = True
    else:
        m = np.zeros((h, w), bool)
        for n, r in enumerate(range(1, h - 5, 9)):
            c = (7 * n) % (w - 9)
            m[r:r + 5, c:c + 9] = True
    m[0, 0] = False
    m[:, -1] |= rng.random(h) < 0.5
    m[-1, :] |= rng.random(w) < 0.5
    return m


# ---------------------------------------------------------- window statistics ----
# (h, w, ksize, every): 64 samples per axis, interior windows whole (4096 values)
S_CASES = ((66, 68, 32, 1), (130, 132, 64, 2))
S_REFUSED = ((66, 68, 33, 1), (130, 132, 65, 2))      # 66 and 65 per axis


@cached
def s_image(h, w, dt):
    """values on a grid of 0.5 (ties; exact in float32), NaNs in two corners: the whole windows
    in the middle hold 4096 finite values, some of their neighbours a NaN"""
    a = (np.random.default_rng(60 + h + w).integers(10, 22, (h, w)) * 0.5).astype(dt)
    a[0, 0] = a[0, 1] = a[h - 1, w - 1] = np.nan
    return a


# --------------------------------------------------------------------- resize ----
R_WIDTHS = (255, 256, 257, 260, 513)     # the block is 256 result columns
# (kind, source shape, result shape)
R_SEP = tuple((kind, (5, 101), (7, dw)) for kind in ('linear', 'cubic', 'lanczos4') for dw in R_WIDTHS)
R_AREA = tuple(('area', (11, dw * 3 // 2 + 1), (7, dw)) for dw in R_WIDTHS)
# integer scales (isy, isx) with 1, 2, 3, 4, 5, 7 elements per result pixel
R_AREA_INT = tuple(('area', (6 * isy, 257 * isx), (6, 257))
                   for isy, isx in ((1, 1), (1, 2), (3, 1), (2, 2), (1, 5), (7, 1)))
R_TINY = tuple((kind, s, (5, 7)) for kind in ('linear', 'cubic', 'lanczos4') for s in ((1, 1), (2, 3)))
R_LIN_AREA = (('linear', (12, 514), (6, 257)),)      # the exact 2 x 2 reduction
R_CASES = R_SEP + R_AREA + R_AREA_INT + R_TINY + R_LIN_AREA
# dw % 4 == 0: (result width, pitch - width, destination offset in elements) -> vector | scalar
R_VEC = ((256, 0, 0), (256, 8, 0), (256, 3, 0), (256, 2, 0), (256, 0, 1), (256, 8, 1), (260, 0, 0),
         (260, 4, 0), (260, 1, 0), (260, 4, 1))


def r_id(c):
    return '%s-%dx%d-to-%dx%d' % (c[0], c[1][0], c[1][1], c[2][0], c[2][1])


@cached
def r_image(shape, dt):
    h, w = shape
    return (np.random.default_rng(80 + 5 * h + w).standard_normal(shape) * 3.0).astype(dt)


# ----------------------------------------------------------------- boundaries ----
def boundary_table():
    """-> [(what, value on one side, value on the other)] as the library answers; the CPU
    module asserts every pair to differ"""
    t = []
    t.append(('cross fastdiv, whole window k = 50 | 51', q('cross_fastdiv', 101 * 101, 101),
              q('cross_fastdiv', 103 * 103, 103)))
    t.append(('circular fastdiv, whole window k = 50 | 51', q('circular_fastdiv', 100, 100),
              q('circular_fastdiv', 102, 102)))
    t.append(('power 2 | 1', q('power', 2), q('power', 1)))
    t.append(('power 1 | 1.5', q('power', 1), q('power', 1.5)))
    t.append(('power 2 | 3', q('power', 2), q('power', 3)))
    t.append(('point spread rows 16000 | 16001', q('point_spread_rows', const('ps_max_rows')),
              q('point_spread_rows', const('ps_max_rows') + 1)))
    t.append(('statistics 64 | 66 per axis', q('stat_samples', 32, 1), q('stat_samples', 33, 1)))
    t.append(('statistics 64 | 65 per axis', q('stat_samples', 64, 2), q('stat_samples', 65, 2)))
    f32 = dt_id(F32)
    t.append(('vresize4 | vresize: width', q('resize_vec4', f32, 256, 256, 0), q('resize_vec4', f32, 257, 257, 0)))
    t.append(('vresize4 | vresize: pitch', q('resize_vec4', f32, 256, 264, 0), q('resize_vec4', f32, 256, 259, 0)))
    t.append(('vresize4 | vresize: pointer', q('resize_vec4', f32, 256, 256, 4096), q('resize_vec4', f32, 256, 256, 4100)))
    t.append(('float64 pointer 16 | 32 bytes', q('resize_vec4', dt_id(F64), 256, 256, 4096 + 32),
              q('resize_vec4', dt_id(F64), 256, 256, 4096 + 16)))
    t.append(('area integer | tables', q('resize_area', 12, 514, 6, 257), q('resize_area', 11, 385, 7, 256)))
    t.append(('area tables | refused', q('resize_area', 11, 385, 7, 256), q('resize_area', 5, 101, 7, 256)))
    t.append(('linear 2 x 2 | separable', q('resize_linear', 12, 514, 6, 257), q('resize_linear', 12, 514, 6, 256)))
    return t


# ----------------------------------------------------------------- comparison ----
def check_rel(got, want, bnd, what=''):
    """asserts |got - want| <= bnd |want| wherever want is finite, and the NaN pattern equal;
    -> the worst err / bound"""
    got, want = np.asarray(got, dtype=F64), np.asarray(want, dtype=F64)
    bnd = np.broadcast_to(np.asarray(bnd, dtype=F64), want.shape)
    assert got.shape == want.shape, (what, got.shape, want.shape)
    assert np.array_equal(np.isnan(got), np.isnan(want)), '%s: NaN pattern differs' % what
    fin = np.isfinite(want)
    if not fin.any():
        return 0.0
    err = np.abs(np.where(fin, got, 0.0) - np.where(fin, want, 0.0))
    lim = np.where(fin, bnd * np.abs(np.where(fin, want, 1.0)), 1.0)
    with np.errstate(divide='ignore', invalid='ignore'):   # (a reference of exactly 0 admits only 0)
        ratio = np.where(err == 0.0, 0.0, err / lim)
    worst = float(ratio.max())
    if worst > 1.0:
        i = np.unravel_index(np.argmax(ratio), ratio.shape)
        raise AssertionError('%s: %d of %d values beyond the bound, worst at %s: got %r want %r, '
                             'err %.3g = %.3g x bound' % (what, (ratio > 1.0).sum(), ratio.size, i,
                                                         got[i], want[i], err[i], worst))
    return worst


# ------------------------------------------------- references, once per case ----
@cached
def u_ref(case):
    from . import interp_ref as ref
    h, w, n, power = case
    x, y, v = points(h, w, n)
    return ref.unstructured_idw(x, y, v, (h, w), power)


@functools.lru_cache(maxsize=None)
def c_ref(case, dt):
    from . import interp_ref as ref
    g, w, k, power, fr, fphi, where, kind = case
    cx, cy = c_centre(g, where)
    return ref.circular_idw(grid((g, w)).astype(dt), c_mask(g, w, kind), k, power, fr, fphi, cx, cy)


@functools.lru_cache(maxsize=None)
def x_ref(case, dt):
    from . import interp_ref as ref
    h, w, k, power, kind = case
    return ref.cross_avg(grid((h, w)).astype(dt), x_mask(h, w, kind), k, power)


@functools.lru_cache(maxsize=None)
def p_ref(case, dt):
    from . import interp_ref as ref
    h, w, k, power, it, kind = case
    return ref.point_spread(grid((h, w)).astype(dt), p_mask(h, w, kind), k, power, it)


@functools.lru_cache(maxsize=None)
def s_ref(case, dt):
    from . import interp_ref as ref
    h, w, k, every = case
    return ref.fast_stat(s_image(h, w, dt), k, every)


@cached
def r_ref(case, dt):
    from . import interp_ref as ref
    kind, ss, ds = case
    return ref.resize(r_image(ss, dt), ds, kind)


# bounds of the existing tests for runs that feed their results back (no closed bound follows)
P_END_TOL = {F32: 3e-6, F64: 1e-10}


def p_bound(case, dt, nmax, depth):
    from . import interp_ref as ref
    if case[4] != 1:
        return P_END_TOL[dt]
    b = ref.bound_rel(nmax, ref.c_ops('point_spread', case[3]), dt) - ref.u_of(dt)
    return np.maximum(depth, 1) * b + ref.u_of(dt)
