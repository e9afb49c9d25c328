"""Plain references of the operations behind csrc/interp_more.hip and csrc/resize.hip, written
from the operations as the header comments of the two files and DESIGN.md state them - numpy and
Python loops, no device, no oracle:

  unstructured_idw     scattered points -> every pixel (x is the ROW coordinate)
  circular_idw         polar-distance fill of the g x g domain, g = shape[0]
  cross_avg            the cross average with its stale slot
  point_spread         border sweeps in raster order, grid AND mask in place
  fast_stat            strided window median / mean, NaN-aware
  resize               cv2.resize, the numpy restatement of tests/golden/gen_golden.py

Every sum of a weighted mean is formed with math.fsum: the reference's own error is the rounding
of the terms, whatever the window size.  What depends on a type stays in that type: the cross
average's `avg` array in the grid's dtype, its float32 weights and uint16 distances, the blend
in the grid's dtype.  The fills return float64 arrays (the value BEFORE the store into the
grid), so that the store's rounding is the u_T of the bound and nothing else.

Bound of a weighted mean sum(w v) / sum(w) over n positive terms (bound_rel):
  (2 (ceil(n / 64) + 6) + c) u64 + u_T
2 sums, each over the 64 lanes of a wave (ceil(n / 64) additions per lane, 6 for the butterfly),
c roundings in one term w v on both sides, u_T the store.  The counted c per operation is in
C_OPS below and in the docstring of tests/test_gpu_interp_paths.py.
"""
import importlib.util
import math
import os

import numpy as np

F32, F64 = np.float32, np.float64
U64 = 2.0 ** -53


def u_of(dt):
    return 2.0 ** -24 if np.dtype(dt) == np.dtype(F32) else U64


# roundings in the final operations of one weight, in units of u64: pow within 2 ulp = 4 u
W_OPS = {2: 1, 1: 2, 0: 5}      # 1 / d2 | sqrt, 1 / . | pow, 1 / .


def pick(power):
    return 2 if power == 2 else (1 if power == 1 else 0)


def c_ops(op, power):
    """roundings of one term w v that can differ between the device and this file, both sides"""
    wops = W_OPS[pick(power)]
    if op == 'unstructured':     # x - i, y - j, two squares, their sum; the weight; w v
        return 2 * (5 + wops + 1)
    if op == 'point_spread':     # the squared distance is an exact integer; the weight; w v
        return 2 * (wops + 1)
    if op == 'circular':
        # radius, dr, midR: the same correctly rounded operations on the same inputs - equal bits.
        # The angles differ (atan2: see circular_idw); from there d, 2 pi - d, (.) midR,
        # fphi (.) are 4 roundings that enter s = p^2 + q^2 doubled, q^2 and the sum 2 more, and
        # w = s^-power multiplies them by power; then the weight and w v
        return 2 * (int(math.ceil(power)) * 10 + wops + 1)
    if op == 'cross':            # sum of values / count; the blend: 3 products, 2 sums, 1 pow
        return 2 * (3 + 2) + 4 + 1
    if op == 'stat':             # sum / n
        return 1
    raise KeyError(op)


def bound_rel(n, c, dt):
    """relative bound of a weighted mean over n window positions (module docstring)"""
    n = np.asarray(n, dtype=F64)
    return (2.0 * (np.ceil(n / 64.0) + 6.0) + c) * U64 + u_of(dt)


def inv_dist_pow(d2, power):
    """1 / d2^(power / 2) as the kernels form it"""
    d2 = np.asarray(d2, dtype=F64)
    with np.errstate(divide='ignore'):
        if power == 2:
            return 1.0 / d2
        if power == 1:
            return 1.0 / np.sqrt(d2)
        return 1.0 / np.power(d2, 0.5 * power)


def _fsum(a):
    return math.fsum(np.asarray(a, dtype=F64).ravel().tolist())


# ------------------------------------------------------------ scattered points ----
def unstructured_idw(x, y, v, shape, power=2):
    """-> float64 (h, w): at a pixel ON a point the first such point's value, else
    sum(w v) / sum(w) over all points, w = 1 / distance^power"""
    x, y, v = (np.asarray(a, dtype=F64) for a in (x, y, v))
    h, w = shape
    ii, jj = np.mgrid[0:h, 0:w].astype(F64)
    dx = x[:, None, None] - ii[None]
    dy = y[:, None, None] - jj[None]
    d2 = dx * dx + dy * dy
    wi = inv_dist_pow(d2, power)
    wv = wi * v[:, None, None]
    out = np.empty(shape, F64)
    for i in range(h):
        for j in range(w):
            hit = np.flatnonzero(d2[:, i, j] == 0.0)
            out[i, j] = v[hit[0]] if hit.size else _fsum(wv[:, i, j]) / _fsum(wi[:, i, j])
    return out


def unstructured_idw_seq(x, y, v, shape, power=2):
    """the same in the reference's order: float64 sums in point order, one point after the other
    for all pixels at once, stopped per pixel at its first hit - what the kernel computes bit for
    bit at power 2 (no pow, no fused multiply-add)"""
    x, y, v = (np.asarray(a, dtype=F64) for a in (x, y, v))
    h, w = shape
    ii, jj = np.mgrid[0:h, 0:w].astype(F64)
    sw, sv = np.zeros(shape), np.zeros(shape)
    hit, over = np.zeros(shape), np.zeros(shape, bool)
    for k in range(x.size):
        on = (x[k] == ii) & (y[k] == jj) & ~over
        hit[on] = v[k]
        over |= on
        dx, dy = x[k] - ii, y[k] - jj
        wi = inv_dist_pow(dx * dx + dy * dy, power)
        sw = np.where(over, sw, sw + wi)
        sv = np.where(over, sv, sv + wi * v[k])
    with np.errstate(invalid='ignore', divide='ignore'):
        return np.where(over, hit, sv / sw)


# ------------------------------------------------------------ polar-distance IDW ----
# |device atan2 - libm atan2| in ulps of the angle.  An ASSUMPTION, not a count: 2 ulp is what
# the device math library documents for atan2 in double precision, 1 ulp glibc's; nobody has
# measured either here.  The observed err / bound of the circular fill (0.05 in float64) says the
# assumption is not tight
ATAN2_ULPS = 3.0


def circular_idw(grid, mask, ksize, power, fr, fphi, cx, cy, defect=None):
    """-> (out float64, written bool, n int, c_angle float64): rows AND columns run to
    g = shape[0]; the window is [i-k, min(i+k, g)) x [j-k, min(j+k, g)), upper end EXCLUSIVE;
    distance = ((fr dr)^2 + (fphi dphi)^2)^2 with dphi = min(2 pi - |dPHI|, |dPHI|) times the
    mean radius; a window without an unmasked pixel leaves its pixel alone.

    c_angle (units of u64, per pixel): what the two atan2 implementations add to c.  An angle is
    off by at most ATAN2_ULPS ulps of pi, |PHI - nphi| by twice that, q = fphi dphi by
    dq = fphi midR times that, s = p^2 + q^2 by 2 q dq and w = s^-power by rho = power 2 q dq / s
    relative; first order in the mean: sum(w v rho) / sum(w v) + sum(w rho) / sum(w)."""
    g = grid.shape[0]
    assert grid.shape[1] >= g
    out = np.asarray(grid, dtype=F64).copy()
    written = np.zeros(grid.shape, bool)
    nn = np.zeros(grid.shape, np.int64)
    cang = np.zeros(grid.shape)
    ii, jj = np.mgrid[0:g, 0:g].astype(F64)
    ni, nj = ii - cx, jj - cy
    RR = np.sqrt(ni * ni + nj * nj)
    PP = np.arctan2(nj, ni)
    two_pi = 6.283185307179586476925286766559
    dphi_abs = 2 * ATAN2_ULPS * 2.0 ** -52 * math.pi
    vals = np.asarray(grid, dtype=F64)
    end = 1 if defect == 'inclusive' else 0   # (DEFECTS, end of this file)
    for i, j in np.argwhere(np.asarray(mask)[:g, :g] != 0):
        xmn, xmx = max(i - ksize, 0), min(i + ksize + end, g)
        ymn, ymx = max(j - ksize, 0), min(j + ksize + end, g)
        if xmx <= xmn or ymx <= ymn:
            continue
        use = np.asarray(mask)[xmn:xmx, ymn:ymx] == 0
        if xmn <= i < xmx and ymn <= j < ymx:
            use[i - xmn, j - ymn] = False
        nn[i, j] = (xmx - xmn) * (ymx - ymn)
        if not use.any():
            continue
        R, PHI = RR[i, j], PP[i, j]
        nR, nphi = RR[xmn:xmx, ymn:ymx][use], PP[xmn:xmx, ymn:ymx][use]
        dr, midR = R - nR, 0.5 * (R + nR)
        d = np.abs(PHI - nphi)
        e = two_pi - d
        dphi = np.where(e < d, e, d) * midR
        p, q = fr * dr, fphi * dphi
        s = p * p + q * q
        wi = inv_dist_pow(s * s, power)
        gv = vals[xmn:xmx, ymn:ymx][use]
        wv = wi * gv
        sw, sv = _fsum(wi), _fsum(wv)
        if sw != 0.0:
            out[i, j] = sv / sw
            written[i, j] = True
            rho = power * 2.0 * np.abs(q) * (abs(fphi) * midR * dphi_abs) / s / U64
            cang[i, j] = _fsum(wv * rho) / sv + _fsum(wi * rho) / sw
    return out, written, nn, cang


# ------------------------------------------------------------ cross average ----
def cross_avg(grid, mask, ksize, power, defect=None):
    """-> (out in the grid's dtype, n: the largest window of an average).  Raster order over the
    masked pixels.  Four searches along the pixel's column and row for the nearest unmasked pixel;
    the value of a found pixel is the mean of the unmasked pixels within +-k of it (window clamped
    to the array), kept in the grid's dtype.  Slots: 0 towards row 0; 2 towards column 0 - VALID
    when that search or the one towards the last row succeeded (the latter's own value is never
    used: with only it successful slot 2 holds what the last earlier pixel left there, and is left
    out when no pixel has); 3 towards the last column, searched only when i < shape[1] - 1.
    Distances are uint16, weights float32, normalised in float32; the blend runs in the grid's
    dtype.  (defect: DEFECTS, end of this file.)"""
    grid = np.asarray(grid)
    dt = grid.dtype.type
    m = np.asarray(mask) != 0
    h, w = grid.shape
    vals = grid.astype(F64)
    if defect == 'pitch':      # the grid inside a buffer of pitch w + 3, read with row stride w
        big = np.full((h + 1, w + 3), -77.0)
        big[:h, :w] = vals
        vals = big.ravel()[:h * w].reshape(h, w)
    out = grid.copy()
    memo = {}
    nmax = [0]

    def avg(i, j):
        if (i, j) not in memo:
            x0, x1 = max(i - ksize, 0), min(i + ksize, h - 1)
            y0, y1 = max(j - ksize, 0), min(j + ksize, w - 1)
            use = ~m[x0:x1 + 1, y0:y1 + 1]
            nmax[0] = max(nmax[0], use.size)
            win = vals[x0:x1 + 1, y0:y1 + 1].copy()
            ny = y1 - y0 + 1
            if defect == 'quotient' and (use.size - 1) * ny >= 1 << 20:
                # the first window position t with t ny >= 2^20 taken with the quotient t / ny + 1:
                # row + 1, column - ny - the element that address holds
                t = -(-(1 << 20) // ny)
                a = t // ny + 1
                flat = min((x0 + a) * w + y0 + t - a * ny, h * w - 1)
                use[t // ny, t % ny] = not m.ravel()[flat]
                win[t // ny, t % ny] = vals.ravel()[flat]
            memo[(i, j)] = dt(_fsum(win[use]) / float(use.sum()))
        return memo[(i, j)]

    def first(line):
        """1-based distance to the first unmasked entry of `line`, 0 when there is none"""
        z = np.flatnonzero(~line)
        d = int(z[0]) + 1 if z.size else 0
        if (defect == 'step9' and d >= 9) or (defect == 'step65' and d >= 65):
            d = min(d + 1, line.size)   # (still an address inside the array)
        return d
    hp = 0.5 * power
    slot2 = None
    for i, j in np.argwhere(m):
        d0 = first(m[:i, j][::-1])
        d1 = first(m[i + 1:, j])
        d2 = first(m[i, :j][::-1])
        d3 = first(m[i, j + 1:]) if i < w - 1 else 0
        if d2:
            slot2 = (avg(i, j - d2), np.uint16(d2))
        terms = []
        if d0:
            terms.append((avg(i - d0, j), np.uint16(d0)))
        if d2 or (d1 and defect != 'no_stale' and slot2 is not None):
            terms.append(slot2)
        if d3:
            terms.append((avg(i, j + d3), np.uint16(d3)))
        wt = [F32(1.0 / (float(d) if hp == 1.0 else float(np.power(F64(d), hp)))) for _, d in terms]
        tot = F32(0)
        for t in wt:
            tot = F32(tot + t)
        acc = dt(0)
        for (v, _), t in zip(terms, wt):
            q = F32(t / tot)
            acc = dt(acc + dt(dt(v) * dt(q)))
        out[i, j] = acc
    return out, nmax[0]


# ------------------------------------------------------------ point spread ----
def ps_border(mask, border):
    """two scans that compare every pixel with the one before it - in row-major order, then in
    column-major order, the predecessor carried across the ends of rows / columns - and SET
    border at the masked side of every change; where that side is the predecessor, its index is
    j - 1 (i - 1), which at j = 0 (i = 0) is -1: the LAST pixel of the row (column).
    -> whether any change was seen"""
    gx, gy = mask.shape
    f = mask.ravel()
    ch = np.flatnonzero(f[1:] != f[:-1]) + 1
    bf = border.reshape(-1)
    on = ch[f[ch]]
    bf[on] = True
    off = ch[~f[ch]]
    j = off % gy
    bf[np.where(j > 0, off - 1, off + gy - 1)] = True
    ft = np.ascontiguousarray(mask.T).ravel()
    ct = np.flatnonzero(ft[1:] != ft[:-1]) + 1
    jj, ii = ct // gx, ct % gx
    val = ft[ct]
    border[ii[val], jj[val]] = True
    border[np.where(ii[~val] > 0, ii[~val] - 1, gx - 1), jj[~val]] = True
    return bool(ch.size or ct.size)


def point_spread(grid, mask, ksize, power, max_iter, defect=None):
    """-> (grid float64, mask bool, n, sweeps, depth): grid and mask as the run leaves them; depth
    is, per filled pixel, the length of the longest chain of fills it rests on (1 = from original
    values only): a mean of positive values passes the relative error of its inputs on without
    enlarging it, so a pixel of depth L is within L times the bound of one mean.  A sweep takes the
    border pixels in raster order; each is filled from the unmasked pixels of
    [i-k, min(i+k, gx)) x [j-k, ymx) - the mask AS THE SWEEP HAS LEFT IT - with ymx = j + k, set
    to gy when it exceeds gx (the ROW count) or gy - and unmasked at once.  A window without an
    unmasked pixel leaves pixel, flag and mask alone.  Sweeps repeat while a border pass sees a
    change and fewer than max_iter have run.  Values are float64 here; the caller rounds into
    the grid's dtype after every sweep when it follows a float32 run sweep by sweep.
    (defect: DEFECTS, end of this file.)"""
    dt = np.asarray(grid).dtype
    g = np.asarray(grid, dtype=F64).copy()
    m = (np.asarray(mask) != 0).copy()
    gx, gy = g.shape
    border = np.zeros(g.shape, bool)
    depth = np.zeros(g.shape, np.int64)
    anyb = ps_border(m, border)
    n, nmax = 0, 0
    while n < max_iter and anyb:
        todo = np.argwhere(border)
        if defect == 'rows_swapped' and todo.size:
            a = int(todo[todo.shape[0] // 2, 0])   # a row with border pixels and the one below it
            b = a + 1
            key = np.where(todo[:, 0] == a, b, np.where(todo[:, 0] == b, a, todo[:, 0]))
            todo = todo[np.lexsort((todo[:, 1], key))]
        for i, j in todo:
            xmn, xmx = max(i - ksize, 0), min(i + ksize, gx)
            ymn, ymx = max(j - ksize, 0), j + ksize
            if ymx > gx or ymx > gy:
                ymx = gy
            if xmx <= xmn or ymx <= ymn:
                continue
            use = ~m[xmn:xmx, ymn:ymx]
            if xmn <= i < xmx and ymn <= j < ymx:
                use[i - xmn, j - ymn] = False
            if not use.any():
                continue
            nmax = max(nmax, use.size)
            xi, yi = np.nonzero(use)
            d2 = ((xi + xmn - i) ** 2 + (yi + ymn - j) ** 2).astype(F64)
            wi = inv_dist_pow(d2, power)
            sw, sv = _fsum(wi), _fsum(wi * g[xmn:xmx, ymn:ymx][use])
            if sw != 0.0:
                # stored in the grid's dtype: later windows of the run read the stored value
                g[i, j] = F64(np.asarray(sv / sw).astype(dt))
                depth[i, j] = 1 + int(depth[xmn:xmx, ymn:ymx][use].max())
                border[i, j] = False
                m[i, j] = False
        anyb = ps_border(m, border)
        n += 1
    return g, m, nmax, n, depth


# ------------------------------------------------------------ window statistics ----
FNS = ('median', 'nanmedian', 'mean', 'nanmean')   # the fn numbers of ipa_fast_filter_stat_dev


def fast_stat(arr, ksize, every, defect=None):
    """-> {fn: float64 (ceil(h / every), ceil(w / every))} for the four fn of FNS: the statistic of arr[max(i-k, 0):min(i+k, h):every, max(j-k, 0):min(j+k, w):every] at
    i = ii every, j = jj every.  The plain forms are NaN when the window holds one, the nan forms
    when it holds nothing else.  (defect: DEFECTS.)"""
    a = np.asarray(arr, dtype=F64)
    h, w = a.shape
    n0, n1 = -(-h // every), -(-w // every)
    out = {fn: np.empty((n0, n1)) for fn in FNS}
    for ii in range(n0):
        for jj in range(n1):
            i, j = ii * every, jj * every
            s = a[max(i - ksize, 0):min(i + ksize, h):every,
                  max(j - ksize, 0):min(j + ksize, w):every].ravel()
            if defect == 'drop_4096' and s.size >= 4096:
                s = s[:4095]
            nan = np.isnan(s)
            fin = np.sort(s[~nan])
            mean = _fsum(fin) / fin.size if fin.size else np.nan
            med = np.nan
            if fin.size:
                med = fin[(fin.size - 1) // 2] if fin.size & 1 else \
                    (fin[(fin.size - 1) // 2] + fin[fin.size // 2]) / 2.0
            out['nanmedian'][ii, jj], out['nanmean'][ii, jj] = med, mean
            out['median'][ii, jj] = np.nan if nan.any() else med
            out['mean'][ii, jj] = np.nan if nan.any() else mean
    return out


# ------------------------------------------------------------ resize ----
_GEN = None


def resize(img, dsize_hw, kind):
    """cv2.resize for 2-D float32 / float64 ('linear', 'cubic', 'lanczos4', 'area'): resize_np of
    tests/golden/gen_golden.py, the restatement the fixtures were generated with - float32
    coefficients, rows rounded to the image's type, no fused multiply-add; INTER_LINEAR at an
    exact 2 x 2 reduction is the area average (OpenCV's rule)"""
    global _GEN
    if _GEN is None:
        path = os.path.join(os.path.dirname(os.path.abspath(__file__)), 'golden', 'gen_golden.py')
        spec = importlib.util.spec_from_file_location('_ipa_gen_golden', path)
        _GEN = importlib.util.module_from_spec(spec)
        spec.loader.exec_module(_GEN)
    sh, sw = img.shape
    dh, dw = dsize_hw
    if kind == 'linear' and sw == 2 * dw and sh == 2 * dh:
        kind = 'area'
    return _GEN.resize_np(np.ascontiguousarray(img), (int(dh), int(dw)), kind)


# ------------------------------------------------------------ defects ----
# What a subtly wrong kernel would compute, as the argument `defect` of the functions above:
# tests/test_cpu_interp_refs.py::test_defects_are_seen runs each over the case list and asserts
# that the comparison with the oracle fails for at least one case - the cases can see the defect.
DEFECTS = {
    'inclusive': 'circular: the upper window end inclusive',
    'no_stale': 'cross average: the stale slot left out',
    'step9': 'cross average: search distance off by one from step 9 on',
    'step65': 'cross average: search distance off by one from step 65 on',
    'quotient': 'cross average: t / ny off by one at the first t beyond the multiply-shift limit',
    'pitch': 'cross average: the grid indexed by w instead of pitch',
    'rows_swapped': 'point spread: a row filled before the row above it',
    'drop_4096': 'statistics: sample 4096 dropped',
}
