"""Plain references of the two structured IDW fills behind csrc/idw.hip, in float64 with exact
sums (math.fsum), written from the reference loops:

  idw_fill       interpolate2dStructuredIDW._calc: every unmasked pixel of the (2 k + 1)^2 window
                 but the centre, the window clamped to the array
  fast_idw_fill  interpolate2dStructuredFastIDW._calc as the sequential walk it is: neighbours in
                 growing distance, stop WITH the (minnvals + 1)-th hit, or BEFORE a neighbour far
                 outside the image (beyond -1 / size + 1 in BOTH axes) once a hit exists

Both return the value BEFORE the store into the grid as float64, so the store's rounding is the
only float32 term of the bound, together with what the bound needs and, for the walk, where and
why it stopped.  `pitch`: the grid is a pitched buffer (h, pitch) of which w columns are the
image; the mask is always w wide.

Bound (bound_abs): the weights are positive, so a float64 sum of n terms in any order is within
(n - 1) u of its exact value relative to the sum of the magnitudes, u = 2^-53; the quotient of two
such sums is within (n + 2) u sum(w |g|) / sum(w) of the exact one (n - 1 for each sum to first
order, one for the division, the rest for the second order), plus half a unit in the last place
of the float32 result for float32 grids.  The terms w g are the same float64 products on both
sides.

`defect` names a wrong variant, for the sensitivity tests of test_cpu_idw_refs.py.
"""
import math

import numpy as np

U64 = 2.0 ** -53
HIT, FAR, END = 'hit', 'far', 'end'


def weights_of(k, power=2, fx=1, fy=1):
    from imgprocessor_amd.interpolate.interpolate2dStructuredIDW import idw_weights
    return idw_weights(k, power, fx, fy)


def neighbours_of(k, power=2):
    """-> (offsets (n, 2) int, weights (n,)) in the walk's order, n = (2 k + 1)^2 - 1"""
    from imgprocessor_amd.interpolate.interpolate2dStructuredFastIDW import growPositions
    idx, dist = growPositions(int(k))
    return np.asarray(idx, np.int64), 1 / dist ** (0.5 * power)


def _mean(ws, gs):
    """-> (value, scale = sum(w |g|) / sum(w)), exact sums of the float64 products"""
    sw = math.fsum(ws)
    if sw == 0.0:
        return None, 0.0
    tv = [w * g for w, g in zip(ws, gs)]
    with np.errstate(invalid='ignore'):
        return math.fsum(tv) / sw if all(t == t for t in tv) else float('nan'), \
            math.fsum(abs(t) for t in tv if t == t) / sw


def _mask_at(mask, yy, xx, defect, pitch):
    h, w = mask.shape
    if defect == 'mask_pitch':      # the mask indexed with the grid's pitch
        return bool(mask.ravel()[(yy * pitch + xx) % mask.size])
    return bool(mask[yy, xx])


def idw_fill(grid, mask, k, weights, defect=None, pitch=None):
    """-> dict(out, filled, scale, n): out float64 (h, w), the grid where nothing was filled"""
    g = np.asarray(grid)
    mask = np.asarray(mask, bool)
    h, w = mask.shape
    pitch = g.shape[1] if pitch is None else pitch
    g64 = g[:, :w].astype(np.float64)
    out = g64.copy()
    filled = np.zeros((h, w), bool)
    scale = np.zeros((h, w))
    nterm = np.zeros((h, w), np.int64)
    for i, j in zip(*np.nonzero(mask)):
        ws, gs = [], []
        for yy in range(max(i - k, 0), min(i + k, h - 1) + 1):
            for xx in range(max(j - k, 0), min(j + k, w - 1) + 1):
                centre = yy == i and xx == j
                if centre and defect != 'centre':
                    continue
                if not centre and _mask_at(mask, yy, xx, defect, pitch):
                    continue
                ws.append(float(weights[yy - i + k, xx - j + k]))
                gs.append(float(g64[yy, xx]))
        v, sc = _mean(ws, gs)
        if v is not None:
            out[i, j], filled[i, j], scale[i, j], nterm[i, j] = v, True, sc, len(ws)
    return dict(out=out, filled=filled, scale=scale, n=nterm)


def fast_idw_fill(grid, mask, offsets, weights, minnvals, defect=None, pitch=None):
    """minnvals as _calc gets it (the wrapper's minnvals - 1).  -> dict(out, filled, scale, n,
    stop, reason, hits, far_unlit, both): per masked pixel the neighbour index at which the walk
    stopped (len(offsets) at the end of the list), why, the hits counted (the stopping one
    included), whether a far-outside neighbour was met with no hit yet, and - where the 64
    neighbours around the stop hold a stop of the other kind as well - their order"""
    g = np.asarray(grid)
    mask = np.asarray(mask, bool)
    h, w = mask.shape
    pitch = g.shape[1] if pitch is None else pitch
    g64 = g[:, :w].astype(np.float64)
    out = g64.copy()
    N = len(offsets)
    shp = (h, w)
    res = dict(out=out, filled=np.zeros(shp, bool), scale=np.zeros(shp), n=np.zeros(shp, np.int64),
               stop=np.full(shp, -1), reason=np.full(shp, '', dtype=object), hits=np.zeros(shp, np.int64),
               far_unlit=np.zeros(shp, bool), both=np.full(shp, '', dtype=object))
    offs = [(int(a), int(b)) for a, b in offsets]
    for i, j in zip(*np.nonzero(mask)):
        ws, gs = [], []
        c, stop, reason = 0, N, END
        events = []   # (index, kind) of every position at which a walk that did not stop would
        cc = 0        # have met a stop condition, with the hits counted as if it never stopped
        for n, (di, dj) in enumerate(offs):
            if defect == 'reset64' and n % 64 == 0:
                c = 0
            iii, jjj = i + di, j + dj
            if 0 <= iii < h and 0 <= jjj < w:
                is_hit = not _mask_at(mask, iii, jjj, defect, pitch)
                if is_hit:
                    if cc == minnvals:
                        events.append((n, HIT))
                    cc += 1
                if stop == N and is_hit:
                    if defect == 'no_stop_hit' and c == minnvals:
                        stop, reason = n, HIT
                        continue
                    ws.append(float(weights[n]))
                    gs.append(float(g64[iii, jjj]))
                    if c == minnvals:
                        stop, reason, c = n, HIT, c + 1
                        continue
                    c += 1
            else:
                far_i, far_j = iii < -1 or iii > h + 1, jjj < -1 or jjj > w + 1
                far = (far_i or far_j) if defect == 'far_or' else (far_i and far_j)
                if far_i and far_j and cc > 0:
                    events.append((n, FAR))
                if stop == N and far:
                    if c > 0 or defect == 'far_no_c':
                        stop, reason = n, FAR
                    elif far_i and far_j:
                        res['far_unlit'][i, j] = True
        v, sc = _mean(ws, gs)
        if v is not None:
            res['out'][i, j], res['filled'][i, j], res['scale'][i, j] = v, True, sc
        res['n'][i, j], res['stop'][i, j], res['reason'][i, j], res['hits'][i, j] = len(ws), stop, reason, c
        if reason != END:
            other = [n for n, kind in events if kind != reason and n // 64 == stop // 64 and n > stop]
            if other:
                res['both'][i, j] = '%s<%s' % (reason, FAR if reason == HIT else HIT)
    return res


def bound_abs(res, dtype):
    """the bound of the module docstring per pixel, as an absolute error of the stored value"""
    b = (res['n'] + 2) * U64 * res['scale']
    if np.dtype(dtype) == np.dtype(np.float32):
        with np.errstate(invalid='ignore'):
            b = b + 0.5 * np.spacing(np.abs(np.nan_to_num(res['out'])).astype(np.float32)).astype(np.float64)
    return b


def worst(got, res, dtype):
    """-> worst err / bound over the filled pixels; the NaN pattern and every pixel that was not
    filled must match exactly (asserted)"""
    got = np.asarray(got)
    want = res['out']
    f = res['filled']
    assert np.array_equal(got[~f], want[~f].astype(got.dtype), equal_nan=True), 'an unfilled pixel changed'
    nan = np.isnan(want)
    assert np.array_equal(np.isnan(got), nan), 'NaN pattern differs'
    ok = f & ~nan
    if not ok.any():
        return 0.0
    err = np.abs(got.astype(np.float64) - want)[ok]
    b = bound_abs(res, dtype)[ok]
    return float(np.max(err / b))
