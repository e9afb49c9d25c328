"""numpy / scipy restatement of uncertainty/temporalSignalStability.py and of what csrc/tss.hip
computes, for the shapes tests/golden/tss.npz does not hold.  test_cpu_tss.py proves it equal to
the fixture; the GPU tests compare the kernels with it.

Two implementations of the event cube:

  events_median   the reference's way: scipy.ndimage.median_filter(diff, 5), |.| > 0.5 * error
  events_count    the kernel's way: per voxel the number of window samples above c and below -c
                  (c = 0.5 * error of the centre pixel), an event where either reaches 63 - with
                  the defects a kernel could have, for the sensitivity tests:
                    'thr62' 'thr64'   another majority
                    'ge'              >= where > belongs
                    'clamp_z' 'clamp_xy'  the edge repeated where scipy reflects
                    'reflect_once'    x and y reflected once where it takes more (an axis of one
                                      sample): the index is still beyond the row or the image,
                                      and the sample is whatever lies there in the stack
                    'halo_short'      samples two beyond the tile border taken one beyond it
                    'nb_threshold'    a sample compared with its own pixel's threshold
                    'centre_line'     samples beyond the tile border on the centre's line
                  and run_lengths(.., merge=True): runs one clean frame apart counted as one

Everything else is the reference's own sequence: the fit of dark_ref.stack_linregress (plain:
no intensity limit, no min_ascent), _calcAvgLen, stencil_ref.masked_mean over [i - 3, i + 3),
scipy's maximum_filter and median_filter.
"""
import numpy as np
from scipy.ndimage import maximum_filter, median_filter

from . import dark_ref, stencil_ref
from .tss_cases import TILE_H, TILE_W

MAJORITY = 63
DEFECTS = ('thr62', 'thr64', 'ge', 'clamp_z', 'clamp_xy', 'reflect_once', 'halo_short', 'nb_threshold',
           'centre_line', 'merge_runs')


def fit(times, stack):
    """-> (offset, ascent, error) of the plain per-pixel line"""
    return dark_ref.stack_linregress(times, stack, np.inf, 0)


def residuals(stack, times, offset, ascent):
    return np.stack([np.asarray(f).astype(np.float64) - (offset + float(t) * ascent)
                     for f, t in zip(stack, times)])


def events_median(stack, times, offset, ascent, error):
    diff = median_filter(residuals(stack, times, offset, ascent), 5)
    with np.errstate(invalid='ignore'):
        return np.abs(diff) > 0.5 * error[None]


# ------------------------------------------------------------------ the count form ----
def _reflect(i, n):
    m = np.mod(i, 2 * n)
    return np.where(m < n, m, 2 * n - 1 - m)


def _clamp(i, n):
    return np.clip(i, 0, n - 1)


def _reflect_once(i, n):
    return np.where(i < 0, -i - 1, np.where(i >= n, 2 * n - 1 - i, i))


def plane_counts(stack, times, offset, ascent, error, defect=None):
    """-> (plus, minus), int (T, h, w): samples of the 5 x 5 window of each frame above c / below
    -c, c the centre pixel's 0.5 * error"""
    st = np.stack([np.asarray(f).astype(np.float64) for f in stack])
    T, h, w = st.shape
    t = np.asarray(times, dtype=np.float64)[:, None, None]
    fold = _clamp if defect == 'clamp_xy' else _reflect
    if defect == 'reflect_once':
        return _plane_counts_flat(st, t, offset, ascent, error)
    c = 0.5 * error
    Y, X = np.mgrid[0:h, 0:w]
    ty0, tx0 = Y // TILE_H * TILE_H, X // TILE_W * TILE_W
    plus, minus = np.zeros((T, h, w), int), np.zeros((T, h, w), int)
    above = (lambda v, lim: v >= lim) if defect == 'ge' else (lambda v, lim: v > lim)
    below = (lambda v, lim: v <= lim) if defect == 'ge' else (lambda v, lim: v < lim)
    with np.errstate(invalid='ignore'):
        for dy in range(-2, 3):
            for dx in range(-2, 3):
                qy, qx = Y + dy, X + dx
                if defect == 'halo_short':
                    qy = np.clip(qy, ty0 - 1, ty0 + TILE_H)
                    qx = np.clip(qx, tx0 - 1, tx0 + TILE_W)
                outside = (qy < ty0) | (qy >= ty0 + TILE_H) | (qx < tx0) | (qx >= tx0 + TILE_W)
                sy, sx = fold(qy, h), fold(qx, w)
                r = st[:, sy, sx] - (offset[sy, sx] + t * ascent[sy, sx])
                if defect == 'centre_line':
                    r = np.where(outside, st[:, sy, sx] - (offset + t * ascent), r)
                lim = c[sy, sx] if defect == 'nb_threshold' else c
                plus += above(r, lim)
                minus += below(r, -lim)
    return plus, minus


def _plane_counts_flat(st, t, offset, ascent, error):
    """plane_counts with one reflection: an index it leaves outside its axis addresses the stack
    (and the planes) as flat memory, held inside the buffer"""
    T, h, w = st.shape
    c = 0.5 * error
    Y, X = np.mgrid[0:h, 0:w]
    off, asc = offset.ravel(), ascent.ravel()
    plus, minus = np.zeros((T, h, w), int), np.zeros((T, h, w), int)
    frame = np.arange(T)[:, None, None] * (h * w)
    for dy in range(-2, 3):
        for dx in range(-2, 3):
            i = _reflect_once(Y + dy, h) * w + _reflect_once(X + dx, w)
            v = st.ravel()[np.clip(frame + i[None], 0, T * h * w - 1)]
            ip = np.clip(i, 0, h * w - 1)
            r = v - (off[ip] + t * asc[ip])
            plus += r > c
            minus += r < -c
    return plus, minus


def window_counts(plus, minus, defect=None):
    """the plane counts summed over the five planes scipy's reflect gives for k - 2 .. k + 2"""
    T = plus.shape[0]
    k = np.arange(T)
    fold = _clamp if defect == 'clamp_z' else _reflect   # along the frames one reflection always does
    cp, cm = np.zeros_like(plus), np.zeros_like(minus)
    for dz in range(-2, 3):
        z = fold(k + dz, T)
        cp += plus[z]
        cm += minus[z]
    return cp, cm


def events_count(stack, times, offset, ascent, error, defect=None):
    cp, cm = window_counts(*plane_counts(stack, times, offset, ascent, error, defect), defect=defect)
    need = {'thr62': 62, 'thr64': 64}.get(defect, MAJORITY)
    return (cp >= need) | (cm >= need)


def run_lengths(evt, merge=False):
    """_calcAvgLen -> float64 (h, w).  merge: the defect of a counter that looks two frames back"""
    evt = np.asarray(evt, dtype=bool)
    nvals = np.zeros(evt.shape[1:])
    nclusters = np.zeros(evt.shape[1:])
    last = np.zeros(evt.shape[1:], bool)
    before = np.zeros(evt.shape[1:], bool)
    for e in evt:
        start = e & ~last & ~(before if merge else False)
        nclusters += start
        nvals += e
        before, last = last, e
    out = np.zeros(evt.shape[1:])
    np.divide(nvals, nclusters, out=out, where=nclusters != 0)
    return out


def run_lengths_grouped(evt):
    """the average run length a second way: per pixel the frames grouped into runs"""
    from itertools import groupby
    evt = np.asarray(evt, dtype=bool)
    out = np.zeros(evt.shape[1:])
    for idx in np.ndindex(*evt.shape[1:]):
        runs = [sum(1 for _ in grp) for on, grp in groupby(evt[(slice(None),) + idx]) if on]
        if runs:
            out[idx] = np.float64(sum(runs)) / np.float64(len(runs))
    return out


# ------------------------------------------------------------------ the 2-D tail ----
def masked_mean7(raw):
    """maskedFilter(avlen, mask=avlen == 0, fn='mean', ksize=7, fill_mask=False) -> (mean, mask)"""
    m0 = raw == 0
    return stencil_ref.masked_mean(raw, m0, 7, fill_mask=False), m0


def finish(mean, m0):
    """uncertainty/temporalSignalStability.py:72-78 with scipy's filters"""
    a = np.array(mean, dtype=np.float64)
    i = maximum_filter(np.asarray(m0) != 0, 3)
    a[i] = 0
    a = maximum_filter(a, 3)
    i = a == 0
    a = median_filter(a, 3)
    a[i] = 0
    return a


def temporal_signal_stability(stack, times, events=events_median):
    """-> dict: error, avlen, ascent, offset (what the reference returns) and events, raw, mean"""
    offset, ascent, error = fit(times, stack)
    evt = events(stack, times, offset, ascent, error)
    raw = run_lengths(evt)
    mean, m0 = masked_mean7(raw)
    return dict(error=error, avlen=finish(mean, m0), ascent=ascent, offset=offset, events=evt, raw=raw,
                mean=mean)
