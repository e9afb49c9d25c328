"""Noise level function (NLF) estimation: the reference's camera/NoiseLevelFunction.py.

The NLF is the noise's standard deviation over image intensity.  ``calcNLF`` measures it from
one frame (noise = frame - its 3x3 median) or from two equivalent exposures (noise = their
difference): the median, the frame moments that set the intensity range and the binned mean of
|noise| over the signal all run in HIP kernels (csrc/nlf.hip; ops.nlf_signal, ops.nlf_moments,
ops.nlf_bins).  The square-root fit over the 50-odd bins that remain is host work
(scipy.optimize.curve_fit, as in the reference).

Frames are (h, w) arrays, uint8 / uint16 / float32 / float64 (other host types go to float64,
np.asfarray), host arrays or DeviceArrays.  Two host frames of different types are both taken as
float64, as np.asfarray of each gives; two DeviceArrays must share their type.  ``x``, ``y`` and
``weights`` are always small host arrays; ``signal`` comes back where the frame lives.

Differences from the reference, all at its undefined corners:
  - ``x[n]`` and ``y[n]`` of a bin with fewer than ``min_len`` pixels are NaN (the reference
    leaves them uninitialised, np.empty); with ``mn_mx_nbins`` an empty bin's ``y`` is NaN, as
    the reference's mean of nothing is.
  - a NaN in ``signal`` raises ValueError when the range is estimated (the reference's
    min / max is ill-defined there); with ``mn_mx_nbins`` a NaN pixel counts in no bin.
  - the function ``oneImageNLF`` / ``_evaluate`` return is an object with a ``.triple =
    (minY, ax, ay)`` attribute - SingleTimeEffectDetection and SNR evaluate it on the device -
    unless the polynomial fallback was taken: then it is a ``ClippedPolyNLF`` with ``.poly =
    (p2, p1, p0, x0, x1)`` or a ``ConstantNLF`` with ``.constant``, which SingleTimeEffectDetection
    evaluates on the device too (the reference returns bare lambdas; the call results are the same
    bits).
  - ``estimateFromImages`` takes arrays, not file paths.
"""
import numpy as np

from .. import ops
from .._staging import _f64_frame, _frame_pair

# factor root-mean-square to average-absolute-deviation
F_RMS2AAD = (2 / np.pi) ** -0.5
# a frame minus its 3x3 median underestimates the noise by this factor
F_NOISE_WITH_MEDIAN = 1 + (1 / 3 ** 2)
N_BINS = 100


class BoundedNLF(object):
    """boundedFunction with its parameters bound: fn(x) on the host, fn.triple for the device"""

    def __init__(self, minY, ax, ay):
        self.triple = (float(minY), float(ax), float(ay))

    def __call__(self, x):
        return boundedFunction(x, *self.triple)


class ClippedPolyNLF(object):
    """smooth()'s second-order polynomial, held to the range it was fitted on: fn(x) on the host,
    fn.poly = (p2, p1, p0, x0, x1) for the device (ops.nlf_threshold).  No ``.triple``: it is no
    square root."""

    def __init__(self, p, x0, x1):
        self._p = np.array(p, dtype=np.float64)
        self.poly = tuple(float(v) for v in self._p) + (float(x0), float(x1))

    def __call__(self, xint):
        return np.poly1d(self._p)(np.clip(xint, self.poly[3], self.poly[4]))


class ConstantNLF(object):
    """smooth()'s last resort, one noise level for every intensity: fn(x) on the host,
    fn.constant for the device"""

    def __init__(self, my):
        self._my = my
        self.constant = float(my)

    def __call__(self, x):
        return self._my


def estimateFromImages(imgs1, imgs2=None, mn_mx=None, nbins=100):
    """the NLF from a set of frames or frame pairs: imgs1[i] and imgs2[i] show the identical
    setup, so their difference is noise.  Returns (x, fn, y_avg, y_vals, w_vals, fitParams, i)."""
    if imgs2 is None:
        imgs2 = [None] * len(imgs1)
    elif len(imgs1) != len(imgs2):
        raise ValueError('imgs1 and imgs2 differ in length')
    y_vals = np.empty((len(imgs1), nbins))
    w_vals = np.zeros((len(imgs1), nbins))
    if mn_mx is None:
        mn, mx = 1e6, -1e6
        for i1 in imgs1:
            mmn, mmx = _getMinMax(i1)
            mn, mx = min(mn, mmn), max(mx, mmx)
    else:
        mn, mx = mn_mx
    x = None
    for n, (i1, i2) in enumerate(zip(imgs1, imgs2)):
        x, y, weights, _ = calcNLF(i1, i2, mn_mx_nbins=(mn, mx, nbins), x=x)
        y_vals[n] = y
        w_vals[n] = weights
    x, y_avg, w_vals, y_vals = _combine(x, y_vals, w_vals)
    fitParams, fn, i = _evaluate(x, y_avg, w_vals)
    return x, fn, y_avg, y_vals, w_vals, fitParams, i


def _combine(x, y_vals, w_vals):
    """the images' bins as one: -> (x, weighted mean of y, normalised weights, y_vals) of the bins
    some image filled"""
    filled = np.sum(w_vals, axis=0) != 0
    w_vals = w_vals[:, filled]
    y_vals = y_vals[:, filled]
    x = x[filled]
    y_avg = np.average(np.nan_to_num(y_vals), weights=w_vals, axis=0)
    w_vals = np.sum(w_vals, axis=0)
    w_vals /= w_vals.sum()
    return x, y_avg, w_vals, y_vals


def _evaluate(x, y, weights):
    """the parameters of ``function`` by curve fitting -> (fitParams, fn, valid indices)"""
    i = _validI(x, y, weights)
    xx = x[i]
    y = y[i]
    try:
        fitParams = _fit(xx, y)
        # bound the function to the lowest y it was fitted on:
        minY = function(xx[0], *fitParams)
        fitParams = np.insert(fitParams, 0, minY)
        fn = BoundedNLF(*fitParams)
    except RuntimeError:
        # no square-root fit with these bins: a polynomial instead
        fitParams = None
        fn = smooth(xx, y, weights[i])
    return fitParams, fn, i


def boundedFunction(x, minY, ax, ay):
    """``function`` limited to a minimum y value"""
    y = function(x, ax, ay)
    return np.maximum(np.nan_to_num(y), minY)


def function(x, ax, ay):
    """general square root function"""
    with np.errstate(invalid='ignore'):
        return ay * (x - ax) ** 0.5


def _validI(x, y, weights):
    """bins with enough pixels and a finite y.  The reference goes on to an outlier test on the
    gradient whose assignment goes into a copy (``i[i][...] = False``) and changes nothing: the
    density filter is its whole result, and that result is kept."""
    return np.logical_and(np.isfinite(y), weights > np.median(weights))


def _fit(x, y):
    from scipy.optimize import curve_fit
    popt, _ = curve_fit(function, x, y, check_finite=False)
    return popt


def smooth(x, y, weights):
    """where a square root does not describe the NLF: a bounded second-order polynomial, and a
    constant where even that cannot be fitted"""
    p = np.polyfit(x, y, w=weights, deg=2)
    if np.any(np.isnan(p)):
        return ConstantNLF(np.average(y, weights=weights))
    return ClippedPolyNLF(p, x[0], x[-1])


def oneImageNLF(img, img2=None, signal=None):
    """the NLF from one frame or two of the same kind -> (fn, signal)"""
    x, y, weights, signal = calcNLF(img, img2, signal)
    _, fn, _ = _evaluate(x, y, weights)
    return fn, signal


def _getMinMax(img):
    """the intensity range most pixels are in: mean +- 3 std, inside [max(min, 0), max]"""
    mn, mx, av, std, n_nan = ops.nlf_moments(img)
    if n_nan:
        raise ValueError('%d NaN values in the signal: its intensity range is undefined' % n_nan)
    return max(mn, av - 3 * std, 0), min(mx, av + 3 * std)


def _edges(mn, step, nbins):
    """the bin edges as the reference's loop accumulates them: e[k + 1] = e[k] + step"""
    e = np.empty(nbins + 1, np.float64)
    m = mn
    for n in range(nbins + 1):
        e[n] = m
        m += step
    return e


def calcNLF(img, img2=None, signal=None, mn_mx_nbins=None, x=None, averageFn='AAD',
            signalFromMultipleImages=False):
    """The noise level function as f(intensity) from one or two frames
    -> (x, y, weights, signal): bin centres, noise level and pixel count per intensity bin.

    img2 - second frame taken under the same conditions: the noise is their difference
    signal - the noise-free frame where the caller has one (else the 3x3 median)
    mn_mx_nbins - (min, max, number of bins) instead of the range estimated from the signal
    x - bin centres of an earlier call with the same mn_mx_nbins, left as they are
    averageFn - 'AAD' (average absolute deviation scaled to RMS) or anything else for RMS
    signalFromMultipleImages - the signal is an average of several frames, not one median
    """
    return _calc(img, img2, signal, mn_mx_nbins, x, averageFn, signalFromMultipleImages, None)


def _calc(img, img2, signal, mn_mx_nbins, x, averageFn, signalFromMultipleImages, bg):
    """calcNLF on frames read as `frame - bg` (what SNR hands to oneImageNLF)"""
    dev, ctx, d_img, d_img2, _, _ = _frame_pair('calcNLF', img, img2, None, (signal, bg))
    if signal is None:
        d_sig = ops.nlf_signal(d_img, d_img2, bg=bg)
    else:
        d_sig = _f64_frame('calcNLF', 'signal', signal, d_img.shape, ctx)
    if img2 is None:
        factor = 1.0 if signalFromMultipleImages else F_NOISE_WITH_MEDIAN
    else:
        # the difference of two noisy frames has twice the variance of one
        factor = 2 ** 0.5
    mn, mx, nbins, min_len = _binning(mn_mx_nbins, d_sig, d_img.shape)
    out_sig = d_sig if dev else (signal if signal is not None else d_sig.get())
    set_x = x is None
    if nbins == 0:   # a range under one unit: nothing to bin
        return (np.empty(0) if set_x else x), np.empty(0), np.zeros(0), out_sig
    step = (mx - mn) / nbins
    edges = _edges(mn, step, nbins)
    rms = averageFn != 'AAD'
    counts, sums = ops.nlf_bins(d_img, d_sig, edges, step, img2=d_img2, bg=bg, factor=factor, rms=rms)
    x, y, weights = _levels(counts, sums, edges, step, min_len, rms, x)
    return x, y, weights, out_sig


def _binning(mn_mx_nbins, signal, shape, min_max=_getMinMax):
    """-> (mn, mx, nbins, min_len): the caller's range and bins, every bin kept; or the signal's
    own range, 100 bins (one per unit of a narrower range) and bins of under 0.1 % of the
    pixels dropped"""
    if mn_mx_nbins is not None:
        mn, mx, nbins = mn_mx_nbins
        return mn, mx, nbins, 0
    mn, mx = min_max(signal)
    min_len = int(shape[0] * shape[1] * 1e-3)
    if min_len < 1:
        min_len = 5
    nbins = N_BINS
    if mx - mn < nbins:
        nbins = int(mx - mn)
    return mn, mx, nbins, min_len


def _levels(counts, sums, edges, step, min_len, rms, x=None):
    """the bins' pixel counts and sums of |noise| (noise ** 2 with rms) -> (x, y, weights); an x
    passed in is left as it is"""
    keep = counts >= min_len
    with np.errstate(invalid='ignore', divide='ignore'):
        mean = sums / counts
        # AAD is scaled to RMS
        y = np.where(keep, mean ** 0.5 if rms else mean * F_RMS2AAD, np.nan)
    weights = np.where(keep, counts, 0).astype(np.float64)
    if x is None:
        x = np.where(keep, edges[1:] - 0.5 * step, np.nan)
    return x, y, weights
