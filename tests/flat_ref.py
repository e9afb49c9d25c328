"""numpy restatement of what csrc/flat.hip computes and of the three functions built on it
(camera/flatField/flatFieldFromCloseDistance.py, camera/flatField/sensitivity.py), for the shapes
tests/golden/flat.npz does not hold.  test_cpu_flat.py proves it equal to the fixture; the GPU tests
compare the kernels with it.

Every sum runs in an explicit loop in the stated order.  The two resizes are the suite's
restatement of cv2.resize (interp_ref.resize), the 3 x 3 median that of nlf_ref (NaN in a window: NaN), the
single-time-effect steps those of test_cpu_ste.SteNumpy, the noise level functions those of
dark_ref.nlf_threshold.
"""
import numpy as np

from . import dark_ref
from .interp_ref import resize
from . import nlf_ref
from .test_cpu_ste import SteNumpy

LUMA_WEIGHTS = (0.299, 0.587, 0.114)
GRID = 10


def median3(a):
    """scipy.ndimage.median_filter(a, 3) with the kernels' rule for what scipy leaves unspecified:
    a NaN in the window gives NaN"""
    a = np.asarray(a, dtype=np.float64)
    m = nlf_ref.median3(a)
    p = np.pad(np.isnan(a), 1, mode='edge')
    h, w = a.shape
    m[np.any([p[dy:dy + h, dx:dx + w] for dy in range(3) for dx in range(3)], axis=0)] = np.nan
    return m


def stack_mean(frames):
    """imgAverage: `out = float(f0); out += f; out /= n`"""
    out = np.array(frames[0], dtype=np.float64)
    with np.errstate(invalid='ignore', over='ignore'):
        for f in frames[1:]:
            out += f
        out /= len(frames)
    return out


def luma(img, weights=LUMA_WEIGHTS):
    """np.average(img, axis=-1, weights=weights), spelled out"""
    w = np.asarray(weights, dtype=np.float64)
    img = np.asarray(img, dtype=np.float64)
    with np.errstate(invalid='ignore', over='ignore'):
        return ((img[..., 0] * w[0] + img[..., 1] * w[1]) + img[..., 2] * w[2]) / w.sum()


def strided_median_max(a, step=GRID):
    """median_filter(a[::step, ::step], 3).max(); 'reflect' repeats the edge sample of the grid"""
    return float(median3(np.asarray(a, dtype=np.float64)[::step, ::step]).max())


def strided_min(a, sy, sx):
    """a[::sy, ::sx].min(), in the frame's type"""
    return np.asarray(a)[::sy, ::sx].min()


def sort_key(a):
    """the key of flatFieldFromCloseDistance2's sort: it wraps for unsigned frames"""
    s0, s1 = a.shape[:2]
    with np.errstate(over='ignore'):
        return np.negative(strided_min(a, s0 // GRID, s1 // GRID))


def flat_scale(img, bg=None, div=None):
    out = np.array(img, dtype=np.float64)
    with np.errstate(invalid='ignore', over='ignore', divide='ignore'):
        if bg is not None:
            out = out - bg
        if div is not None:
            out = out / div
    return out


def nlf_lower_mask(frame, avg, kind, params, nstd):
    """frame > avg - nlf(avg) * nstd, compared in float64"""
    avg = np.asarray(avg, dtype=np.float64)
    with np.errstate(invalid='ignore', over='ignore'):
        thr = avg - dark_ref.nlf_threshold(avg, kind, params, nstd)
        return np.asarray(frame).astype(np.float64) > thr


def small_shape(shape, f):
    return int(round(shape[0] / f)), int(round(shape[1] / f))


def sens_signal(frame, bg=None):
    """i = float(frame); i -= bg"""
    i = np.asarray(frame).astype(np.float64)
    return i if bg is None else i - bg


def sens_shrink(frame, bg=None, f=10):
    """the INTER_AREA half of fastMean(median_filter(i, 3), f)"""
    with np.errstate(invalid='ignore', over='ignore'):
        i = sens_signal(frame, bg)
        return resize(median3(i), small_shape(i.shape, f), 'area')


def sensitivity(frames, bg=None, f=10):
    out = None
    for frame in frames:
        with np.errstate(invalid='ignore', divide='ignore', over='ignore'):
            i = sens_signal(frame, bg)
            smooth = resize(sens_shrink(frame, bg, f), i.shape, 'linear')
            q = i / smooth
            out = q if out is None else out + q
    return out / len(frames)


def flat_field_1(imgs, bg):
    """flatFieldFromCloseDistance; bg: a number or the background frames"""
    img = stack_mean(imgs)
    img = img - (bg if np.ndim(bg) == 0 else stack_mean(bg))
    if img.ndim == 3:
        img = luma(img)
    return img / strided_median_max(img)


def nlf_fn(kind, params):
    """the host function of a (kind, params) pair"""
    return lambda x: dark_ref.nlf_threshold(x, kind, params, 1.0)


def flat_field_2(images, bg, kind, params, nstd=6, listen=None):
    """flatFieldFromCloseDistance2 with the noise level function given -> (flat field, sort order).
    listen(frame, avg, thr, lower): called per frame added with the state its decisions are made
    on - avg, the STE threshold and the lower threshold avg - nlf(avg) * nstd"""
    order = sorted(range(len(images)), key=lambda k: sort_key(images[k]))
    images = [images[k] for k in order]
    avg_bg = bg if np.ndim(bg) == 0 else stack_mean(bg)
    i0 = np.asarray(images[0]).astype(np.float64) - avg_bg
    i1 = np.asarray(images[1]).astype(np.float64) - avg_bg
    fn = nlf_fn(kind, params)
    thr = fn(np.min((i0, i1), axis=0)) * nstd
    det = SteNumpy([i0, i1], None, None, thr=thr)
    for i in images[1:]:
        lower = det.avg - fn(det.avg) * nstd
        if listen is not None:
            listen(i, det.avg.copy(), det.thr, lower)
        det.add(np.asarray(i).astype(np.float64), np.asarray(i) > lower)
    return det.avg / strided_median_max(det.avg), order
