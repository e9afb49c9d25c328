"""ipa_conv2d / ipa_sepconv2d restated in numpy float64: the yardstick of
tests/test_gpu_conv_paths.py (validated without a GPU against scipy, the C oracle and the
reference's own fixtures in tests/test_cpu_conv_refs.py).

Written from the definitions (include/imgproc_hip.h), with no tile, wave or LDS logic: the frame
is padded one axis at a time with np.pad, then shifted slices are summed tap by tap.

  conv2d      out[y, x] = sum_{i, j} k[i, j] * P[y + i - kh // 2, x + j - kw // 2], P the frame
              extended by `mode_y` along the rows and `mode` along the columns; 0 where mask == 0
  sepconv2d   the same along axis 0 with ky, THE RESULT ROUNDED TO THE IMAGE DTYPE (scipy's
              per-axis intermediate array), then along axis 1 with kx; a constant border pads
              the intermediate with cval

The centre of a kernel is k // 2 (scipy's, even sizes included).  Weights and cval are rounded
to the image dtype first, as the kernels hold them; every product and sum is float64, so the
error of an implementation against these is its own.

ref_abs is the same sum over |img|, |k|, |cval|: the magnitude a rounding-error bound is
relative to (bound(), below).
"""
import numpy as np

# library border mode -> np.pad mode
PAD = {'reflect': 'symmetric', 'mirror': 'reflect', 'nearest': 'edge', 'wrap': 'wrap',
       'constant': 'constant'}

UNIT = {np.dtype(np.float32): 2.0 ** -24, np.dtype(np.float64): 2.0 ** -53}


def _rounded(v, dtype):
    """v as the kernel holds it: rounded to the image dtype, then exact in float64"""
    return np.asarray(v, dtype=np.float64).astype(dtype).astype(np.float64)


def _pad(a, axis, before, after, mode, cval):
    width = [(0, 0), (0, 0)]
    width[axis] = (before, after)
    if mode == 'constant':
        return np.pad(a, width, mode='constant', constant_values=cval)
    return np.pad(a, width, mode=PAD[mode])


def _correlate1d(a, k, axis, mode, cval):
    """float64 a along `axis` with the taps k, centre len(k) // 2"""
    n = len(k)
    p = _pad(a, axis, n // 2, n - 1 - n // 2, mode, cval)
    out = np.zeros(a.shape)
    size = a.shape[axis]
    with np.errstate(invalid='ignore', over='ignore'):
        for i in range(n):
            sl = [slice(None), slice(None)]
            sl[axis] = slice(i, i + size)
            out += k[i] * p[tuple(sl)]
    return out


def _conv2d(a, k, mode, cval, mode_y):
    kh, kw = k.shape
    H, W = a.shape
    p = _pad(a, 0, kh // 2, kh - 1 - kh // 2, mode_y if mode_y is not None else mode, cval)
    p = _pad(p, 1, kw // 2, kw - 1 - kw // 2, mode, cval)
    out = np.zeros((H, W))
    with np.errstate(invalid='ignore', over='ignore'):
        for i in range(kh):
            for j in range(kw):
                out += k[i, j] * p[i:i + H, j:j + W]
    return out


def ref_conv2d(img, k, mode='reflect', cval=0.0, mode_y=None, mask=None):
    """-> float64 (H, W); mode along the columns, mode_y (default: mode) along the rows"""
    img = np.asarray(img)
    k = _rounded(k, img.dtype)
    assert img.ndim == 2 and k.ndim == 2
    out = _conv2d(img.astype(np.float64), k, mode, float(_rounded(cval, img.dtype)), mode_y)
    if mask is not None:
        out[np.asarray(mask) == 0] = 0.0
    return out


def ref_sepconv2d(img, ky, kx, mode='reflect', cval=0.0, mode_y=None):
    """-> float64 (H, W); None (or no taps) skips an axis"""
    img = np.asarray(img)
    assert img.ndim == 2
    cv = float(_rounded(cval, img.dtype))
    a = img.astype(np.float64)
    if ky is not None and len(ky):
        a = _correlate1d(a, _rounded(ky, img.dtype), 0, mode_y if mode_y is not None else mode, cv)
        with np.errstate(over='ignore'):
            a = a.astype(img.dtype).astype(np.float64)   # the intermediate array of the image dtype
    if kx is not None and len(kx):
        a = _correlate1d(a, _rounded(kx, img.dtype), 1, mode, cv)
    return a


def ref_abs(img, k, mode='reflect', cval=0.0, mode_y=None, mask=None):
    """the sum of ref_conv2d (k a 2-D array) or of ref_sepconv2d (k a pair (ky, kx), through
    both passes) over |img|, |k|, |cval|"""
    img = np.asarray(img)
    a = np.abs(img.astype(np.float64))
    cv = abs(float(_rounded(cval, img.dtype)))
    if isinstance(k, tuple):
        for taps, axis, m in ((k[0], 0, mode_y if mode_y is not None else mode), (k[1], 1, mode)):
            if taps is not None and len(taps):
                a = _correlate1d(a, np.abs(_rounded(taps, img.dtype)), axis, m, cv)
        return a
    out = _conv2d(a, np.abs(_rounded(k, img.dtype)), mode, cv, mode_y)
    if mask is not None:
        out[np.asarray(mask) == 0] = 0.0
    return out


def n_terms(k):
    """the n of the bound: kh * kw for a dense kernel, nky + nkx + 2 for a pair of taps (the
    rounding of the intermediate counts once per pass)"""
    if isinstance(k, tuple):
        return sum(len(t) for t in k if t is not None) + 2
    return int(np.asarray(k).size)


def bound(img, k, mode='reflect', cval=0.0, mode_y=None, mask=None):
    """per-pixel |got - ref| allowed to ANY summation order in the image's precision u, fused
    or not: a sum of n products stays within gamma_n = n u / (1 - n u) of the exact value,
    relative to the sum of the absolute values; + 2 for rounding the weights to the image dtype
    and for the final store.  (n + 2) u ref_abs, no further margin."""
    img = np.asarray(img)
    return (n_terms(k) + 2) * UNIT[img.dtype] * ref_abs(img, k, mode, cval, mode_y, mask)
