"""The 2-D polynomial fit family of ``ops`` (csrc/poly.hip), re-exported there as
``ops.poly2d_moments``, ``ops.poly2d_solve``, ``ops.poly2d_eval``, ``ops.high_grad_mask`` and
``ops.clip01``.  Like every family it goes through ``_stage_in`` / ``_stage_out``: host arrays in
give host arrays out, DeviceArrays stay on the device.

The fit is a least-squares fit of sum c[j][i] T_j(v) T_i(u), Chebyshev polynomials of the pixel
position mapped to [-1, 1] (include/imgproc_hip.h).  The device sums the moments; the
(order+1)^2-square system is solved here, on the host, in float64.
"""
import ctypes as C

import numpy as np

from . import _lib as L
from .device import DeviceArray, dtype_id
from ._staging import _ctx_of, _dptr, _f64_frame, _is_dev, _stage_in, _stage_out, _u8_frame

MAX_ORDER = 5            # kPolyMaxOrder of csrc/poly.hip
MAX_WINDOW = 31          # kHighGradMaxSize
FLOAT_DTYPES = (np.float32, np.float64)
# a Gram matrix whose smallest eigenvalue is below this fraction of its largest is singular
SINGULAR_RCOND = 1e-13


def _order(name, order):
    o = int(order)
    if o != order or o < 0:
        raise ValueError('%s: the order must be an integer >= 0 (got %r)' % (name, order))
    if o > MAX_ORDER:
        raise NotImplementedError('%s: orders 0 .. %d (got %d)' % (name, MAX_ORDER, o))
    return o


def _float_host(a):
    """host frames: float32 / float64 as they are; nothing else is a fitted field"""
    a = np.asarray(a)
    if a.dtype not in FLOAT_DTYPES:
        raise TypeError('needs float32 / float64 arrays (got %s)' % a.dtype)
    return np.ascontiguousarray(a)


def poly2d_moments(img, mask=None, order=2, ctx=None):
    """interpolate/polyfit2d.py:13-18, 46-49 -> (M, R, count): over the pixels of `img` (float32 /
    float64) where `mask` (uint8 / bool, None: nowhere) is NOT set, M[b, a] = sum T_b(v) T_a(u) for
    a, b <= 2 order, R[j, i] = sum img T_j(v) T_i(u) for i, j <= order, and the number of those
    pixels (ipa_poly2d_moments_dev).  Host float64 arrays and an int, whatever `img` is.  Orders
    above 5 are a NotImplementedError."""
    o = _order('poly2d_moments', order)
    dev, ctx, d, h, w = _stage_in('poly2d_moments', img, ctx, FLOAT_DTYPES, _float_host, (mask,))
    d_mask = None if mask is None else _u8_frame('poly2d_moments', 'the mask', mask, (h, w), ctx)
    n, k = 2 * o + 1, o + 1
    out = np.empty(n * n + k * k + 1)
    ctx._check(ctx._lib.ipa_poly2d_moments_dev(
        ctx.handle, d.ptr, dtype_id(d.dtype), h, w, w, d_mask.ptr if d_mask is not None else None, w, o,
        _dptr(out)), 'poly2d_moments')
    return out[:n * n].reshape(n, n), out[n * n:n * n + k * k].reshape(k, k), int(out[-1])


def poly2d_gram(M, order):
    """the Gram matrix of the basis T_j(v) T_i(u), row / column index j (order + 1) + i, from the
    moments: T_i T_k = (T_{i+k} + T_{|i-k|}) / 2 along each axis"""
    k = int(order) + 1
    i = np.arange(k)
    s, d = i[:, None] + i[None, :], np.abs(i[:, None] - i[None, :])   # [i, k]
    M = np.asarray(M, dtype=np.float64)
    G = np.zeros((k, k, k, k))                                       # [j, i, l, k]
    for bv in (s, d):
        for bu in (s, d):
            G += M[bv[:, None, :, None], bu[None, :, None, :]]
    return (0.25 * G).reshape(k * k, k * k)


def poly2d_solve(M, R, count, order):
    """the (order + 1, order + 1) coefficients c[j, i] of T_j(v) T_i(u) from the moments, in float64 on
    the host.  ValueError where the reference's lstsq would return a minimum-norm answer: fewer valid
    pixels than coefficients, or a singular Gram matrix (smallest eigenvalue below 1e-13 of the
    largest - a single row or column at order >= 1, valid pixels on too few lines)."""
    k = int(order) + 1
    if count < k * k:
        raise ValueError('polynomial fit of order %d: %d valid pixels for %d coefficients' % (order, count, k * k))
    G = poly2d_gram(M, order)
    if not np.isfinite(G).all():
        raise ValueError('polynomial fit of order %d: the moments are not finite' % order)
    ev = np.linalg.eigvalsh(G)
    if not ev[0] > SINGULAR_RCOND * ev[-1]:
        raise ValueError('polynomial fit of order %d: the valid pixels do not determine it (Gram matrix '
                         'eigenvalues %.3g .. %.3g)' % (order, ev[0], ev[-1]))
    return np.linalg.solve(G, np.asarray(R, dtype=np.float64).reshape(-1)).reshape(k, k)


def _coef(name, coef):
    c = np.ascontiguousarray(coef, dtype=np.float64)
    if c.ndim != 2 or c.shape[0] != c.shape[1] or c.shape[0] < 1:
        raise ValueError('%s: the coefficients must be (order + 1, order + 1) (got shape %s)' % (name, c.shape))
    return c, _order(name, c.shape[0] - 1)


def poly2d_eval(coef, arr, mask=None, outgrid=None, inplace=False, residuum=False, ctx=None):
    """interpolate/polyfit2d.py:22-28, 50-64: the polynomial with coefficients coef[j, i] of
    T_j(v) T_i(u) on the frame of `arr` (float32 / float64; its shape is the coordinate map, its
    dtype the result's), computed in double and rounded once (ipa_poly2d_eval_dev).
      outgrid=(yy, xx)  float64 pixel positions, any 2-D shape -> the values there (positions outside
                        the frame extrapolate); arr's values are not read
      mask=None         every pixel rewritten -> a new array
      mask              the pixels where it is set replaced -> a copy, or `arr` itself with
                        inplace=True (a host array is written too)
    residuum=True (not with an outgrid) returns (result, sum |new - old| over the replaced pixels):
    camera/flatField/postprocessing/polynomial.py:37 times the frame's size."""
    c, o = _coef('poly2d_eval', coef)
    if outgrid is not None or mask is None:
        others = tuple(outgrid) if outgrid is not None else ()
        if outgrid is not None and (residuum or inplace):
            raise ValueError('poly2d_eval: an outgrid has neither a residuum nor an in-place result')
        dev = _is_dev(arr)
        need_in = outgrid is None and (residuum or inplace)
        if need_in or dev:
            dev, ctx, d, h, w = _stage_in('poly2d_eval', arr, ctx, FLOAT_DTYPES, _float_host, others)
            dt = d.dtype
        else:   # a host frame gives its shape and type only: nothing goes up
            a = np.asarray(arr)
            if a.dtype not in FLOAT_DTYPES:
                raise TypeError('poly2d_eval needs float32 / float64 arrays (got %s)' % a.dtype)
            if a.ndim != 2:
                raise ValueError('poly2d_eval works on 2-D arrays (got shape %s)' % (a.shape,))
            ctx, d, (h, w), dt = _ctx_of(*others, ctx=ctx), None, a.shape, a.dtype
        if h < 1 or w < 1:
            raise ValueError('poly2d_eval: empty frame')
        if outgrid is not None:
            yy, xx = outgrid
            shape = tuple(yy.shape)
            if len(shape) != 2 or shape[0] < 1 or shape[1] < 1:
                raise ValueError('poly2d_eval: the outgrid must be two 2-D arrays (got shape %s)' % (shape,))
            d_gy = _f64_frame('poly2d_eval', 'outgrid[0]', yy, shape, ctx)
            d_gx = _f64_frame('poly2d_eval', 'outgrid[1]', xx, shape, ctx)
            d_out = DeviceArray(ctx, shape, dt)
            ctx._check(ctx._lib.ipa_poly2d_eval_dev(
                ctx.handle, _dptr(c), o, L.POLY_GRID, None, dtype_id(dt), h, w, w, None, w, d_gy.ptr, d_gx.ptr,
                shape[0], shape[1], shape[1], d_out.ptr, shape[1], None), 'poly2d_eval')
            return _stage_out(dev, d_out)
        d_out = d if inplace else DeviceArray(ctx, (h, w), dt)
        res = C.c_double(0.0)
        ctx._check(ctx._lib.ipa_poly2d_eval_dev(
            ctx.handle, _dptr(c), o, L.POLY_ALL, d.ptr if need_in else None, dtype_id(dt), h, w, w, None, w,
            None, None, 0, 0, 0, d_out.ptr, w, C.byref(res) if residuum else None), 'poly2d_eval')
        out = _finish(dev, arr, d_out, inplace)
        return (out, res.value) if residuum else out
    dev, ctx, d, h, w = _stage_in('poly2d_eval', arr, ctx, FLOAT_DTYPES, _float_host, (mask,))
    d_mask = _u8_frame('poly2d_eval', 'the mask', mask, (h, w), ctx)
    d_out = d if inplace else DeviceArray(ctx, (h, w), d.dtype)
    res = C.c_double(0.0)
    ctx._check(ctx._lib.ipa_poly2d_eval_dev(
        ctx.handle, _dptr(c), o, L.POLY_FILL, d.ptr, dtype_id(d.dtype), h, w, w, d_mask.ptr, w, None, None, 0, 0, 0,
        d_out.ptr, w, C.byref(res) if residuum else None), 'poly2d_eval')
    out = _finish(dev, arr, d_out, inplace)
    return (out, res.value) if residuum else out


def _finish(dev, arr, d_out, inplace):
    """the result as the input came; in place on a host array writes that array"""
    if dev:
        return d_out
    if inplace:
        if not isinstance(arr, np.ndarray):
            raise TypeError('in place needs an ndarray or a DeviceArray')
        arr[...] = d_out.get()
        return arr
    return d_out.get()


def high_grad_window(shape):
    """camera/flatField/postprocessing/polynomial.py:12-14: the dilation window of a frame"""
    return min(max(min(shape) // 5, 3), 15)


def high_grad_mask(arr, threshold=0.01, size=None, ctx=None):
    """camera/flatField/postprocessing/polynomial.py:10-14 (_highGrad) -> (mask, count):
    maximum_filter(|scipy.ndimage.laplace(arr, mode='reflect')| > threshold, size) as uint8 0 / 1 and
    the number of set pixels (ipa_high_grad_dev).  arr: float32 / float64; size None: the
    reference's min(max(min(shape) // 5, 3), 15); windows above 31 are a NotImplementedError."""
    s = high_grad_window(arr.shape if _is_dev(arr) else np.shape(arr)) if size is None else int(size)
    if s < 1:
        raise ValueError('high_grad_mask: window %d' % s)
    if s > MAX_WINDOW:
        raise NotImplementedError('high_grad_mask: windows up to %d (got %d)' % (MAX_WINDOW, s))
    dev, ctx, d, h, w = _stage_in('high_grad_mask', arr, ctx, FLOAT_DTYPES, _float_host)
    d_mask = DeviceArray(ctx, (h, w), np.uint8)
    n = C.c_double(0.0)
    ctx._check(ctx._lib.ipa_high_grad_dev(ctx.handle, d.ptr, dtype_id(d.dtype), h, w, w, float(threshold), s,
                                          d_mask.ptr, w, C.byref(n)), 'high_grad_mask')
    return _stage_out(dev, d_mask), int(n.value)


def clip01(arr, ctx=None):
    """np.clip(arr, 0, 1, out=arr) (camera/flatField/postprocessing/polynomial.py:49): a DeviceArray
    in place, a host array as a new array; NaN stays (ipa_clip01_dev)"""
    dev, ctx, d, h, w = _stage_in('clip01', arr, ctx, FLOAT_DTYPES, _float_host)
    ctx._check(ctx._lib.ipa_clip01_dev(ctx.handle, d.ptr, dtype_id(d.dtype), h, w, w), 'clip01')
    return _stage_out(dev, d)
