"""The dark-current family of ``ops`` (csrc/dark.hip), re-exported there as ``ops.pair_min``,
``ops.nlf_threshold``, ``ops.stack_linregress``, ``ops.dark_current_eval`` and ``ops.cast_trunc``.
Like every family it goes through ``_stage_in`` / ``_stage_out``: host arrays in give host arrays
out, DeviceArrays stay on the device.
"""
import numpy as np

from . import _lib as L
from .device import DeviceArray, dtype_id
from ._staging import (PIXEL_DTYPES, _dev_out, _dptr, _f64_frame, _f64_host, _frame_pair, _px_host, _stage_in,
                       _stage_out, frame_stack)

MAX_FRAMES = 64   # kDarkMaxT of csrc/dark.hip


def pair_min(img, img2, ctx=None):
    """np.min((img, img2), axis=0) as float64, NaN winning: the image the reference hands to
    oneImageNLF (features/SingleTimeEffectDetection.py:39-42; ipa_pair_min_dev).  uint8 / uint16 /
    float32 / float64 frames of one type (two host frames of different types both go to
    float64)."""
    dev, ctx, d, d2, h, w = _frame_pair('pair_min', img, img2, ctx)
    d_out = DeviceArray(ctx, (h, w), np.float64)
    ctx._check(ctx._lib.ipa_pair_min_dev(ctx.handle, d.ptr, d2.ptr, dtype_id(d.dtype), h, w, w, w,
                                         d_out.ptr, w), 'pair_min')
    return _stage_out(dev, d_out)


def nlf_params(nlf):
    """(kind, parameters) of a noise level function the device can evaluate, or None: a
    (minY, ax, ay) triple or an object with ``.triple``, ``.poly`` = (p2, p1, p0, x0, x1) or
    ``.constant`` (what camera/NoiseLevelFunction.py returns)"""
    if callable(nlf):
        for attr, kind, n in (('triple', L.NLF_BOUNDED_SQRT, 3), ('poly', L.NLF_CLIPPED_POLY, 5)):
            p = getattr(nlf, attr, None)
            if p is not None:
                return kind, L.dbl(p, n)
        c = getattr(nlf, 'constant', None)
        return None if c is None else (L.NLF_CONSTANT, L.dbl([c], 1))
    return L.NLF_BOUNDED_SQRT, L.dbl(nlf, 3)


def nlf_threshold(x, nlf, nstd=1.0, out=None, ctx=None):
    """nlf(x) * nstd over a float64 frame (features/SingleTimeEffectDetection.py:44;
    ipa_nlf_threshold_dev).  nlf: see nlf_params; any other callable raises TypeError - it is host
    code.  `out` (device input only) may be x itself."""
    kp = nlf_params(nlf)
    if kp is None:
        raise TypeError('nlf_threshold: the function carries no .triple, .poly or .constant')
    dev, ctx, d, h, w = _stage_in('nlf_threshold', x, ctx, (np.float64,), _f64_host, (out,))
    d_out = _dev_out(ctx, out, (h, w), np.float64) if dev else DeviceArray(ctx, (h, w), np.float64)
    ctx._check(ctx._lib.ipa_nlf_threshold_dev(ctx.handle, d.ptr, h, w, w, kp[0], kp[1], float(nstd),
                                              d_out.ptr, w), 'nlf_threshold')
    return _stage_out(dev, d_out)


def stack_linregress(times, imgs, mx_intensity=65535, min_ascent=0.001, ctx=None):
    """getLinearityFunction of camera/DarkCurrentMap.py:61-80 in one launch -> (offset, ascent,
    error), float64 (h, w): per pixel the line image(t) = offset + ascent * t through the frames
    that are not above mx_intensity, its rms residual, and the reference's min_ascent step
    (ipa_stack_linregress_dev, where the arithmetic is spelled out).  imgs: a (T, h, w) array or a
    list of T frames, uint8 / uint16 / float32 / float64, 2 <= T <= 64 (ValueError below,
    NotImplementedError above)."""
    frames = frame_stack('stack_linregress', imgs)
    t = np.ascontiguousarray(np.asarray(times, dtype=np.float64).ravel())
    n = frames.shape[0]
    if t.size != n:
        raise ValueError('stack_linregress: %d times for %d frames' % (t.size, n))
    if n < 2:
        raise ValueError('stack_linregress: a line needs at least 2 frames (got %d)' % n)
    if n > MAX_FRAMES:
        raise NotImplementedError('stack_linregress: at most %d frames (got %d)' % (MAX_FRAMES, n))
    dev, ctx, d, h, w = _stage_in('stack_linregress', frames, ctx, PIXEL_DTYPES, _px_host, ndims=(3,))
    outs = [DeviceArray(ctx, (h, w), np.float64) for _ in range(3)]
    ctx._check(ctx._lib.ipa_stack_linregress_dev(
        ctx.handle, d.ptr, dtype_id(d.dtype), n, h, w, w, h * w, _dptr(t), float(mx_intensity),
        float(min_ascent), outs[0].ptr, outs[1].ptr, outs[2].ptr, w), 'stack_linregress')
    return tuple(_stage_out(dev, o) for o in outs)


def dark_current_eval(offset, ascent, exposuretime, limit, dtype=np.float64, ctx=None):
    """the dark current at one exposure time, the model CameraCalibration.calcDarkCurrent holds
    (camera/CameraCalibration.py:509-519): offset + ascent * exposuretime, `limit` (2 ** depth - 1)
    where above it, NaN kept; float64 or float32 (ipa_dark_current_eval_dev)."""
    if np.dtype(dtype) not in (np.float32, np.float64):
        raise TypeError('dark_current_eval: the output is float32 / float64 (got %s)' % np.dtype(dtype))
    dev, ctx, d_off, h, w = _stage_in('dark_current_eval', offset, ctx, (np.float64,), _f64_host,
                                      (ascent,))
    d_asc = _f64_frame('dark_current_eval', 'ascent', ascent, (h, w), ctx)
    d_out = DeviceArray(ctx, (h, w), dtype)
    ctx._check(ctx._lib.ipa_dark_current_eval_dev(
        ctx.handle, d_off.ptr, d_asc.ptr, h, w, w, float(exposuretime), float(limit), d_out.ptr,
        dtype_id(dtype), w), 'dark_current_eval')
    return _stage_out(dev, d_out)


def cast_trunc(img, dtype, out=None, ctx=None):
    """a float64 frame into uint8 / uint16 / float32 / float64 as numpy's `out[:] = img` converts
    it: integers truncated toward zero (camera/DarkCurrentMap.py:108-114; ipa_cast_trunc_dev).
    Defined for finite values inside the target's range."""
    dtype_id(dtype)
    dev, ctx, d, h, w = _stage_in('cast_trunc', img, ctx, (np.float64,), _f64_host, (out,))
    d_out = _dev_out(ctx, out, (h, w), dtype) if dev else DeviceArray(ctx, (h, w), dtype)
    ctx._check(ctx._lib.ipa_cast_trunc_dev(ctx.handle, d.ptr, h, w, w, d_out.ptr, dtype_id(dtype), w),
               'cast_trunc')
    return _stage_out(dev, d_out)
