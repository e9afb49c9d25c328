"""The flat-field family of ``ops`` (csrc/flat.hip), re-exported there as ``ops.stack_mean``,
``ops.luma``, ``ops.strided_median_max``, ``ops.strided_min``, ``ops.flat_scale``,
``ops.nlf_lower_mask``, ``ops.sens_shrink`` and ``ops.sens_accumulate``.  Like every family it goes
through ``_stage_in`` / ``_stage_out``: host arrays in give host arrays out, DeviceArrays stay on the
device; the two extrema are host scalars.
"""
import ctypes as C

import numpy as np

from . import _lib as L
from .device import DeviceArray, dtype_id
from ._staging import (PIXEL_DTYPES, _bg, _dev_out, _f64_frame, _f64_host, _is_dev, _px_host, _stage_in,
                       _stage_out, frame_stack)
from .ops_dark import nlf_params

LUMA_WEIGHTS = (0.299, 0.587, 0.114)   # red, green, blue (transformations.py:132-134)


def stack_mean(imgs, ctx=None):
    """the float64 mean of a (n, h, w) stack or a list of n frames, summed in frame order and then
    divided by n: numpy's `out = float(f0); out += f; out /= n` bit for bit
    (transform/imgAverage.py:14-21; ipa_stack_mean_dev).  uint8 / uint16 / float32 / float64, any
    n >= 1.  Colour frames - a (n, h, w, 3) stack or a list of (h, w, 3) frames - give (h, w, 3)."""
    frames = frame_stack('stack_mean', imgs, ndims=(2, 3))
    if frames.shape[0] < 1:
        raise ValueError('stack_mean: no frames')
    if len(frames.shape) == 4:   # served as (n, h, w * c)
        n, h, w, c = frames.shape
        if _is_dev(frames):
            flat = DeviceArray._wrap(frames.ctx, frames.ptr, (n, h, w * c), frames.dtype, False, base=frames)
            out = stack_mean(flat, ctx)
            return DeviceArray._wrap(out.ctx, out.ptr, (h, w, c), out.dtype, False, base=out)
        return stack_mean(_px_host(frames).reshape(n, h, w * c), ctx).reshape(h, w, c)
    n = frames.shape[0]
    dev, ctx, d, h, w = _stage_in('stack_mean', frames, ctx, PIXEL_DTYPES, _px_host, ndims=(3,))
    d_out = DeviceArray(ctx, (h, w), np.float64)
    ctx._check(ctx._lib.ipa_stack_mean_dev(ctx.handle, d.ptr, dtype_id(d.dtype), n, h, w, w, h * w,
                                           d_out.ptr, w), 'stack_mean')
    return _stage_out(dev, d_out)


def luma(img, weights=LUMA_WEIGHTS, ctx=None):
    """np.average(img, axis=-1, weights=weights) of an interleaved float64 (h, w, 3) frame
    (toGray, transformations.py:126-135; ipa_luma_dev): ((r * w0 + g * w1) + b * w2) / sum(w), the
    divisor computed here as numpy computes it."""
    wgt = np.asarray(weights, dtype=np.float64)
    if wgt.shape != (3,):
        raise ValueError('luma takes three weights')
    shape = tuple(img.shape) if _is_dev(img) else np.shape(img)
    if len(shape) != 3 or shape[2] != 3:
        raise ValueError('luma takes an (h, w, 3) frame (got shape %s)' % (shape,))
    dev, ctx, d, _, _ = _stage_in('luma', img, ctx, (np.float64,), _f64_host, ndims=(3,))
    h, w = d.shape[:2]
    d_out = DeviceArray(ctx, (h, w), np.float64)
    ctx._check(ctx._lib.ipa_luma_dev(ctx.handle, d.ptr, h, w, 3 * w, L.dbl(wgt, 3), float(wgt.sum()),
                                     d_out.ptr, w), 'luma')
    return _stage_out(dev, d_out)


def _extremum(name, img, sy, sx, mode, dtypes, host, ctx):
    if int(sy) < 1 or int(sx) < 1:
        raise ValueError('%s: slice step cannot be zero or negative (got %d, %d)' % (name, sy, sx))
    _, ctx, d, h, w = _stage_in(name, img, ctx, dtypes, host)
    r = C.c_double()
    ctx._check(ctx._lib.ipa_strided_extremum_dev(ctx.handle, d.ptr, dtype_id(d.dtype), h, w, w, int(sy),
                                                 int(sx), mode, C.byref(r)), name)
    return d.dtype, r.value


def strided_median_max(img, step=10, ctx=None):
    """median_filter(img[::step, ::step], 3).max() of a float64 frame as a Python float, scipy's
    'reflect' border on the strided grid (camera/flatField/flatFieldFromCloseDistance.py:36, :91;
    ipa_strided_extremum_dev).  A NaN in any window gives NaN."""
    return _extremum('strided_median_max', img, step, step, L.EXTREMUM_MEDIAN_MAX, (np.float64,),
                     _f64_host, ctx)[1]


def strided_min(img, step_y, step_x, ctx=None):
    """img[::step_y, ::step_x].min() in the frame's own type - a numpy scalar of uint8 / uint16 /
    float32 / float64 (camera/flatField/flatFieldFromCloseDistance.py:62; ipa_strided_extremum_dev)"""
    dt, v = _extremum('strided_min', img, step_y, step_x, L.EXTREMUM_MIN, PIXEL_DTYPES, _px_host, ctx)
    return dt.type(v)


def flat_scale(img, bg=None, div=None, out=None, ctx=None):
    """(img - bg) / div over a float64 frame, or one of the two steps where the other argument is
    None (camera/flatField/flatFieldFromCloseDistance.py:34-37, :96; ipa_flat_scale_dev).  bg: a
    scalar or a float64 (h, w) frame.  `out` (device input only) may be img itself."""
    dev, ctx, d, h, w = _stage_in('flat_scale', img, ctx, (np.float64,), _f64_host, (bg, out))
    d_bg, bgp, bg_pitch, bgv = _bg('flat_scale', bg, (h, w), ctx)
    d_out = _dev_out(ctx, out, (h, w), np.float64) if dev else DeviceArray(ctx, (h, w), np.float64)
    ctx._check(ctx._lib.ipa_flat_scale_dev(
        ctx.handle, d.ptr, h, w, w, bgp, bg_pitch, bgv, int(bg is not None),
        1.0 if div is None else float(div), int(div is not None), d_out.ptr, w), 'flat_scale')
    return _stage_out(dev, d_out)


def nlf_lower_mask(img, avg, nlf, nstd=6, out=None, ctx=None):
    """uint8 `img > avg - nlf(avg) * nstd`, compared in float64, NaN false: the pixels that are not
    erroneously dark (camera/flatField/flatFieldFromCloseDistance.py:80-81; ipa_nlf_lower_mask_dev).
    img: uint8 / uint16 / float32 / float64, avg: float64.  nlf: see nlf_params; any other callable
    raises TypeError - it is host code.  The result is what ste_update takes as `mask`; a host
    frame gives a bool array."""
    kp = nlf_params(nlf)
    if kp is None:
        raise TypeError('nlf_lower_mask: the function carries no .triple, .poly or .constant')
    dev, ctx, d, h, w = _stage_in('nlf_lower_mask', img, ctx, PIXEL_DTYPES, _px_host, (avg, out))
    d_avg = _f64_frame('nlf_lower_mask', 'avg', avg, (h, w), ctx)
    d_out = _dev_out(ctx, out, (h, w), np.uint8) if dev else DeviceArray(ctx, (h, w), np.uint8)
    ctx._check(ctx._lib.ipa_nlf_lower_mask_dev(ctx.handle, d.ptr, dtype_id(d.dtype), h, w, w, d_avg.ptr, w,
                                               kp[0], kp[1], float(nstd), d_out.ptr, w), 'nlf_lower_mask')
    return d_out if dev else d_out.get().astype(bool)


def small_shape(shape, f):
    """(round(h / f), round(w / f)): the small image of fastMean (filters/fastMean.py:10-12)"""
    dh, dw = int(round(shape[0] / f)), int(round(shape[1] / f))
    if dh < 1 or dw < 1:
        raise ValueError('a %d x %d frame shrunk by %s is empty' % (shape[0], shape[1], f))
    if dh > shape[0] or dw > shape[1]:
        raise NotImplementedError('f = %s enlarges the frame (INTER_AREA is built for downscaling)' % (f,))
    return dh, dw


def sens_shrink(img, bg=None, f=10, out=None, ctx=None):
    """cv2.resize(median_filter(img - bg, 3), round(shape / f), INTER_AREA) as float64: the small
    image inside fastMean (camera/flatField/sensitivity.py:21-23; ipa_sens_shrink_dev).  One kernel
    where the frame is a whole number of blocks in both directions."""
    shape = tuple(img.shape) if _is_dev(img) else np.shape(img)
    if len(shape) != 2:
        raise ValueError('sens_shrink works on 2-D arrays (got shape %s)' % (shape,))
    dh, dw = small_shape(shape, f)
    dev, ctx, d, h, w = _stage_in('sens_shrink', img, ctx, PIXEL_DTYPES, _px_host, (bg, out))
    d_bg, bgp, bg_pitch, bgv = _bg('sens_shrink', bg, (h, w), ctx)
    d_out = _dev_out(ctx, out, (dh, dw), np.float64) if dev else DeviceArray(ctx, (dh, dw), np.float64)
    ctx._check(ctx._lib.ipa_sens_shrink_dev(ctx.handle, d.ptr, dtype_id(d.dtype), h, w, w, bgp, bg_pitch,
                                            bgv, dh, dw, d_out.ptr, dw), 'sens_shrink')
    return _stage_out(dev, d_out)


def sens_accumulate(img, small, acc, bg=None, first=False, n_last=0, ctx=None):
    """acc = (img - bg) / up(small) where `first`, acc += that otherwise, then acc /= n_last where
    n_last > 0; up = cv2.resize(small, img.shape, INTER_LINEAR), evaluated per pixel
    (camera/flatField/sensitivity.py:23-29; ipa_sens_accumulate_dev).  acc is a float64 (h, w)
    DeviceArray, updated in place and returned."""
    dev, ctx, d, h, w = _stage_in('sens_accumulate', img, ctx, PIXEL_DTYPES, _px_host, (bg, small, acc))
    if not _is_dev(acc) or tuple(acc.shape) != (h, w) or acc.dtype != np.float64:
        raise ValueError('sens_accumulate: acc must be a float64 DeviceArray of shape %s' % ((h, w),))
    d_small = small if _is_dev(small) else ctx.to_device(_f64_host(small))
    if d_small.dtype != np.float64 or d_small.ndim != 2:
        raise ValueError('sens_accumulate: small must be a 2-D float64 array')
    dh, dw = d_small.shape
    d_bg, bgp, bg_pitch, bgv = _bg('sens_accumulate', bg, (h, w), ctx)
    ctx._check(ctx._lib.ipa_sens_accumulate_dev(
        ctx.handle, d.ptr, dtype_id(d.dtype), h, w, w, bgp, bg_pitch, bgv, d_small.ptr, dh, dw, dw,
        acc.ptr, w, int(bool(first)), int(n_last)), 'sens_accumulate')
    return acc
