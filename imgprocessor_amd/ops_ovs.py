"""The object / vignetting separation family of ``ops`` (csrc/ovs.hip), re-exported there as
``ops.ovs_object``, ``ops.ovs_flatfield`` and ``ops.masked_running_mean_update``.  Like every
family it goes through ``_stage_in`` / ``_stage_out``: host arrays in give host arrays out,
DeviceArrays stay on the device.
"""
import numpy as np

from .device import DeviceArray, dtype_id
from ._staging import (PIXEL_DTYPES, _dptr, _f64_frame, _f64_host, _is_dev, _px_host, _stage_in, _stage_out,
                       _u8_frame, frame_stack)

MAX_FRAMES = 64   # kOvsMaxN of csrc/ovs.hip


def _mats(name, M, n):
    """n destination -> source matrices as one C-contiguous float64 (n, 3, 3) array"""
    m = np.ascontiguousarray(np.asarray(M, dtype=np.float64))
    if m.shape == (3, 3):
        m = m[None]
    if m.ndim != 3 or m.shape[1:] != (3, 3):
        raise ValueError('%s: the matrices must be 3 x 3 (got shape %s)' % (name, m.shape))
    if m.shape[0] != n:
        raise ValueError('%s: %d matrices for %d fitted images' % (name, m.shape[0], n))
    return np.ascontiguousarray(m)


def _fits(name, fits, ctx):
    frames = frame_stack(name, fits)
    n = frames.shape[0]
    if n < 1:
        raise ValueError('%s: needs at least one fitted image' % name)
    if n > MAX_FRAMES:
        raise NotImplementedError('%s: at most %d fitted images (got %d)' % (name, MAX_FRAMES, n))
    return frames, n


def ovs_object(ff, fits, M, ctx=None):
    """camera/flatField/vignettingFromRandomSteps.py:241-249 in one launch -> (object, count),
    float64 and int32 (oh, ow): per pixel the running mean over the fitted images, in order, of
    fit_k / w_k where w_k != 0, w_k being the flat field `ff` (float64 (fh, fw)) sampled at
    M[k] * (x, y, 1) exactly as ``warp_perspective(ff, M[k], ., 'linear_cv_q5', 'constant', 0.0)``
    samples it (ipa_ovs_object_dev).  fits: a (N, oh, ow) array or a list of N frames, uint8 /
    uint16 / float32 / float64, 1 <= N <= 64 (ValueError below, NotImplementedError above);
    M: (N, 3, 3) destination -> source matrices."""
    frames, n = _fits('ovs_object', fits, ctx)
    m = _mats('ovs_object', M, n)
    dev, ctx, d, oh, ow = _stage_in('ovs_object', frames, ctx, PIXEL_DTYPES, _px_host, (ff,), ndims=(3,))
    if not _is_dev(ff):
        ff = np.asarray(ff, dtype=np.float64)
    if len(ff.shape) != 2:
        raise ValueError('ovs_object: the flat field must be a 2-D float64 array')
    d_ff = _f64_frame('ovs_object', 'the flat field', ff, ff.shape, ctx)
    fh, fw = d_ff.shape
    d_obj = DeviceArray(ctx, (oh, ow), np.float64)
    d_cnt = DeviceArray.counts(ctx, (oh, ow))
    ctx._check(ctx._lib.ipa_ovs_object_dev(
        ctx.handle, d_ff.ptr, fh, fw, fw, d.ptr, dtype_id(d.dtype), n, oh, ow, ow, oh * ow, _dptr(m),
        d_obj.ptr, ow, d_cnt.ptr, ow), 'ovs_object')
    return _stage_out(dev, d_obj), _stage_out(dev, d_cnt)


def ovs_flatfield(obj, fits, masks, M, ff_shape, ctx=None, *, clip=False, sub_step=0):
    """camera/flatField/vignettingFromRandomSteps.py:253-265 in one launch -> (flat field, count),
    float64 and int32 of shape ff_shape: per pixel the running mean over the fitted images, in
    order, of v_k = nan_to_num(sample(div_k, M[k] * (x, y, 1))) where v_k != 0; div_k is fit_k /
    obj with NaN where masks[k] is set and is never stored (ipa_ovs_flatfield_dev).  obj: float64
    (oh, ow); fits as in ovs_object; masks: uint8 / bool (N, oh, ow).  Keyword only: clip=True
    stores np.clip(., 0, 1); sub_step=s > 0 appends a host float64 array, the unclipped result at
    [::s, ::s] - what the loop's residuum reads."""
    frames, n = _fits('ovs_flatfield', fits, ctx)
    m = _mats('ovs_flatfield', M, n)
    dev, ctx, d, oh, ow = _stage_in('ovs_flatfield', frames, ctx, PIXEL_DTYPES, _px_host, (obj, masks),
                                    ndims=(3,))
    d_obj = _f64_frame('ovs_flatfield', 'the object', obj, (oh, ow), ctx)
    d_masks = _u8_frame('ovs_flatfield', 'the masks', masks, (n, oh, ow), ctx)
    fh, fw = int(ff_shape[0]), int(ff_shape[1])
    if fh < 1 or fw < 1:
        raise ValueError('ovs_flatfield: empty flat field %s' % (tuple(ff_shape),))
    s = int(sub_step)
    d_ff = DeviceArray(ctx, (fh, fw), np.float64)
    d_cnt = DeviceArray.counts(ctx, (fh, fw))
    d_sub = DeviceArray(ctx, (-(-fh // s), -(-fw // s)), np.float64) if s > 0 else None
    ctx._check(ctx._lib.ipa_ovs_flatfield_dev(
        ctx.handle, d_obj.ptr, ow, d.ptr, dtype_id(d.dtype), n, oh, ow, ow, oh * ow, d_masks.ptr, ow, oh * ow,
        _dptr(m), d_ff.ptr, fh, fw, fw, d_cnt.ptr, fw, 1 if clip else 0, d_sub.ptr if s > 0 else None,
        max(s, 1), d_sub.shape[1] if s > 0 else 0), 'ovs_flatfield')
    out = (_stage_out(dev, d_ff), _stage_out(dev, d_cnt))
    return out + (d_sub.get(),) if s > 0 else out


def masked_running_mean_update(avg, n, data, mask=None, ctx=None):
    """one ``MaskedMovingAverage.update(data, mask)`` (camera/flatField/vignettingFromRandomSteps.py
    :146-151) -> (avg, n): where mask is set (None: everywhere) n += 1 and avg = data if n == 1
    else avg + (data - avg) / n (ipa_masked_running_mean_dev).  avg: float64, n: int32; DeviceArrays
    are updated in place and returned, host arrays are left alone and new ones returned.  data:
    uint8 / uint16 / float32 / float64; mask: uint8 / bool."""
    dev, ctx, d_avg, h, w = _stage_in('masked_running_mean_update', avg, ctx, (np.float64,), _f64_host,
                                      (n, data, mask))
    if dev:
        if not _is_dev(n) or n.dtype != np.int32 or tuple(n.shape) != (h, w):
            raise ValueError('masked_running_mean_update: a device average needs int32 device counts of its shape')
        d_n = n
    else:
        cnt = np.ascontiguousarray(n, dtype=np.int32)
        if cnt.shape != (h, w):
            raise ValueError('masked_running_mean_update: average and counts differ in shape')
        d_n = DeviceArray.counts(ctx, (h, w))
        d_n.set(cnt)
    d_data = data if _is_dev(data) else ctx.to_device(_px_host(data))
    if d_data.dtype not in PIXEL_DTYPES:
        raise TypeError('masked_running_mean_update needs uint8 / uint16 / float32 / float64 data (got %s)'
                        % d_data.dtype)
    if tuple(d_data.shape) != (h, w):
        raise ValueError('masked_running_mean_update: data of shape %s for an average of shape %s'
                         % (tuple(d_data.shape), (h, w)))
    d_mask = None if mask is None else _u8_frame('masked_running_mean_update', 'the mask', mask, (h, w), ctx)
    ctx._check(ctx._lib.ipa_masked_running_mean_dev(
        ctx.handle, d_avg.ptr, w, d_n.ptr, w, d_data.ptr, dtype_id(d_data.dtype), w,
        d_mask.ptr if d_mask is not None else None, w, h, w), 'masked_running_mean_update')
    return _stage_out(dev, d_avg), _stage_out(dev, d_n)
