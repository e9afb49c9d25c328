"""The signal-stability family of ``ops`` (csrc/tss.hip), re-exported there as
``ops.tss_event_length`` and ``ops.tss_finish``.  Like every family it goes through ``_stage_in`` /
``_stage_out``: host arrays in give host arrays out, DeviceArrays stay on the device.
"""
import numpy as np

from .device import DeviceArray, dtype_id
from ._staging import (PIXEL_DTYPES, _dptr, _f64_frame, _f64_host, _px_host, _stage_in, _stage_out, _u8_frame,
                       frame_stack)

MAX_FRAMES = 64   # kTssMaxT of csrc/tss.hip


def tss_event_length(stack, times, offset, ascent, error, events=False, ctx=None, *, zero_mask=False):
    """uncertainty/temporalSignalStability.py:56-66 and _calcAvgLen in one launch -> avlen, float64
    (h, w): the average length of the runs of event frames, an event being
    |median_filter(stack - (offset + t * ascent), 5)| > 0.5 * error, decided by counting the window
    values beyond +-0.5 * error instead of selecting the median (ipa_tss_event_length_dev, where the
    arithmetic is spelled out).  stack: a (T, h, w) array or a list of T frames, uint8 / uint16 /
    float32 / float64, 2 <= T <= 64 (ValueError below, NotImplementedError above); offset, ascent,
    error: float64 (h, w), what ops.stack_linregress returns.  events=True: (avlen, events), the
    uint8 (T, h, w) event cube; zero_mask=True (keyword only) appends the uint8 mask avlen == 0.
    Undefined for NaN samples."""
    frames = frame_stack('tss_event_length', stack)
    t = np.ascontiguousarray(np.asarray(times, dtype=np.float64).ravel())
    n = frames.shape[0]
    if t.size != n:
        raise ValueError('tss_event_length: %d times for %d frames' % (t.size, n))
    if n < 2:
        raise ValueError('tss_event_length: needs at least 2 frames (got %d)' % n)
    if n > MAX_FRAMES:
        raise NotImplementedError('tss_event_length: at most %d frames (got %d)' % (MAX_FRAMES, n))
    dev, ctx, d, h, w = _stage_in('tss_event_length', frames, ctx, PIXEL_DTYPES, _px_host,
                                  (offset, ascent, error), ndims=(3,))
    planes = [_f64_frame('tss_event_length', name, a, (h, w), ctx)
              for name, a in (('offset', offset), ('ascent', ascent), ('error', error))]
    d_avlen = DeviceArray(ctx, (h, w), np.float64)
    d_events = DeviceArray(ctx, (n, h, w), np.uint8) if events else None
    d_mask = DeviceArray(ctx, (h, w), np.uint8) if zero_mask else None
    ctx._check(ctx._lib.ipa_tss_event_length_dev(
        ctx.handle, d.ptr, dtype_id(d.dtype), n, h, w, w, h * w, _dptr(t), planes[0].ptr, planes[1].ptr,
        planes[2].ptr, w, d_avlen.ptr, w, d_mask.ptr if zero_mask else None, w,
        d_events.ptr if events else None, w, h * w), 'tss_event_length')
    out = [_stage_out(dev, a) for a in (d_avlen, d_events, d_mask) if a is not None]
    return out[0] if len(out) == 1 else tuple(out)


def tss_finish(mean, mask, ctx=None):
    """the tail of uncertainty/temporalSignalStability.py (:72-78) -> float64 (h, w): the mask
    dilated 3 x 3, zeros written there, a 3 x 3 maximum and a 3 x 3 median whose zeros are those of
    the maximum, the edge repeated (ipa_tss_finish_dev).  mean: float64, NaN where masked - what
    ops.masked_mean(raw, mask, 7, fill_mask=False, fn='mean') returns; mask: uint8 / bool, raw == 0."""
    dev, ctx, d, h, w = _stage_in('tss_finish', mean, ctx, (np.float64,), _f64_host, (mask,))
    if dev and not isinstance(mask, DeviceArray):
        raise TypeError('tss_finish: device array needs a device mask')
    d_mask = _u8_frame('tss_finish', 'the mask', mask, (h, w), ctx)
    d_out = DeviceArray(ctx, (h, w), np.float64)
    ctx._check(ctx._lib.ipa_tss_finish_dev(ctx.handle, d.ptr, d_mask.ptr, h, w, w, w, d_out.ptr, w),
               'tss_finish')
    return _stage_out(dev, d_out)
