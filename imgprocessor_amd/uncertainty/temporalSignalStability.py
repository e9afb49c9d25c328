"""``temporalSignalStability`` — reference: imgProcessor/uncertainty/temporalSignalStability.py:12-107.

An (electroluminescence) signal is not stable over time, especially next to cracks.  From a time
series of corrected frames the function returns, per pixel, the residual of a line fit through
time (the signal uncertainty), the average length of the signal's fluctuation events and the
fit's ascent and offset - what adjustUncertToExposureTime needs to carry an uncertainty over to
another exposure time.

The reference's cost is ``median_filter(diff, 5)`` on the (T, h, w) residual cube.  The median is
used for one comparison only, ``|median| > 0.5 * error``, and that is decided here by counting the
window values beyond the threshold (ops.tss_event_length); no cube is ever written.  Four launches:

  1. ops.stack_linregress(times, imgs, mx_intensity=inf, min_ascent=0): the plain least-squares
     line and its rms residual (linRegressUsingMasked2dArrays(times, imgs, calcError=True)).  Its
     `ascent = 0 where NaN` step only touches pixels that are degenerate already (NaN data, all
     times equal); their offset and error stay NaN and they never hold an event.
  2. ops.tss_event_length: the raw event length and the mask raw == 0 (:56-69).
  3. ops.masked_mean(raw, mask, 7, fill_mask=False, fn='mean'): maskedFilter's own window
     [i - 3, i + 3) (:70).
  4. ops.tss_finish: the two maximum filters and the median filter (:72-78).

``down_scale_factor > 1`` raises NotImplementedError: it is cv2.resize(INTER_AREA) of every frame,
which ops.resize does not offer, and it was the reference's way of making the CPU median bearable.
NaN samples are undefined, as they are in the reference (its median's selection depends on the
order of the values).
"""
import numpy as np

from .. import ops
from .._staging import PIXEL_DTYPES, _px_host, _stage_in, _stage_out, frame_stack
from ..ops_tss import MAX_FRAMES


def temporalSignalStability(imgs, times, down_scale_factor=1, ctx=None):
    """-> (error, avlen, ascent, offset), float64 (h, w), in the reference's order.  imgs: a
    (T, h, w) array, a list of frames, a (T, h, w) DeviceArray or a list of DeviceArrays (uint8 /
    uint16 / float32 / float64, 2 <= T <= 64); times: the T absolute measurement times.  Device
    frames stay on the device and the results are DeviceArrays."""
    if down_scale_factor > 1:
        raise NotImplementedError('temporalSignalStability: down_scale_factor > 1 needs an INTER_AREA resize')
    imgs = frame_stack('temporalSignalStability', imgs)   # a list is stacked once, where its frames live
    t = np.asarray(times, dtype=np.float64).ravel()
    if imgs.shape[0] != t.size:
        raise ValueError('temporalSignalStability: %d times for %d frames' % (t.size, imgs.shape[0]))
    if imgs.shape[0] < 2:
        raise ValueError('temporalSignalStability: a line needs at least 2 frames (got %d)' % imgs.shape[0])
    if imgs.shape[0] > MAX_FRAMES:
        raise NotImplementedError('temporalSignalStability: at most %d frames (got %d)' % (MAX_FRAMES, imgs.shape[0]))
    # host frames go up once; everything between the four launches stays on the device
    dev, ctx, d, _, _ = _stage_in('temporalSignalStability', imgs, ctx, PIXEL_DTYPES, _px_host, ndims=(3,))
    offset, ascent, error = ops.stack_linregress(t, d, mx_intensity=np.inf, min_ascent=0)
    raw, zero = ops.tss_event_length(d, t, offset, ascent, error, zero_mask=True)
    avlen = ops.tss_finish(ops.masked_mean(raw, zero, 7, fill_mask=False, fn='mean'), zero)
    return tuple(_stage_out(dev, a) for a in (error, avlen, ascent, offset))
