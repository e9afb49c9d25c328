"""Pixel sensitivity from homogeneously illuminated frames: the reference's
camera/flatField/sensitivity.py (section 5 of K. Bedrich, M. Bokalic et al., Electroluminescence
imaging of PV devices: advanced flat field calibration, 2017).

Per frame ``i = frame - bg`` in float64, ``smooth = fastMean(median_filter(i, 3), f)`` and
``out += i / smooth``; at the end ``out /= n``.  Two HIP kernels per frame (csrc/flat.hip):
ops.sens_shrink goes from the frame to fastMean's small image without writing the median frame,
ops.sens_accumulate enlarges the small image per pixel and steps the accumulator.  A frame is read
twice and the float64 accumulator is read and written once.

Frames are (h, w) arrays, uint8 / uint16 / float32 / float64, host arrays or DeviceArrays (a list
or one stack); host frames give a numpy array, device frames a DeviceArray.  ``bg`` is what
utils/getBackground.py takes: None, one frame, or several frames (their STE-free average).
``f`` is an extension: the reference fixes fastMean's default of 10.
"""
import numpy as np

from ... import ops, ops_flat
from ...device import DeviceArray, default_context
from ...utils.getBackground import getBackground
from .flatFieldFromCloseDistance import _ctx_of, _on_device, _stack, _view


def _bg_shape(bg):
    """the frame shape of what getBackground takes, without touching it: None for no frame"""
    if bg is None or (not isinstance(bg, DeviceArray) and np.ndim(bg) == 0):
        return None
    if isinstance(bg, (tuple, list)):
        return tuple(bg[0].shape) if isinstance(bg[0], DeviceArray) else np.shape(bg[0])
    shape = tuple(bg.shape) if isinstance(bg, DeviceArray) else np.shape(bg)
    return shape[1:] if len(shape) == 3 else shape


def sensitivity(imgs, bg=None, f=10):
    dev, n, shape, st = _stack('sensitivity', imgs, (2,))
    if n < 1:
        raise ValueError('sensitivity: no images')
    h, w = shape
    dh, dw = ops_flat.small_shape((h, w), f)
    if _bg_shape(bg) not in (None, (h, w)):
        raise ValueError('sensitivity: the background %s differs from the frames %s' % (_bg_shape(bg), (h, w)))
    # ---- nothing above touches a device
    ctx = _ctx_of(st) if dev else default_context()
    d = _on_device(ctx, st)
    bg = getBackground(bg)
    if not isinstance(bg, DeviceArray) and np.ndim(bg) != 0:
        bg = ctx.to_device(np.ascontiguousarray(bg, dtype=np.float64))
    elif isinstance(bg, DeviceArray) and bg.dtype != np.float64:
        bg = ops.stack_mean(_view(bg, (1,) + bg.shape))   # as float64
    small = DeviceArray(ctx, (dh, dw), np.float64)
    out = DeviceArray(ctx, (h, w), np.float64)
    for k in range(n):
        frame = d.frame(k)
        ops.sens_shrink(frame, bg, f, out=small)
        ops.sens_accumulate(frame, small, out, bg, first=k == 0, n_last=n if k == n - 1 else 0)
    return out if dev else out.get()
