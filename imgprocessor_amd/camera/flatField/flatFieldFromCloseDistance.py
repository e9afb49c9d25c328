"""Flat field from close-distance frames: the reference's
camera/flatField/flatFieldFromCloseDistance.py ("Method A" of K. Bedrich, M. Bokalic et al.,
Electroluminescence imaging of PV devices: advanced flat field calibration, 2017).

Frames of a homogeneous device held directly in front of the lens are averaged, the background is
subtracted and the result is scaled by an artefact-free maximum,
``median_filter(img[::10, ::10], 3).max()``.  Every frame pass runs in HIP kernels (csrc/flat.hip,
csrc/ste.hip, csrc/nlf.hip); what stays on the host is the sort of the frames by one number each
and, in the second variant, the noise level function's fit over ~50 bins.

Frames are uint8 / uint16 / float32 / float64 arrays, host arrays or DeviceArrays (a list of
frames or one stack).  Host frames are uploaded once and the result comes back as a numpy array;
with device frames nothing but scalars leaves the device and the result is a DeviceArray.  The
result feeds ``CameraCalibration.addFlatField`` (``.get()`` for a DeviceArray).

Differences from the reference:
  - ``bg_imgs`` / ``bgImages`` = None raises NotImplementedError (see utils/getBackground2.py).
  - ``flatFieldFromCloseDistance``: the reference calls ``toGray`` unconditionally and so works on
    colour frames (h, w, 3) only; (h, w) frames skip the grey step here instead of raising.
  - ``flatFieldFromCloseDistance2``: ``calcStd=True`` raises NotImplementedError (the variance of the
    running mean is not part of the HIP path); fewer than two images raise ValueError (the
    reference falls over an unbound name).  Everything else follows the reference as written: the
    frames are sorted by ``-img[::s0 // 10, ::s1 // 10].min()`` in their own type (the key wraps for
    unsigned frames), the first two frames of that order start the single-time-effect detection
    minus the background, and all frames from the second one on are added raw.
  - frames are arrays, not file paths (TypeError).
"""
import ctypes as C
import numbers

import numpy as np

from ... import ops
from ..._staging import _px_host, check_dev_frames, gather_dev
from ...device import DeviceArray, default_context
from ...features.SingleTimeEffectDetection import SingleTimeEffectDetection
from ...utils.getBackground2 import getBackground2
from ..NoiseLevelFunction import oneImageNLF

GRID = 10   # the maximum is taken over every 10th pixel


def _is_path(f):
    return isinstance(f, (str, bytes)) or hasattr(f, '__fspath__')


def _stack(name, images, ndims):
    """the refusals of a list of frames or a stack -> (dev, n, frame shape, the stack - for a list
    of device frames the list).  Nothing is allocated or uploaded."""
    if _is_path(images):
        raise TypeError('%s takes arrays, not file paths' % name)
    if isinstance(images, (np.ndarray, DeviceArray)):
        st = images
        n, shape = (st.shape[0], tuple(st.shape[1:])) if len(st.shape) else (0, ())
    else:
        st = list(images)
        if any(_is_path(f) for f in st):
            raise TypeError('%s takes arrays, not file paths' % name)
        dev = [isinstance(f, DeviceArray) for f in st]
        if any(dev) and not all(dev):
            raise TypeError('%s: mix of host and device frames' % name)
        if st and dev[0]:
            check_dev_frames(name, st)
        elif st:
            st = np.stack([np.asarray(f) for f in st])
        n, shape = len(st), (tuple(st[0].shape) if len(st) else ())
    if n and len(shape) not in ndims:
        raise ValueError('%s takes frames of %s dimensions (got frames of shape %s)'
                         % (name, ' or '.join(str(d) for d in ndims), shape))
    return n > 0 and not isinstance(st, np.ndarray), n, shape, st


def _ctx_of(st):
    return (st if isinstance(st, DeviceArray) else st[0]).ctx


def _on_device(ctx, st):
    """what _stack returned as one DeviceArray"""
    if isinstance(st, DeviceArray):
        return st
    return gather_dev('frames', st) if isinstance(st, list) else ctx.to_device(_px_host(st))


def _view(d, shape, k=0):
    """frame k of the DeviceArray d, taken as `shape` (no copy)"""
    nbytes = int(np.prod(shape, dtype=np.int64)) * d.dtype.itemsize
    return DeviceArray._wrap(d.ctx, C.c_void_p(d.ptr.value + k * nbytes), shape, d.dtype, False, base=d)


def _background(name, bg, shape):
    """the refusals of getBackground2 and of its frames -> a number or the background stack;
    nothing is uploaded"""
    if bg is None or (isinstance(bg, numbers.Number) and not isinstance(bg, bool)):
        return getBackground2(bg)
    _, n, bg_shape, st = _stack(name, bg, (len(shape),))
    if n < 1:
        raise ValueError('%s: no background images' % name)
    if bg_shape != tuple(shape):
        raise ValueError('%s: background frames %s differ from the images %s' % (name, bg_shape, tuple(shape)))
    return st


def _average_bg(ctx, bg):
    """getBackground2 of what _background returned -> a number or a float64 DeviceArray"""
    return bg if isinstance(bg, numbers.Number) else getBackground2(_on_device(ctx, bg))


def flatFieldFromCloseDistance(imgs, bg_imgs=None):
    """average of `imgs` minus the background, as grey values, scaled by
    median_filter(img[::10, ::10], 3).max() -> float64 (h, w)"""
    name = 'flatFieldFromCloseDistance'
    if bg_imgs is None:
        getBackground2(None)
    dev, n, shape, st = _stack(name, imgs, (2, 3))
    if n < 1:
        raise ValueError('%s: no images' % name)
    if len(shape) == 3 and shape[2] != 3:
        raise ValueError('%s: colour frames are (h, w, 3) (got %s)' % (name, shape))
    bg = _background(name, bg_imgs, shape)
    # ---- nothing above touches a device
    ctx = _ctx_of(st) if dev else default_context()
    row = (shape[0], int(np.prod(shape[1:])))
    img = _view(ops.stack_mean(_on_device(ctx, st)), row)
    bg = _average_bg(ctx, bg)
    ops.flat_scale(img, bg=_view(bg, row) if isinstance(bg, DeviceArray) else bg, out=img)
    if len(shape) == 3:
        img = ops.luma(_view(img, shape))
    mx = ops.strided_median_max(img, GRID)
    ops.flat_scale(img, div=mx, out=img)
    return img if dev else img.get()


def flatFieldFromCloseDistance2(images, bgImages=None, calcStd=False, nlf=None, nstd=6):
    """as flatFieldFromCloseDistance, with single-time effects and erroneously dark areas kept out
    of the average.  nlf: a noise level function (see SingleTimeEffectDetection); None: estimated
    from the two brightest frames (oneImageNLF)."""
    name = 'flatFieldFromCloseDistance2'
    if calcStd:
        raise NotImplementedError('calcStd: the variance of the running mean is not part of the HIP path')
    if bgImages is None:
        getBackground2(None)
    dev, n, shape, st = _stack(name, images, (2,))
    if n < 2:
        raise ValueError('%s needs at least 2 images (got %d)' % (name, n))
    h, w = shape
    s0, s1 = h // GRID, w // GRID
    if s0 == 0 or s1 == 0:
        raise ValueError('slice step cannot be zero: frames of fewer than %d rows or columns (%d x %d)'
                         % (GRID, h, w))
    if nlf is not None and not callable(nlf) and len(tuple(float(v) for v in nlf)) != 3:
        raise TypeError('nlf must be a callable or a (minY, ax, ay) triple')
    bg = _background(name, bgImages, (h, w))
    # ---- nothing above touches a device
    ctx = _ctx_of(st) if dev else default_context()
    d = _on_device(ctx, st)
    frames = [d.frame(k) for k in range(n)]
    # start with the brightest images: the key in the frame's own type, as numpy negates it
    with np.errstate(over='ignore'):
        keys = [np.negative(ops.strided_min(f, s0, s1)) for f in frames]
    frames = [frames[k] for k in sorted(range(n), key=lambda k: keys[k])]
    bg = _average_bg(ctx, bg)
    i0, i1 = (ops.flat_scale(ops.stack_mean(_view(f, (1, h, w))), bg=bg) for f in frames[:2])
    if nlf is None:
        nlf = oneImageNLF(i0, i1)[0]
    det = SingleTimeEffectDetection([i0, i1], nlf, nStd=nstd)
    device_nlf = ops.nlf_params(nlf) is not None
    mask = DeviceArray(ctx, (h, w), np.uint8)
    for f in frames[1:]:
        # exclude erroneously darker areas
        if device_nlf:
            ops.nlf_lower_mask(f, det.noSTE, nlf, nstd, out=mask)
        else:
            avg = det.noSTE.get()   # a host function: the round trip SingleTimeEffectDetection documents
            with np.errstate(invalid='ignore'):
                mask.set((f.get() > avg - nlf(avg) * nstd).astype(np.uint8))
        det.addImage(f, mask)
    ma = det.noSTE
    out = ops.flat_scale(ma, div=ops.strided_median_max(ma, GRID))
    return out if dev else out.get()
