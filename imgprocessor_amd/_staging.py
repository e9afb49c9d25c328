"""How the functional layer (ops.py and every ops_*.py family) takes its arrays: host numpy arrays
are staged to the device and the result comes back as numpy, DeviceArrays stay in HBM.  The one
home of the staging helpers: no family imports them from another."""
import ctypes as C

import numpy as np

from . import _lib as L
from .device import DeviceArray, default_context

# the element types of a camera frame: what the calibration kernels read as they are
PIXEL_DTYPES = (np.uint8, np.uint16, np.float32, np.float64)


def _is_dev(a):
    return isinstance(a, DeviceArray)


def _ctx_of(*arrs, **kw):
    ctx = kw.get('ctx')
    for a in arrs:
        if _is_dev(a):
            if ctx is not None and a.ctx is not ctx:
                raise ValueError('arrays live on different contexts')
            ctx = a.ctx
    return ctx or default_context()


def _p(a):
    return a.ptr if _is_dev(a) else a.ctypes.data_as(C.c_void_p)


def _dptr(a):
    """const double* to a C-contiguous float64 ndarray (the pointer keeps the array alive)"""
    return a.ctypes.data_as(L._dp)


def _dev_out(ctx, out, shape, dtype):
    if out is None:
        return DeviceArray(ctx, shape, dtype)
    if not _is_dev(out) or out.shape != tuple(shape) or out.dtype != np.dtype(dtype):
        raise ValueError('out must be a DeviceArray of shape %s dtype %s' % (shape, dtype))
    return out


def _stage_in(name, x, ctx, dtypes=None, host=None, others=(), ndims=(2,), bad_shape=ValueError):
    """One image of a single-image op, host array or DeviceArray -> (dev, ctx, d_in, h, w).
    A host array goes through `host` (which may refuse it; None: the op takes DeviceArrays
    only) and up to the device.  `dtypes`: what the kernel takes (None: the library decides),
    TypeError otherwise; `bad_shape`: what a wrong number of dimensions raises.  `others` may
    be DeviceArrays too and must live on the same context."""
    dev = _is_dev(x)
    if not dev and host is None:
        raise TypeError('%s needs a DeviceArray' % name)
    ctx = _ctx_of(x, *others, ctx=ctx)
    d_in = x if dev else ctx.to_device(host(x))
    if dtypes is not None and d_in.dtype not in dtypes:
        raise TypeError('%s needs %s arrays (got %s)'
                        % (name, ' / '.join(np.dtype(t).name for t in dtypes), d_in.dtype))
    if d_in.ndim not in ndims:
        raise bad_shape('%s works on %s-D arrays (got shape %s)'
                        % (name, ' / '.join(str(d) for d in ndims), d_in.shape))
    return dev, ctx, d_in, d_in.shape[-2], d_in.shape[-1]


def _stage_out(dev, d_out):
    """the result as the input came: DeviceArray for a DeviceArray, numpy otherwise"""
    return d_out if dev else d_out.get()


def _px_host(a):
    """host frames: uint8 / uint16 / float32 / float64 as they are, anything else as float64
    (np.asfarray)"""
    a = np.asarray(a)
    return np.ascontiguousarray(a if a.dtype in PIXEL_DTYPES else a.astype(np.float64))


def _f64_host(a):
    return np.ascontiguousarray(a, dtype=np.float64)


def _frame_pair(name, img, img2, ctx=None, others=()):
    """The frame(s) of a call on the device -> (dev, ctx, d_img, d_img2 or None, h, w); dev: the
    first frame came as a DeviceArray.  The kernels read a pair in ONE element type.  The
    reference takes np.asfarray of each frame on its own, so two host frames of different types
    both go up as float64 - never one cast to the other's type; where a DeviceArray is involved
    nothing is converted, and a pair of different types is a ValueError."""
    if img2 is not None and not _is_dev(img) and not _is_dev(img2):
        img, img2 = _px_host(img), _px_host(img2)
        if img.dtype != img2.dtype:
            img, img2 = img.astype(np.float64), img2.astype(np.float64)
    dev, ctx, d, h, w = _stage_in(name, img, ctx, PIXEL_DTYPES, _px_host, (img2,) + tuple(others))
    d2 = None
    if img2 is not None:
        d2 = img2 if _is_dev(img2) else ctx.to_device(_px_host(img2))
        if d2.dtype != d.dtype or tuple(d2.shape) != tuple(d.shape):
            raise ValueError('%s: img2 (%s %s) must match the image\'s shape and dtype (%s %s)'
                             % (name, d2.dtype, tuple(d2.shape), d.dtype, tuple(d.shape)))
    return dev, ctx, d, d2, h, w


def _side_frame(name, what, a, shape, ctx, dtype, says):
    d = a if _is_dev(a) else ctx.to_device(np.ascontiguousarray(a, dtype=dtype))
    if d.dtype != dtype or tuple(d.shape) != tuple(shape):
        raise ValueError('%s: %s must be a %s array of shape %s (got %s %s)'
                         % (name, what, says, tuple(shape), d.dtype, tuple(d.shape)))
    return d


def _f64_frame(name, what, a, shape, ctx):
    """a float64 side array of the given shape (signal, noise, a fitted plane) on the device"""
    return _side_frame(name, what, a, shape, ctx, np.float64, 'float64')


def _u8_frame(name, what, a, shape, ctx):
    """a uint8 / bool side array of the given shape (a mask, a stack of masks) on the device"""
    return _side_frame(name, what, a, shape, ctx, np.uint8, 'uint8 / bool')


def _bg(name, bg, shape, ctx):
    """`img - bg` -> (device float64 frame or None, its pointer, pitch, scalar).  The frame is
    returned so that the caller holds it until after the launch: a block that went back to the
    context's pool would be handed out again as the result."""
    if bg is None:
        return None, None, 0, 0.0
    if not _is_dev(bg) and np.ndim(bg) == 0:
        return None, None, 0, float(bg)
    if not _is_dev(bg):
        bg = np.broadcast_to(np.asarray(bg, dtype=np.float64), shape)
    d = _f64_frame(name, 'bg', bg, shape, ctx)
    return d, d.ptr, shape[1], 0.0


def check_dev_frames(name, frames):
    """a non-empty list of DeviceArrays must share shape, dtype and context; nothing is allocated"""
    f0 = frames[0]
    for f in frames:
        if f.shape != f0.shape or f.dtype != f0.dtype or f.ctx is not f0.ctx:
            raise ValueError('%s: device frames must share shape, dtype and context' % name)


def gather_dev(name, frames):
    """a list of DeviceArrays (grey or colour) -> one (n, ...) DeviceArray, copied on the device"""
    check_dev_frames(name, frames)
    f0 = frames[0]
    st = DeviceArray(f0.ctx, (len(frames),) + f0.shape, f0.dtype)
    for k, f in enumerate(frames):
        DeviceArray._wrap(st.ctx, C.c_void_p(st.ptr.value + k * f0.nbytes), f0.shape, f0.dtype, False,
                          base=st).copy_from(f)
    return st


def frame_stack(name, imgs, ndims=(2,)):
    """A stack, or a list of frames that are all on the host or all on the device -> a host
    (n, ...) array or one DeviceArray: an array or a DeviceArray as it is, host frames through
    np.stack, device frames gathered on the device.  TypeError for a mix, ValueError for frames
    that have none of the `ndims` numbers of dimensions; an empty list gives an empty (0, 0, 0)
    array, which every caller refuses by its frame count."""
    if _is_dev(imgs) or isinstance(imgs, np.ndarray):
        st = imgs
    else:
        frames = list(imgs)
        dev = [_is_dev(f) for f in frames]
        if any(dev) and not all(dev):
            raise TypeError('%s: mix of host and device frames' % name)
        if not frames:
            st = np.empty((0, 0, 0))
        else:
            st = gather_dev(name, frames) if dev[0] else np.stack([np.asarray(f) for f in frames])
    if len(st.shape) - 1 not in ndims:
        raise ValueError('%s takes a stack or a list of frames of %s dimensions (got shape %s)'
                         % (name, ' or '.join(str(d) for d in ndims), tuple(st.shape)))
    return st
