"""How the functional layer (ops.py, ops_nlf.py) takes its arrays: host numpy arrays are staged
to the device and the result comes back as numpy, DeviceArrays stay in HBM."""
import ctypes as C

import numpy as np

from . import _lib as L
from .device import DeviceArray, default_context


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
