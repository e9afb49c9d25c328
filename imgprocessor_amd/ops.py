"""Functional layer over the C ABI: every function takes either host numpy
arrays (staged through the context workspace, result returned as numpy) or
``DeviceArray``s (enqueued on the context stream, result stays in HBM).

Shapes: (h, w) image or (n, h, w) batch of independent frames.
"""
import ctypes as C

import numpy as np

from . import _lib as L
from .device import DeviceArray, default_context, dtype_id, as_frames
from ._staging import (PIXEL_DTYPES, _is_dev, _ctx_of, _p, _dptr, _dev_out, _px_host, _stage_in,  # noqa: F401
                       _stage_out)
# the noise-level-function / SNR family lives in ops_nlf.py
from .ops_nlf import nlf_signal, nlf_moments, nlf_bins, snr_map, snr_bg_median  # noqa: F401
# the dark-current family lives in ops_dark.py
from .ops_dark import (pair_min, nlf_threshold, stack_linregress, dark_current_eval,  # noqa: F401
                       cast_trunc, nlf_params)
# the flat-field family lives in ops_flat.py
from .ops_flat import (stack_mean, luma, strided_median_max, strided_min, flat_scale,  # noqa: F401
                       nlf_lower_mask, sens_shrink, sens_accumulate)
# the signal-stability family lives in ops_tss.py
from .ops_tss import tss_event_length, tss_finish  # noqa: F401
# the object / vignetting separation family lives in ops_ovs.py
from .ops_ovs import ovs_object, ovs_flatfield, masked_running_mean_update  # noqa: F401
# the 2-D polynomial fit family lives in ops_poly.py
from .ops_poly import (poly2d_moments, poly2d_gram, poly2d_solve, poly2d_eval, high_grad_window,  # noqa: F401
                       high_grad_mask, clip01)
# the spot family (histogram, Otsu, labelling) lives in ops_spot.py
from .ops_spot import histogram, otsu_threshold, spot_mask, label, largest_component, spot_take  # noqa: F401
# the discrete-steps family (cell means, the separation loop, the offset grid) lives in ops_steps.py
from .ops_steps import cell_edges, cell_means, steps_separate, offset_meshgrid, isnan_mask  # noqa: F401
# the vignetting-function fit family (Kang-Weiss, angle of view) lives in ops_fn2d.py
from .ops_fn2d import fn2d_normal, fn2d_eval, fn2d_divide, fn2d_fit  # noqa: F401

INTERPOLATIONS = {
    # exact-coordinate forms (scipy / scikit-image semantics)
    'nearest': L.INTER_NEAREST,
    'linear': L.INTER_LINEAR,                 # == map_coordinates(order=1), skimage order=1
    'cubic': L.INTER_CUBIC_KEYS,              # Keys a=-0.5 == skimage order=3
    'cubic_cv': L.INTER_CUBIC_CV,             # Keys a=-0.75, exact coordinates
    # cv2-style: coordinates rounded to 1/32 px (INTER_BITS=5)
    'linear_cv_q5': L.INTER_LINEAR | L.INTER_Q5,
    'cubic_cv_q5': L.INTER_CUBIC_CV | L.INTER_Q5,
    'lanczos4': L.INTER_LANCZOS4,
}
BORDERS = {
    'constant': L.BORDER_CONSTANT, 'replicate': L.BORDER_REPLICATE, 'nearest': L.BORDER_REPLICATE,
    'edge': L.BORDER_REPLICATE, 'reflect': L.BORDER_REFLECT, 'symmetric': L.BORDER_REFLECT,
    'wrap': L.BORDER_WRAP, 'grid-wrap': L.BORDER_WRAP, 'mirror': L.BORDER_REFLECT101,
    'reflect101': L.BORDER_REFLECT101,
}


def interp_id(v):
    if isinstance(v, str):
        try:
            return INTERPOLATIONS[v]
        except KeyError:
            raise ValueError('unknown interpolation %r (one of %s)' % (v, sorted(INTERPOLATIONS)))
    return int(v)


def border_id(v):
    if isinstance(v, str):
        try:
            return BORDERS[v]
        except KeyError:
            raise ValueError('unknown border mode %r (one of %s)' % (v, sorted(BORDERS)))
    return int(v)


def _host(a, dtype=None):
    a = np.ascontiguousarray(a, dtype=dtype)
    dtype_id(a.dtype)
    return a


def _mat3(M):
    return L.dbl(np.ravel(np.asarray(M, dtype=np.float64)), 9)


def _lens(K, dist5, newK):
    """K, dist5 = [k1, k2, p1, p2, k3], newK as the exports take them"""
    return L.dbl(np.ravel(K), 9), L.dbl(np.ravel(dist5)[:5], 5), L.dbl(np.ravel(newK), 9)


def _out_dtype(src_dtype, out_dtype):
    return np.dtype(src_dtype if out_dtype is None else out_dtype)


# ------------------------------------------------------------------ maps --
def to_planes(img, ctx=None):
    """(H, W, C) image (host or device) -> device batch (C, H, W), the layout copy on the device
    (ipa_deinterleave_dev): what cv2.remap / warpPerspective do channel by channel
    (camera/LensDistortion.py:323-326, camera/PerspectiveCorrection.py:401-405)"""
    ctx = _ctx_of(img, ctx=ctx)
    d = img if _is_dev(img) else ctx.to_device(img)
    if d.ndim != 3:
        raise ValueError('to_planes expects a (H,W,C) image')
    h, w, c = d.shape
    out = ctx.empty((c, h, w), d.dtype)
    ctx._check(ctx._lib.ipa_deinterleave_dev(ctx.handle, d.ptr, dtype_id(d.dtype), h, w, c, w * c,
                                             out.ptr, w, h * w), 'deinterleave')
    return out


def from_planes(planes, out=None, ctx=None):
    """device batch (C, H, W) -> device (H, W, C) image (ipa_interleave_dev)"""
    ctx = _ctx_of(planes, ctx=ctx)
    if not _is_dev(planes) or planes.ndim != 3:
        raise TypeError('from_planes expects a device batch (C,H,W)')
    c, h, w = planes.shape
    dst = _dev_out(ctx, out, (h, w, c), planes.dtype)
    ctx._check(ctx._lib.ipa_interleave_dev(ctx.handle, planes.ptr, dtype_id(planes.dtype), h, w, c, w,
                                           h * w, dst.ptr, w * c), 'interleave')
    return dst


def build_undistort_map(K, dist5, newK, h, w, ctx=None, device=False):
    """cv2.initUndistortRectifyMap(K, d, None, newK, (w,h), CV_32FC1)"""
    ctx = ctx or default_context()
    lib = ctx._lib
    K, d, nK = _lens(K, dist5, newK)
    if device:
        mx, my = DeviceArray(ctx, (h, w), np.float32), DeviceArray(ctx, (h, w), np.float32)
        ctx._check(lib.ipa_build_undistort_map_dev(ctx.handle, K, d, nK, h, w, mx.ptr, my.ptr, w),
                   'build_undistort_map')
        return mx, my
    mx, my = np.empty((h, w), np.float32), np.empty((h, w), np.float32)
    ctx._check(lib.ipa_build_undistort_map(ctx.handle, K, d, nK, h, w, _p(mx), _p(my)),
               'build_undistort_map')
    return mx, my


def _check_dev_maps(mapx, mapy):
    """device maps are read with plain (not range-checked) loads: refuse anything that is not a
    pair of equally shaped 2-D float32 arrays instead of reinterpreting it"""
    if not (_is_dev(mapx) and _is_dev(mapy)):
        raise TypeError('device source needs device maps')
    if mapx.dtype != np.float32 or mapy.dtype != np.float32:
        raise TypeError('mapx/mapy must be float32 (got %s / %s)' % (mapx.dtype, mapy.dtype))
    if mapx.ndim != 2 or tuple(mapx.shape) != tuple(mapy.shape):
        raise ValueError('mapx/mapy must be 2-D and of equal shape (got %s / %s)'
                         % (mapx.shape, mapy.shape))


# ----------------------------------------------------------------- remap --
def _fused_dtype(src_dtype, separable):
    """what the remap -> filter chains write: float64 for float64 frames under a dense kernel,
    float32 for everything else and for every separable chain"""
    return np.dtype(np.float64 if not separable and src_dtype == np.float64 else np.float32)


def _dense_filt(kernel, conv_mode):
    k = np.ascontiguousarray(kernel, dtype=np.float64)
    return (_dptr(k), k.shape[0], k.shape[1]), conv_mode, False


def _sep_filt(ky, kx, conv_mode):
    ky = np.ascontiguousarray(ky, dtype=np.float64).ravel()
    kx = np.ascontiguousarray(kx, dtype=np.float64).ravel()
    return (_dptr(ky), ky.size, _dptr(kx), kx.size), conv_mode, True


def _geometry(name, src, coords, out_hw, interpolation, border_mode, border_value, out_dtype, out,
              ctx, filt=None):
    """The call that remap, undistort, warp_perspective, warp_grid and their chains share:
    ipa_<name>_dev for a DeviceArray source, the host-pointer ipa_<name> for anything else.
    Either takes the source (pointer, dtype, h, w[, pitch]), then `coords` - the export's own
    middle (maps, lens model, matrix, cells) in the form that goes with the source - then
    `filt` for a chain (_dense_filt / _sep_filt), then the result (pointer, dtype, h, w[, pitch])
    with the frame count[, frame strides], the sampling and the filter's border pair.  Arrays
    are dense: pitches are the widths, frame strides h * w.  out_hw None: the source's shape."""
    interp, border = interp_id(interpolation), border_id(border_mode)
    dev = _is_dev(src)
    ctx = _ctx_of(src, ctx=ctx)
    if not dev:
        src = _host(src)
    n, sh, sw = as_frames(src)
    dh, dw = out_hw or (sh, sw)
    if filt is None:
        taps, conv, odt = (), (), _out_dtype(src.dtype, out_dtype)
    else:
        taps, conv_mode, separable = filt
        conv, odt = (border_id(conv_mode),) * 2, _fused_dtype(src.dtype, separable)
    oshape = (dh, dw) if len(src.shape) == 2 else (n, dh, dw)
    sampling = (interp, border, float(border_value)) + conv
    if dev:
        dst = _dev_out(ctx, out, oshape, odt)
        status = getattr(ctx._lib, 'ipa_%s_dev' % name)(
            ctx.handle, src.ptr, dtype_id(src.dtype), sh, sw, sw, *coords, *taps,
            dst.ptr, dtype_id(odt), dh, dw, dw, n, sh * sw, dh * dw, *sampling)
    else:
        dst = np.empty(oshape, odt)
        status = getattr(ctx._lib, 'ipa_%s' % name)(
            ctx.handle, _p(src), dtype_id(src.dtype), sh, sw, *coords,
            _p(dst), dtype_id(odt), dh, dw, n, *sampling)
    ctx._check(status, name)
    return dst


def _dev_only(name, ctx, *arrs):
    """the chains take DeviceArrays only -> their context"""
    ctx = _ctx_of(*arrs, ctx=ctx)
    if not all(_is_dev(a) for a in arrs):
        raise TypeError('%s works on DeviceArrays (use Context.to_device)' % name)
    return ctx


def remap(src, mapx, mapy, interpolation='linear', border_mode='constant', border_value=0.0,
          out_dtype=None, out=None, ctx=None, map_roi=None):
    """cv2.remap(src, mapx, mapy, ...).  map_roi=(x, y, w, h) (device maps only)
    evaluates just that window of the maps — the keepSize=False crop of
    LensDistortion.correct without computing the discarded border."""
    if _is_dev(src):
        ctx = _ctx_of(src, mapx, mapy, ctx=ctx)
        _check_dev_maps(mapx, mapy)
        mh, mw = mapx.shape
        dh, dw, moff = mh, mw, 0
        if map_roi is not None:
            rx, ry, rw, rh = [int(v) for v in map_roi]
            if not (0 <= rx and 0 <= ry and rw > 0 and rh > 0 and rx + rw <= mw and ry + rh <= mh):
                raise ValueError('map_roi %s outside the %dx%d maps' % (map_roi, mh, mw))
            dh, dw, moff = rh, rw, (ry * mw + rx) * 4
        coords = (C.c_void_p(mapx.ptr.value + moff), C.c_void_p(mapy.ptr.value + moff), mw)
    else:
        if map_roi is not None:
            raise ValueError('map_roi needs device arrays')
        ctx = ctx or default_context()
        mapx, mapy = _host(mapx, np.float32), _host(mapy, np.float32)
        if mapx.shape != mapy.shape or mapx.ndim != 2:
            raise ValueError('mapx/mapy must be 2-D and of equal shape')
        dh, dw = mapx.shape
        coords = (_p(mapx), _p(mapy))
    return _geometry('remap', src, coords, (dh, dw), interpolation, border_mode, border_value,
                     out_dtype, out, ctx)


def undistort(src, K, dist5, newK=None, interpolation='linear', border_mode='constant',
              border_value=0.0, out_dtype=None, out_shape=None, out=None, ctx=None):
    """LensDistortion.correct without map arrays (analytic coordinates)"""
    return _geometry('undistort', src, _lens(K, dist5, K if newK is None else newK), out_shape,
                     interpolation, border_mode, border_value, out_dtype, out, ctx)


def warp_perspective(src, M_dst2src, out_shape, interpolation='linear', border_mode='constant',
                     border_value=0.0, out_dtype=None, out=None, ctx=None):
    """cv2.warpPerspective with M the DESTINATION->SOURCE matrix (pass inv(H)
    for a plain call, H for WARP_INVERSE_MAP)"""
    return _geometry('warp_perspective', src, (_mat3(M_dst2src),),
                     (int(out_shape[0]), int(out_shape[1])), interpolation, border_mode,
                     border_value, out_dtype, out, ctx)


def _grid_cells(cell_rects, cell_M):
    rects = np.ascontiguousarray(cell_rects, dtype=np.int32)
    M = np.ascontiguousarray(cell_M, dtype=np.float64)
    if rects.ndim != 2 or rects.shape[1] != 4:
        raise ValueError('cell_rects must have shape (n, 4): x0, y0, w, h (got %s)' % (rects.shape,))
    n = rects.shape[0]
    if M.size != 9 * n or M.shape[0] != n:
        raise ValueError('cell_M must hold one 3x3 matrix per cell (got %s for %d cells)'
                         % (M.shape, n))
    return rects, M, n


def warp_grid_plan(cell_rects, out_shape):
    """who owns which pixel of a piecewise warp (ipa_warp_grid_plan; host only, no device):
    -> (colband (dw,) uint16, rowband (dh,) uint16, owner (n_rowbands, n_colbands) int16), the
    pixel (x, y) belongs to cell owner[rowband[y], colband[x]], -1 = none"""
    rects = np.ascontiguousarray(cell_rects, dtype=np.int32).reshape(-1, 4)
    dh, dw = int(out_shape[0]), int(out_shape[1])
    lib = L.lib()
    nr, nc = C.c_int(0), C.c_int(0)
    rp = rects.ctypes.data_as(L._ip)
    L.check(lib.ipa_warp_grid_plan(rp, rects.shape[0], dh, dw, None, None, None, C.byref(nr),
                                   C.byref(nc)), None, 'warp_grid_plan')
    col, row = np.empty(dw, np.uint16), np.empty(dh, np.uint16)
    owner = np.empty((nr.value, nc.value), np.int16)
    L.check(lib.ipa_warp_grid_plan(rp, rects.shape[0], dh, dw, _p(col), _p(row), _p(owner),
                                   C.byref(nr), C.byref(nc)), None, 'warp_grid_plan')
    return col, row, owner


def warp_grid(src, cell_rects, cell_M, out_shape, interpolation='linear', border_mode='constant',
              border_value=0.0, out_dtype=None, out=None, ctx=None):
    """piecewise cv2.warpPerspective in one launch (PerspectiveCorrection.correctGrid): cell i
    paints the rectangle cell_rects[i] = (x0, y0, w, h) of the output through cell_M[i], the 3x3
    matrix from the cell's LOCAL destination pixel (X - x0, Y - y0, 1) to the source - bit for bit
    ``warp_perspective(src, cell_M[i], (h, w), ...)`` pasted there.  Rectangles come in paint
    order; where they overlap the last one wins.  Pixels no rectangle covers receive what a
    pixel wholly outside the source receives under 'constant' with border_value."""
    rects, M, nc = _grid_cells(cell_rects, cell_M)
    return _geometry('warp_grid', src, (rects.ctypes.data_as(L._ip), _dptr(M), nc),
                     (int(out_shape[0]), int(out_shape[1])), interpolation, border_mode,
                     border_value, out_dtype, out, ctx)


# --------------------------------------------------------------- filters --
def _float_img(img):
    """filters run on float32/float64 (the reference's toFloatArray rule for ints)"""
    if _is_dev(img):
        if img.dtype not in (np.float32, np.float64):
            raise TypeError('device filters need float32/float64 arrays')
        return img
    img = np.asarray(img)
    if img.dtype not in (np.float32, np.float64):
        img = img.astype(np.float32 if img.dtype.itemsize <= 2 else np.float64)
    return np.ascontiguousarray(img)


def conv2d(img, kernel, mode='reflect', cval=0.0, mask=None, mode_y=None, out=None, ctx=None):
    """centred correlation == scipy.ndimage.correlate(img, kernel, mode=mode, cval=cval);
    mode applies to x (columns), mode_y (default: same) to y (rows)"""
    bx = border_id(mode)
    by = border_id(mode_y) if mode_y is not None else bx
    k = np.ascontiguousarray(kernel, dtype=np.float64)
    if k.ndim != 2:
        raise ValueError('kernel must be 2-D')
    kp = _dptr(k)
    img = _float_img(img)
    ctx = _ctx_of(img, mask, ctx=ctx)
    n, h, w = as_frames(img)
    if _is_dev(img):
        if mask is not None:
            if not _is_dev(mask):
                raise TypeError('device image needs a device mask')
            if mask.dtype != np.uint8 or tuple(mask.shape) != (h, w):
                raise ValueError('device mask must be uint8 of shape %s (got %s %s)'
                                 % ((h, w), mask.dtype, mask.shape))
        dst = _dev_out(ctx, out, img.shape, img.dtype)
        ctx._check(ctx._lib.ipa_conv2d_dev(ctx.handle, img.ptr, dtype_id(img.dtype), h, w, w, kp,
                                           k.shape[0], k.shape[1],
                                           mask.ptr if mask is not None else None, w, dst.ptr, w,
                                           n, h * w, h * w, bx, by, float(cval)), 'conv2d')
        return dst
    m = None
    if mask is not None:
        m = np.ascontiguousarray(mask, dtype=np.uint8)
        if m.shape != (h, w):
            raise ValueError('mask shape %s != image shape %s' % (m.shape, (h, w)))
    dst = np.empty_like(img)
    ctx._check(ctx._lib.ipa_conv2d(ctx.handle, _p(img), dtype_id(img.dtype), h, w, kp, k.shape[0],
                                   k.shape[1], _p(m) if m is not None else None, _p(dst), n, bx,
                                   by, float(cval)), 'conv2d')
    return dst


def sepconv2d(img, ky, kx, mode='reflect', cval=0.0, out=None, ctx=None):
    """separable correlation, axis 0 (ky) then axis 1 (kx); None skips an axis"""
    b = border_id(mode)
    ky = np.zeros(0) if ky is None else np.ascontiguousarray(ky, dtype=np.float64).ravel()
    kx = np.zeros(0) if kx is None else np.ascontiguousarray(kx, dtype=np.float64).ravel()
    taps = (_dptr(ky), ky.size, _dptr(kx), kx.size)
    img = _float_img(img)
    ctx = _ctx_of(img, ctx=ctx)
    n, h, w = as_frames(img)
    if _is_dev(img):
        dst = _dev_out(ctx, out, img.shape, img.dtype)
        ctx._check(ctx._lib.ipa_sepconv2d_dev(ctx.handle, img.ptr, dtype_id(img.dtype), h, w, w,
                                              *taps, dst.ptr, w, n, h * w, h * w, b, b,
                                              float(cval)), 'sepconv2d')
        return dst
    dst = np.empty_like(img)
    ctx._check(ctx._lib.ipa_sepconv2d(ctx.handle, _p(img), dtype_id(img.dtype), h, w, *taps,
                                      _p(dst), n, b, b, float(cval)), 'sepconv2d')
    return dst


def gaussian_kernel1d(sigma, radius=None, truncate=4.0):
    """the taps scipy.ndimage.gaussian_filter uses: radius=int(truncate*sigma+0.5)"""
    sigma = float(sigma)
    if radius is None:
        radius = int(truncate * sigma + 0.5)
    x = np.arange(-radius, radius + 1, dtype=np.float64)
    k = np.exp(-0.5 / (sigma * sigma) * x ** 2)
    return k / k.sum()


def gaussian_filter(img, sigma, mode='reflect', cval=0.0, truncate=4.0, out=None, ctx=None):
    """scipy.ndimage.gaussian_filter(img, sigma, mode=..., truncate=...) for 2-D frames"""
    if np.isscalar(sigma):
        sigma = (sigma, sigma)
    ks = [gaussian_kernel1d(s, truncate=truncate) if s > 1e-15 else None for s in sigma]
    return sepconv2d(img, ks[0], ks[1], mode, cval, out=out, ctx=ctx)


_FLOATS = (np.float32, np.float64)


def _nonzero_u8(a):
    return np.ascontiguousarray(np.asarray(a) != 0, dtype=np.uint8)


def extend_array(arr, kernelXY, modex='reflect', modey='reflect', ctx=None):
    """filters/_extendArrayForConvolution.py:5-97 on the device"""
    kx, ky = int(kernelXY[0]), int(kernelXY[1])
    dev, ctx, d_in, h, w = _stage_in('extend_array', arr, ctx, host=_host)
    oshape = (h + 2 * (ky // 2), w + 2 * (kx // 2))
    d_out = DeviceArray(ctx, oshape, d_in.dtype)
    ctx._check(ctx._lib.ipa_extend_array_dev(ctx.handle, d_in.ptr, dtype_id(d_in.dtype), h, w, w,
                                             kx, ky, border_id(modex), border_id(modey), d_out.ptr,
                                             oshape[1]), 'extend_array')
    return _stage_out(dev, d_out)


def conv_ydep(arr, kernels, modex='wrap', modey='reflect', ctx=None):
    """row-dependent k0 x k1 correlation, NaN-skipping
    (filters/varYSizeGaussianFilter.py:53-68); kernels: (H, k0, k1) float64"""
    dev, ctx, d_in, h, w = _stage_in('conv_ydep', arr, ctx, host=_float_img)
    k = np.ascontiguousarray(kernels, dtype=np.float64)
    if k.ndim != 3 or k.shape[0] != h:
        raise ValueError('kernels must be (H, k0, k1)')
    d_k = ctx.to_device(k)
    d_out = DeviceArray(ctx, (h, w), d_in.dtype)
    ctx._check(ctx._lib.ipa_conv_ydep_dev(ctx.handle, d_in.ptr, dtype_id(d_in.dtype), h, w, w,
                                          d_k.ptr, k.shape[1], k.shape[2], border_id(modex),
                                          border_id(modey), d_out.ptr, w), 'conv_ydep')
    if dev:
        d_out._keepalive = d_k  # the table must outlive the asynchronous launch
    return _stage_out(dev, d_out)


def var_y_gauss(arr, sig_min, sig_max, ky, rowk, modex='wrap', modey='reflect', ctx=None):
    """filters/varYSizeGaussianFilter.py:9-68 in one launch pair: per-row Gaussian tables built
    on the device (stdys = linspace(sig_min, sig_max, H)), `rowk` = the kx x-responses"""
    dev, ctx, d_in, h, w = _stage_in('var_y_gauss', arr, ctx, host=_float_img)
    rk = np.ascontiguousarray(rowk, dtype=np.float64).ravel()
    d_out = DeviceArray(ctx, (h, w), d_in.dtype)
    ctx._check(ctx._lib.ipa_var_y_gauss_dev(
        ctx.handle, d_in.ptr, dtype_id(d_in.dtype), h, w, w, float(sig_min), float(sig_max),
        int(ky), _dptr(rk), rk.size, border_id(modex), border_id(modey), d_out.ptr, w),
        'var_y_gauss')
    return _stage_out(dev, d_out)


def local_std(img, blurred, ksize, ctx=None):
    """filters/standardDeviation.py:34-70 (_calc) for ksize=(kx, ky)"""
    dev, ctx, d_img, h, w = _stage_in('local_std', img, ctx, host=_float_img, others=(blurred,))
    d_bl = blurred if _is_dev(blurred) else ctx.to_device(
        np.ascontiguousarray(blurred, dtype=d_img.dtype))
    if d_bl.shape != d_img.shape or d_bl.dtype != d_img.dtype:
        raise ValueError('img and blurred must be 2-D arrays of equal shape and dtype')
    d_out = DeviceArray(ctx, (h, w), d_img.dtype)
    ctx._check(ctx._lib.ipa_local_std_dev(ctx.handle, d_img.ptr, d_bl.ptr, dtype_id(d_img.dtype),
                                          h, w, w, w, int(ksize[0]), int(ksize[1]), d_out.ptr, w),
               'local_std')
    return _stage_out(dev, d_out)


def _float_ndarray(a):
    if not (isinstance(a, np.ndarray) and a.dtype in _FLOATS):
        raise TypeError('masked_mean needs a float32/float64 ndarray')
    return np.ascontiguousarray(a)


def masked_mean(arr, mask, ksize, fill_mask=True, ctx=None, fn='median'):
    """filters/maskedFilter.py:12-102 (_calcMean / _calcMedian by ``fn``; default and every value
    other than 'mean': median, as in the reference).  fill_mask=True fills ``arr`` IN PLACE (host
    arrays are copied back into ``arr``); fill_mask=False returns a new NaN-padded array."""
    fn = 'mean' if fn == 'mean' else 'median'
    if _is_dev(arr) and not _is_dev(mask):
        raise TypeError('device array needs a device mask')
    dev, ctx, d_arr, h, w = _stage_in('masked_mean', arr, ctx, _FLOATS, _float_ndarray, (mask,))
    d_mask = mask if dev else ctx.to_device(np.ascontiguousarray(mask, dtype=np.uint8))
    if tuple(d_mask.shape) != tuple(d_arr.shape) or d_mask.dtype != np.uint8:
        raise ValueError('arr and mask must be 2-D arrays of equal shape (mask uint8/bool)')
    d_out = d_arr if fill_mask else DeviceArray(ctx, (h, w), d_arr.dtype)
    f = ctx._lib.ipa_masked_mean_dev if fn == 'mean' else ctx._lib.ipa_masked_median_dev
    ctx._check(f(ctx.handle, d_arr.ptr, dtype_id(d_arr.dtype), d_mask.ptr, h, w, w, w, int(ksize),
                 int(bool(fill_mask)), d_out.ptr, w), 'masked_' + fn)
    if fill_mask and not dev:
        arr[...] = d_out.get()
        return arr
    return _stage_out(dev, d_out)


def nan_max(arr, ksize, ctx=None):
    """filters/nan_maximum_filter.py:17-37"""
    dev, ctx, d_arr, h, w = _stage_in('nan_max', arr, ctx, _FLOATS, _float_img, bad_shape=TypeError)
    d_out = DeviceArray(ctx, (h, w), d_arr.dtype)
    ctx._check(ctx._lib.ipa_nan_max_dev(ctx.handle, d_arr.ptr, dtype_id(d_arr.dtype), h, w, w,
                                        int(ksize), d_out.ptr, w), 'nan_max')
    return _stage_out(dev, d_out)


def closest_distance(arr, ksize=30, dtype=np.uint16, ctx=None):
    """render/closestDirectDistance.py:17-41: distance to the closest non-zero pixel (device
    input: uint8, non-zero = set)"""
    dtype = np.dtype(dtype)
    if dtype not in (np.uint16, np.float64):
        raise NotImplementedError('closest_distance writes uint16 or float64')
    dev, ctx, d_arr, h, w = _stage_in('closest_distance', arr, ctx, (np.uint8,), _nonzero_u8)
    d_out = DeviceArray(ctx, (h, w), dtype)
    ctx._check(ctx._lib.ipa_closest_distance_dev(ctx.handle, d_arr.ptr, h, w, w, int(ksize),
                                                 d_out.ptr, dtype_id(dtype), w), 'closest_distance')
    return _stage_out(dev, d_out)


def pos_intensity_unc(image, sx, sy, ksize, ctx=None):
    """uncertainty/positionToIntensityUncertainty.py:7-49; ksize = half window.  sx / sy are
    both scalars or both (H, W) maps; returns float64"""
    maps = isinstance(sx, (np.ndarray, DeviceArray))
    dev, ctx, d_img, h, w = _stage_in('pos_intensity_unc', image, ctx, _FLOATS, _float_img,
                                      (sx, sy), bad_shape=TypeError)
    d_sx = d_sy = None
    if maps:
        d_sx = sx if _is_dev(sx) else ctx.to_device(np.ascontiguousarray(sx, dtype=np.float64))
        d_sy = sy if _is_dev(sy) else ctx.to_device(np.ascontiguousarray(sy, dtype=np.float64))
        if tuple(d_sx.shape) != (h, w) or tuple(d_sy.shape) != (h, w) or \
                d_sx.dtype != np.float64 or d_sy.dtype != np.float64:
            raise ValueError('sigma maps must be float64 arrays of the image shape')
    d_out = DeviceArray(ctx, (h, w), np.float64)
    ctx._check(ctx._lib.ipa_pos_intensity_unc_dev(
        ctx.handle, d_img.ptr, dtype_id(d_img.dtype), h, w, w,
        d_sx.ptr if maps else None, d_sy.ptr if maps else None, w,
        0.0 if maps else float(sx), 0.0 if maps else float(sy), int(ksize), d_out.ptr, w),
        'pos_intensity_unc')
    return _stage_out(dev, d_out)


def median_threshold(img, threshold=0.1, condition='>', want_indices=True, ctx=None, size=3):
    """filters/medianThreshold.py:7-30: -> (out, indices) new arrays"""
    if condition not in ('>', '<'):
        raise ValueError("condition must be '>' or '<'")
    dev, ctx, d_img, h, w = _stage_in('median_threshold', img, ctx, _FLOATS, _float_img,
                                      bad_shape=TypeError)
    d_out = DeviceArray(ctx, (h, w), d_img.dtype)
    d_idx = DeviceArray(ctx, (h, w), np.uint8) if want_indices else None
    size = int(size)
    if size < 1:
        raise ValueError('size must be >= 1')
    ctx._check(ctx._lib.ipa_median_threshold_size_dev(
        ctx.handle, d_img.ptr, dtype_id(d_img.dtype), h, w, w, size, float(threshold),
        int(condition == '<'), d_out.ptr, w, d_idx.ptr if want_indices else None, w),
        'median_threshold')
    if dev:
        return d_out, d_idx
    return d_out.get(), (d_idx.get().astype(bool) if want_indices else None)


def calib_prefilter(img, bg=None, ff=None, threshold=0.1, out=None, ctx=None):
    """stages 2-4 of CameraCalibration.correct (camera/CameraCalibration.py:416-437) in one
    kernel: dark current, flat field, nan_to_num + thresholded 3x3 median.  bg / ff are cast to
    the image dtype; returns a new array (DeviceArray for device input)."""
    dev, ctx, d_img, h, w = _stage_in('calib_prefilter', img, ctx, _FLOATS, _float_img, (bg, ff),
                                      bad_shape=TypeError)

    def side(a, name):
        if a is None:
            return None
        if _is_dev(a):
            if a.dtype != d_img.dtype or tuple(a.shape) != (h, w):
                raise ValueError('%s must match the image shape and dtype' % name)
            return a
        a = np.asarray(a)
        if a.shape != (h, w):
            a = np.broadcast_to(a, (h, w))
        return ctx.to_device(np.ascontiguousarray(a, dtype=d_img.dtype))

    d_bg, d_ff = side(bg, 'bg'), side(ff, 'ff')
    d_out = _dev_out(ctx, out, (h, w), d_img.dtype) if dev else DeviceArray(ctx, (h, w), d_img.dtype)
    ctx._check(ctx._lib.ipa_calib_prefilter_dev(
        ctx.handle, d_img.ptr, dtype_id(d_img.dtype), d_bg.ptr if d_bg is not None else None,
        d_ff.ptr if d_ff is not None else None, h, w, w, w, w, float(threshold), d_out.ptr, w),
        'calib_prefilter')
    return _stage_out(dev, d_out)


# ------------------------------------------------- single-time effects --
STE_DTYPES = PIXEL_DTYPES


def _ste_state(a, shape, dtype, name):
    if not _is_dev(a) or tuple(a.shape) != shape or a.dtype != dtype:
        raise ValueError('%s must be a %s DeviceArray of shape %s' % (name, np.dtype(dtype), shape))
    return a


def ste_update(frames, avg, count, thr, first_pair=False, nlf=None, nstd=4, mask=None,
               mask_ste=None, mask_clean=None, ctx=None):
    """single-time-effect removal over a stack (features/SingleTimeEffectDetection.py:23-75):
    steps the running mean through `frames` and leaves the state in place.

    frames: (n, h, w) or (h, w), host or DeviceArray, uint8 / uint16 / float32 / float64 (other
    host types go to float64).  avg (float64), count (int32) and thr (float64) are (h, w)
    DeviceArrays: the state, updated in place.  first_pair: start from frames 0 and 1 (avg =
    min, count = 1, thr = nlf(avg) * nstd, then max(f0, f1), f2, ...); otherwise continue from the
    state.  nlf: (minY, ax, ay) of NoiseLevelFunction.boundedFunction, evaluated on the device,
    or None: thr already holds the threshold.  mask: the caller's clean mask for every frame
    (host bool or device uint8).  mask_ste (OR-accumulated) and mask_clean (the last frame's)
    are (h, w) uint8 DeviceArrays or None.  Up to 8 frames per launch (ipa_ste_dev)."""
    ctx = _ctx_of(frames, avg, count, thr, mask, mask_ste, mask_clean, ctx=ctx)
    if _is_dev(frames):
        d = frames
        if d.dtype not in STE_DTYPES:
            raise TypeError('ste_update: device frames must be uint8/uint16/float32/float64')
    else:
        d = ctx.to_device(_px_host(frames))
    n, h, w = as_frames(d)
    shape = (h, w)
    _ste_state(avg, shape, np.float64, 'avg')
    _ste_state(count, shape, np.int32, 'count')
    _ste_state(thr, shape, np.float64, 'thr')
    for a, name in ((mask_ste, 'mask_ste'), (mask_clean, 'mask_clean')):
        if a is not None:
            _ste_state(a, shape, np.uint8, name)
    if mask is not None:
        if _is_dev(mask):
            _ste_state(mask, shape, np.uint8, 'mask')
        else:
            m = np.broadcast_to(np.asarray(mask, dtype=bool), shape)
            mask = ctx.to_device(np.ascontiguousarray(m, dtype=np.uint8))
    cnlf = None
    if nlf is not None:
        cnlf = L.dbl(nlf, 3)
    ctx._check(ctx._lib.ipa_ste_dev(
        ctx.handle, d.ptr, dtype_id(d.dtype), n, h, w, w, h * w, 1 if first_pair else 0,
        cnlf, float(nstd), avg.ptr, count.ptr, thr.ptr, w,
        mask.ptr if mask is not None else None,
        mask_ste.ptr if mask_ste is not None else None,
        mask_clean.ptr if mask_clean is not None else None, w), 'ste_update')


def remove_single_pixels(arr, out=None, ctx=None):
    """filters/removeSinglePixels.py:4-30, not in place: a set pixel stays set only when one of
    its <= 8 in-image neighbours is set.  Host input (any dtype, non-zero = set) gives a bool
    array, a (h, w) uint8 DeviceArray gives a uint8 DeviceArray."""
    dev, ctx, d, h, w = _stage_in('remove_single_pixels', arr, ctx, (np.uint8,), _nonzero_u8,
                                  (out,), bad_shape=TypeError)
    d_out = _dev_out(ctx, out, (h, w), np.uint8) if dev else DeviceArray(ctx, (h, w), np.uint8)
    ctx._check(ctx._lib.ipa_remove_single_pixels_dev(ctx.handle, d.ptr, h, w, w, d_out.ptr, w),
               'remove_single_pixels')
    return d_out if dev else d_out.get().astype(bool)


# ------------------------------------------------------------ denoising --
def _nlm_args(patch_size, patch_distance, h, sigma):
    patch_size, patch_distance = int(patch_size), int(patch_distance)
    h, sigma = float(h), float(sigma)
    if not 2 <= patch_size <= 11:
        raise ValueError('nl_means: patch_size must be in 2 ... 11 (got %d)' % patch_size)
    if patch_distance < 0:
        raise ValueError('nl_means: patch_distance must not be negative (got %d)' % patch_distance)
    if not h > 0 or not sigma >= 0:
        raise ValueError('nl_means: h must be positive and sigma not negative')
    return patch_size, patch_distance, h, sigma


def nl_means(img, patch_size=7, patch_distance=11, h=0.1, sigma=0.0, out=None, ctx=None):
    """non-local-means denoising, skimage.restoration.denoise_nl_means(img, patch_size,
    patch_distance, h, fast_mode=True, sigma=sigma) of scikit-image 0.18 with the exact
    exponential (ipa_nl_means_dev; camera/CameraCalibration.py:461-474).

    img: (h, w) or (n, h, w) batch of independent frames, host or DeviceArray, float32 (computed
    in float32) or float64 (in double); integer images raise TypeError.  An even patch_size is
    the next odd one.  patch_size <= 11; patch_distance as far as the LDS tile holds it (30 / 20
    for float32 / float64 at patch_size 7).  Not in place: `out` (device input only) must not be
    the source.  Returns a new array, a DeviceArray for device input."""
    patch_size, patch_distance, h, sigma = _nlm_args(patch_size, patch_distance, h, sigma)
    dev = _is_dev(img)
    if not dev:
        img = np.asarray(img)
    if np.dtype(img.dtype) not in (np.float32, np.float64):
        raise TypeError('nl_means needs float32 / float64 frames (got %s)' % np.dtype(img.dtype))
    if len(img.shape) not in (2, 3) or min(img.shape[-2:]) < 2 or img.shape[0] < 1:
        raise ValueError('nl_means takes a (h, w) image or (n, h, w) batch with h, w >= 2, got shape %s'
                         % (tuple(img.shape),))
    if out is not None and (not dev or out is img):
        raise ValueError('nl_means: out must be a DeviceArray other than the (device) source')
    dev, ctx, d, hh, ww = _stage_in('nl_means', img, ctx, _FLOATS, np.ascontiguousarray, (out,),
                                    ndims=(2, 3))
    n = as_frames(d)[0]
    d_out = _dev_out(ctx, out, d.shape, d.dtype)
    ctx._check(ctx._lib.ipa_nl_means_dev(
        ctx.handle, d.ptr, dtype_id(d.dtype), n, hh, ww, ww, hh * ww, patch_size, patch_distance, h,
        sigma, d_out.ptr, ww, hh * ww), 'nl_means')
    return _stage_out(dev, d_out)


def nan_to_zero(img):
    """img[isnan(img)] = 0 in place on a float32 / float64 DeviceArray, (h, w) or (n, h, w)
    (ipa_nan_to_zero_dev; camera/CameraCalibration.py:467).  Returns img."""
    _, ctx, _, hh, ww = _stage_in('nan_to_zero', img, None, _FLOATS, ndims=(2, 3))
    ctx._check(ctx._lib.ipa_nan_to_zero_dev(ctx.handle, img.ptr, dtype_id(img.dtype),
                                            as_frames(img)[0], hh, ww, ww, hh * ww), 'nan_to_zero')
    return img


# ------------------------------------------------- fused remap -> filter --
def remap_conv2d(src, mapx, mapy, kernel, interpolation='linear', border_mode='constant',
                 border_value=0.0, conv_mode='reflect', out=None, ctx=None):
    """remap followed by a K x K centred correlation, one kernel, device arrays only"""
    ctx = _dev_only('remap_conv2d', ctx, src, mapx, mapy)
    _check_dev_maps(mapx, mapy)
    return _geometry('remap_conv2d', src, (mapx.ptr, mapy.ptr, mapx.shape[1]), mapx.shape,
                     interpolation, border_mode, border_value, None, out, ctx,
                     _dense_filt(kernel, conv_mode))


def undistort_conv2d(src, K, dist5, newK, kernel, interpolation='linear', border_mode='constant',
                     border_value=0.0, conv_mode='reflect', out_shape=None, out=None, ctx=None):
    ctx = _dev_only('undistort_conv2d', ctx, src)
    return _geometry('undistort_conv2d', src, _lens(K, dist5, K if newK is None else newK),
                     out_shape, interpolation, border_mode, border_value, None, out, ctx,
                     _dense_filt(kernel, conv_mode))


def warp_perspective_conv2d(src, M_dst2src, out_shape, kernel, interpolation='linear',
                            border_mode='constant', border_value=0.0, conv_mode='reflect',
                            out=None, ctx=None):
    ctx = _dev_only('warp_perspective_conv2d', ctx, src)
    return _geometry('warp_perspective_conv2d', src, (_mat3(M_dst2src),),
                     (int(out_shape[0]), int(out_shape[1])), interpolation, border_mode,
                     border_value, None, out, ctx, _dense_filt(kernel, conv_mode))


def remap_sepconv2d(src, mapx, mapy, ky, kx, interpolation='linear', border_mode='constant',
                    border_value=0.0, conv_mode='reflect', out=None, ctx=None):
    """remap followed by a separable correlation (axis 0 with ky, then axis 1 with kx; the
    scipy.ndimage.gaussian_filter order) — one kernel where built, device arrays only"""
    ctx = _dev_only('remap_sepconv2d', ctx, src, mapx, mapy)
    _check_dev_maps(mapx, mapy)
    return _geometry('remap_sepconv2d', src, (mapx.ptr, mapy.ptr, mapx.shape[1]), mapx.shape,
                     interpolation, border_mode, border_value, None, out, ctx,
                     _sep_filt(ky, kx, conv_mode))


def undistort_sepconv2d(src, K, dist5, newK, ky, kx, interpolation='linear',
                        border_mode='constant', border_value=0.0, conv_mode='reflect',
                        out_shape=None, out=None, ctx=None):
    ctx = _dev_only('undistort_sepconv2d', ctx, src)
    return _geometry('undistort_sepconv2d', src, _lens(K, dist5, K if newK is None else newK),
                     out_shape, interpolation, border_mode, border_value, None, out, ctx,
                     _sep_filt(ky, kx, conv_mode))


def warp_perspective_sepconv2d(src, M_dst2src, out_shape, ky, kx, interpolation='linear',
                               border_mode='constant', border_value=0.0, conv_mode='reflect',
                               out=None, ctx=None):
    ctx = _dev_only('warp_perspective_sepconv2d', ctx, src)
    return _geometry('warp_perspective_sepconv2d', src, (_mat3(M_dst2src),),
                     (int(out_shape[0]), int(out_shape[1])), interpolation, border_mode,
                     border_value, None, out, ctx, _sep_filt(ky, kx, conv_mode))


# ------------------------------------------------------------------- IDW --
def _fill(name, grid, mask, args, ctx, masked=True, any_dtype=False, mask_written=False):
    """The in-place fills: ipa_<name>_dev on a DeviceArray grid, the host-pointer ipa_<name> on
    an ndarray, either with (grid, dtype[, mask], h, w[, pitch]) and then the fill's own `args`.
    `masked` False: the fill takes no mask.  The library reads h * w mask bytes, so a mask of any other
    shape is refused here (ValueError), on the host and on the device.  A host grid is written
    where it lies and must be a C-contiguous 2-D ndarray, float32 / float64 unless `any_dtype`;
    `mask_written`: so is the mask, bool / uint8."""
    ctx = _ctx_of(grid, mask, ctx=ctx)
    if _is_dev(grid):
        if grid.ndim != 2:
            raise ValueError('grid must be 2-D')
        m = ()
        if masked:
            if not _is_dev(mask):
                raise TypeError('device grid needs a device mask')
            if mask.dtype != np.uint8 or tuple(mask.shape) != tuple(grid.shape):
                raise ValueError('device mask must be uint8 of shape %s (got %s %s)'
                                 % (grid.shape, mask.dtype, mask.shape))
            m = (mask.ptr,)
        h, w = grid.shape
        status = getattr(ctx._lib, 'ipa_%s_dev' % name)(
            ctx.handle, grid.ptr, dtype_id(grid.dtype), *m, h, w, w, *args)
    else:
        if not (isinstance(grid, np.ndarray) and grid.flags.c_contiguous and grid.ndim == 2):
            raise ValueError('grid must be a C-contiguous 2-D ndarray (it is modified in place)')
        if not any_dtype and grid.dtype not in _FLOATS:
            raise TypeError('grid must be float32 or float64')
        m = ()
        if mask_written:
            if not (isinstance(mask, np.ndarray) and mask.flags.c_contiguous and
                    mask.shape == grid.shape and mask.dtype in (np.bool_, np.uint8)):
                raise ValueError('mask must be a C-contiguous bool / uint8 array of the grid\'s shape '
                                 '(it is modified in place)')
            m = (_p(mask.view(np.uint8)),)
        elif masked:
            mask = np.ascontiguousarray(mask, dtype=np.uint8)
            if mask.shape != grid.shape:
                raise ValueError('mask and grid differ in shape')
            m = (_p(mask),)
        h, w = grid.shape
        status = getattr(ctx._lib, 'ipa_%s' % name)(
            ctx.handle, _p(grid), dtype_id(grid.dtype), *m, h, w, *args)
    ctx._check(status, name)
    return grid


def idw_fill(grid, mask, ksize, weights, ctx=None):
    """in-place IDW hole filling (interpolate2dStructuredIDW._calc)"""
    w = np.ascontiguousarray(weights, dtype=np.float64)
    if w.shape != (2 * ksize + 1, 2 * ksize + 1):
        raise ValueError('weights must be (2*ksize+1)^2')
    return _fill('idw_fill', grid, mask, (int(ksize), _dptr(w)), ctx, any_dtype=True)


def fast_idw_fill(grid, mask, offsets, weights, minnvals, ctx=None):
    """in-place growing-distance IDW (interpolate2dStructuredFastIDW._calc)"""
    offs = np.ascontiguousarray(offsets, dtype=np.int32)
    w = np.ascontiguousarray(weights, dtype=np.float64)
    n = int(w.size)
    if offs.shape != (n, 2):
        raise ValueError('offsets must be (n,2) matching weights')
    return _fill('fast_idw_fill', grid, mask, (_p(offs), _dptr(w), n, int(minnvals)),
                 ctx, any_dtype=True)


def unstructured_idw(x, y, v, grid, power=2, ctx=None):
    """every pixel of `grid` from n scattered points (interpolate2dUnstructuredIDW), in place"""
    xs, ys, vs = (np.ascontiguousarray(np.ravel(a), dtype=np.float64) for a in (x, y, v))
    if not (xs.size == ys.size == vs.size and vs.size >= 1):
        raise ValueError('x, y, v must be 1-D, of equal length >= 1')
    return _fill('unstructured_idw', grid, None,
                 (_dptr(xs), _dptr(ys), _dptr(vs), int(vs.size), float(power)), ctx, masked=False)


def circular_idw_fill(grid, mask, ksize, power=2, fr=1, fphi=1, cx=0, cy=0, ctx=None):
    """in-place IDW hole filling with polar distances (interpolateCircular2dStructuredIDW)"""
    return _fill('circular_idw_fill', grid, mask,
                 (int(ksize), float(power), float(fr), float(fphi), float(cx), float(cy)), ctx)


def cross_avg_fill(grid, mask, ksize, power=2, ctx=None):
    """in-place fill of large holes from the four axis directions
    (interpolate2dStructuredCrossAvg)"""
    return _fill('cross_avg_fill', grid, mask, (int(ksize), float(power)), ctx)


def point_spread_idw(grid, mask, ksize, power=2, max_iter=1e5, ctx=None):
    """in-place point-spread IDW fill (interpolate2dStructuredPointSpreadIDW): grid AND mask are
    modified - filled pixels are unmasked"""
    return _fill('point_spread_idw', grid, mask,
                 (int(ksize), float(power), int(min(max_iter, 2 ** 62))), ctx, mask_written=True)


# ------------------------------------------------------- fastFilter / fastMean --
RESIZE_INTERP = {'linear': L.RESIZE_LINEAR, 'cubic': L.RESIZE_CUBIC, 'area': L.RESIZE_AREA,
                 'lanczos4': L.RESIZE_LANCZOS4}
RESIZE_INTERP.update({v: v for v in list(RESIZE_INTERP.values())})   # cv2's INTER_* numbers as they are
FAST_FILTER_FN = {'median': L.STAT_MEDIAN, 'nanmedian': L.STAT_NANMEDIAN, 'mean': L.STAT_MEAN,
                  'nanmean': L.STAT_NANMEAN}


def resize(img, dsize_hw, interpolation='linear', out=None, ctx=None, src_shape=None):
    """cv2.resize(img, (w, h), interpolation=...) for 2-D float32 / float64 images;
    dsize_hw = (rows, columns) of the result.  ``src_shape`` (device arrays): resize only the
    top-left (rows, columns) of ``img`` - fastFilter's cropped grid, without a copy"""
    if interpolation not in RESIZE_INTERP:
        raise ValueError('resize: interpolation %r is not built (linear / 1, cubic / 2, area / 3, '
                         'lanczos4 / 4; cv2.INTER_NEAREST = 0 and the exact variants are not)'
                         % (interpolation,))
    interp = RESIZE_INTERP[interpolation]
    dh, dw = int(dsize_hw[0]), int(dsize_hw[1])
    if _is_dev(img):
        ctx = _ctx_of(img, ctx=ctx)
        if img.ndim != 2:
            raise ValueError('resize takes one 2-D image')
        sh, sw = img.shape
        pitch = sw
        if src_shape is not None:
            if not (0 < int(src_shape[0]) <= sh and 0 < int(src_shape[1]) <= sw):
                raise ValueError('src_shape %r outside the %r array' % (tuple(src_shape), img.shape))
            sh, sw = int(src_shape[0]), int(src_shape[1])
        dst = _dev_out(ctx, out, (dh, dw), img.dtype)
        ctx._check(ctx._lib.ipa_resize_dev(ctx.handle, img.ptr, dtype_id(img.dtype), sh, sw, pitch,
                                           dst.ptr, dh, dw, dw, interp), 'resize')
        return dst
    if src_shape is not None:
        img = np.asarray(img)[:int(src_shape[0]), :int(src_shape[1])]
    ctx = ctx or default_context()
    img = _float_img(img)
    if img.ndim != 2:
        raise ValueError('resize takes one 2-D image')
    sh, sw = img.shape
    dst = np.empty((dh, dw), img.dtype)
    ctx._check(ctx._lib.ipa_resize(ctx.handle, _p(img), dtype_id(img.dtype), sh, sw, _p(dst), dh,
                                   dw, interp), 'resize')
    return dst


def fast_filter_stat(arr, ksize, every, fn='median', ctx=None):
    """the strided window statistics of fastFilter (filters/fastFilter.py:52-122): float64 array of
    ceil(h / every) x ceil(w / every) cells"""
    f = FAST_FILTER_FN[fn]
    every, ksize = int(every), int(ksize)
    if _is_dev(arr):
        ctx = _ctx_of(arr, ctx=ctx)
        h, w = arr.shape
        out = ctx.empty((-(-h // every), -(-w // every)), np.float64)
        ctx._check(ctx._lib.ipa_fast_filter_stat_dev(ctx.handle, arr.ptr, dtype_id(arr.dtype), h, w,
                                                     w, ksize, every, f, out.ptr),
                   'fast_filter_stat')
        return out
    ctx = ctx or default_context()
    arr = _float_img(arr)
    if arr.ndim != 2:
        raise ValueError('fast_filter_stat takes one 2-D array')
    h, w = arr.shape
    out = np.empty((-(-h // every), -(-w // every)), np.float64)
    ctx._check(ctx._lib.ipa_fast_filter_stat(ctx.handle, _p(arr), dtype_id(arr.dtype), h, w, ksize,
                                             every, f, _p(out)), 'fast_filter_stat')
    return out
