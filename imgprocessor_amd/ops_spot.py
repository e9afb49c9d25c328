"""The spot family of ``ops`` (csrc/spot.hip), re-exported there as ``ops.histogram``,
``ops.otsu_threshold``, ``ops.spot_mask``, ``ops.label``, ``ops.largest_component`` and
``ops.spot_take``: what camera/flatField/vignettingFromSpotAverage.py needs of numpy, skimage and
scipy.  Like every family it goes through ``_stage_in`` / ``_stage_out``: host arrays in give host
arrays out, DeviceArrays stay on the device; counts, thresholds and the scalars of a component are
host values.
"""
import ctypes as C

import numpy as np

from . import _lib as L
from .device import DeviceArray, dtype_id
from ._staging import PIXEL_DTYPES, _bg, _ctx_of, _is_dev, _px_host, _stage_in, _stage_out

MAX_BINS = 2048   # kSpotMaxBins of csrc/spot.hip


def _bins(name, nbins):
    """the refusals of a bin count, before anything touches a device"""
    n = int(nbins)
    if n != nbins or n < 1:
        raise ValueError('%s: `bins` must be a positive integer (got %r)' % (name, nbins))
    if n > MAX_BINS:
        raise NotImplementedError('%s: at most %d bins (got %d)' % (name, MAX_BINS, n))
    return n


def _src(name, img, bg, ctx, others=()):
    """the frame and its background on the device -> (dev, ctx, the frame - held until after the
    launch -, the background frame or None, the arguments every entry point starts with)"""
    dev, ctx, d, h, w = _stage_in(name, img, ctx, PIXEL_DTYPES, _px_host, (bg,) + tuple(others))
    d_bg, bgp, bg_pitch, bgv = _bg(name, bg, (h, w), ctx)
    return dev, ctx, d, d_bg, (ctx.handle, d.ptr, dtype_id(d.dtype), h, w, w, bgp, bg_pitch, bgv)


def _range(name, ctx, args):
    r = (C.c_double * 5)()
    ctx._check(ctx._lib.ipa_spot_range_dev(*(args + (r,))), name)
    return tuple(r)


def _histogram(name, ctx, args, rng, nbins):
    """np.histogram(frame - bg, nbins) given the frame's range -> (counts, edges)"""
    lo, hi, n_nan, n_inf = rng[:4]
    if n_nan or n_inf:
        raise ValueError('%s: autodetected range of [%s, %s] is not finite'
                         % (name, 'nan' if n_nan else lo, 'nan' if n_nan else hi))
    if lo == hi:   # numpy's range of a constant array
        lo, hi = lo - 0.5, hi + 0.5
    edges = np.linspace(lo, hi, nbins + 1, endpoint=True, dtype=np.float64)
    counts = np.zeros(nbins, np.uint64)
    ctx._check(ctx._lib.ipa_spot_histogram_dev(*(args + (
        edges.ctypes.data_as(L._dp), nbins, counts.ctypes.data_as(C.c_void_p)))), name)
    return counts.astype(np.int64), edges


def histogram(img, nbins=256, bg=None, ctx=None):
    """np.histogram((img - bg).ravel(), nbins) -> (counts int64, edges float64), the counts formed
    on the device by numpy's bin rule (vignettingFromSpotAverage.py:56 under skimage's
    threshold_otsu; ipa_spot_range_dev, ipa_spot_histogram_dev).  img: uint8 / uint16 / float32 /
    float64; bg: None, a scalar or a float64 (h, w) frame.  1 <= nbins <= 2048 (ValueError below,
    NotImplementedError above); a NaN or an infinity raises ValueError as numpy does."""
    nbins = _bins('histogram', nbins)
    _, ctx, d, d_bg, args = _src('histogram', img, bg, ctx)
    return _histogram('histogram', ctx, args, _range('histogram', ctx, args), nbins)


def otsu_threshold(img, bg=None, nbins=256, ctx=None):
    """skimage.filters.threshold_otsu(img - bg, nbins) (0.18) as a float
    (vignettingFromSpotAverage.py:56): a frame whose pixels all equal the first one returns that
    value; otherwise the histogram comes from the device and the formula over its nbins numbers is
    numpy on the host, written as skimage writes it."""
    nbins = _bins('otsu_threshold', nbins)
    _, ctx, d, d_bg, args = _src('otsu_threshold', img, bg, ctx)
    rng = _range('otsu_threshold', ctx, args)
    if rng[2] == 0 and rng[0] == rng[1]:   # np.all(image == first_pixel)
        return rng[4]
    counts, edges = _histogram('otsu_threshold', ctx, args, rng, nbins)
    counts = counts.astype(float)
    bin_centers = (edges[:-1] + edges[1:]) / 2.
    with np.errstate(divide='ignore', invalid='ignore'):
        # class probabilities for all possible thresholds
        weight1 = np.cumsum(counts)
        weight2 = np.cumsum(counts[::-1])[::-1]
        # class means for all possible thresholds
        mean1 = np.cumsum(counts * bin_centers) / weight1
        mean2 = (np.cumsum((counts * bin_centers)[::-1]) / weight2[::-1])[::-1]
        variance12 = weight1[:-1] * weight2[1:] * (mean1[:-1] - mean2[1:]) ** 2
    return float(bin_centers[np.argmax(variance12)])


def spot_mask(img, t, bg=None, out=None, ctx=None):
    """uint8 ``minimum_filter(img - bg > t, 3)``: the threshold mask, eroded by 3 x 3 with positions
    beyond the frame left out (vignettingFromSpotAverage.py:61; ipa_spot_mask_dev)"""
    dev, ctx, d, d_bg, args = _src('spot_mask', img, bg, ctx, (out,))
    h, w = d.shape
    if out is not None and (not dev or not _is_dev(out) or out.shape != (h, w) or out.dtype != np.uint8):
        raise ValueError('spot_mask: out must be a uint8 DeviceArray of shape %s for a device frame' % ((h, w),))
    d_out = out if out is not None else DeviceArray(ctx, (h, w), np.uint8)
    ctx._check(ctx._lib.ipa_spot_mask_dev(*(args + (float(t), d_out.ptr, w))), 'spot_mask')
    return _stage_out(dev, d_out)


def _mask_host(m):
    m = np.asarray(m)
    return np.ascontiguousarray(m.view(np.uint8) if m.dtype == np.bool_ else
                                m if m.dtype == np.uint8 else (m != 0).astype(np.uint8))


def _connectivity(name, connectivity):
    if connectivity not in (1, 2):
        raise ValueError('%s: connectivity is 1 (4 neighbours) or 2 (8 neighbours) on 2-D images (got %r)'
                         % (name, connectivity))
    return int(connectivity)


def _sizes(ctx, d_labels, n):
    h, w = d_labels.shape
    if n == 0:
        return np.zeros(0, np.int64)
    d_sizes = DeviceArray._wrap(ctx, ctx._alloc(n * 8), (n,), np.int64, True)
    ctx._check(ctx._lib.ipa_label_sizes_dev(ctx.handle, d_labels.ptr, h, w, w, n, d_sizes.ptr), 'label')
    return d_sizes.get()


def _label(ctx, d_mask, connectivity):
    h, w = d_mask.shape
    d_labels = DeviceArray.counts(ctx, (h, w))
    n = C.c_int()
    ctx._check(ctx._lib.ipa_label_dev(ctx.handle, d_mask.ptr, h, w, w, connectivity, d_labels.ptr, w, C.byref(n)),
               'label')
    return d_labels, n.value


def label(mask, connectivity=2, return_sizes=False, ctx=None):
    """``skimage.measure.label(mask, background=0, return_num=True, connectivity=connectivity)``
    -> (labels int32, n[, sizes]): the connected components of the non-zero pixels of a uint8 /
    bool mask, numbered 1 .. n in the raster order of their first pixels, 0 elsewhere
    (vignettingFromSpotAverage.py:61; ipa_label_dev).  connectivity 2 is skimage's default on
    images (8 neighbours), 1 is scipy.ndimage.label's (4 neighbours).  return_sizes appends the n
    pixel counts, a host int64 array (ipa_label_sizes_dev)."""
    connectivity = _connectivity('label', connectivity)
    dev, ctx, d, h, w = _stage_in('label', mask, ctx, (np.uint8,), _mask_host)
    d_labels, n = _label(ctx, d, connectivity)
    out = (_stage_out(dev, d_labels), n)
    return out + (_sizes(ctx, d_labels, n),) if return_sizes else out


def _labels_dev(name, labels, shape, ctx):
    """an int32 label image on the device; a host one goes up through DeviceArray.counts"""
    d = labels
    if not _is_dev(labels):
        host = np.ascontiguousarray(labels, dtype=np.int32)
        d = DeviceArray.counts(ctx, host.shape)
        d.set(host)
    if d.dtype != np.int32 or d.ndim != 2 or (shape is not None and tuple(d.shape) != tuple(shape)):
        raise ValueError('%s: labels must be a 2-D int32 array%s (got %s %s)'
                         % (name, '' if shape is None else ' of shape %s' % (tuple(shape),), d.dtype, tuple(d.shape)))
    return d


def largest_component(labels_or_mask, n=None, connectivity=2, ctx=None):
    """(label, size, (sum_y, sum_x)) of the largest component - the lowest label among equals, as
    np.argmax of the sizes - or None where there is no component (vignettingFromSpotAverage.py:63-66;
    ipa_label_largest_dev).  The coordinate sums are exact integers: sum / size is
    scipy.ndimage.center_of_mass to the bit.  int32 input is a label image and needs its count n; a
    uint8 / bool mask is labelled first."""
    a = labels_or_mask
    if (a.dtype if _is_dev(a) else np.asarray(a).dtype) == np.int32:
        if n is None:
            raise ValueError('largest_component: a label image needs its count n')
        ctx = _ctx_of(a, ctx=ctx)
        d = _labels_dev('largest_component', a, None, ctx)
    else:
        connectivity = _connectivity('largest_component', connectivity)
        _, ctx, d_mask, _, _ = _stage_in('largest_component', a, ctx, (np.uint8,), _mask_host)
        d, n = _label(ctx, d_mask, connectivity)
    h, w = d.shape
    r = (C.c_longlong * 4)()
    ctx._check(ctx._lib.ipa_label_largest_dev(ctx.handle, d.ptr, h, w, w, int(n), r), 'largest_component')
    return None if r[0] == 0 else (int(r[0]), int(r[1]), (int(r[2]), int(r[3])))


def _zeros(ctx, shape, dtype):
    d = DeviceArray(ctx, shape, dtype)
    ctx._check(ctx._lib.ipa_memset(ctx.handle, d.ptr, 0, d.nbytes), 'memset')
    return d


def spot_take(img, labels=None, label=0, rows=None, bg=None, fit=None, mask=None, ctx=None):
    """vignettingFromSpotAverage.py:72-77 for one frame -> (fit, mask, maximum, sum, count): where
    the int32 `labels` equal `label` (the spot form) or, with rows=(r, c), on the whole rows r and c
    (the row form, what ``img[np.array([r, c])]`` selects), fit = img - bg and mask = 1
    (ipa_spot_take_dev).  fit (float64) and mask (uint8) are DeviceArrays updated in place, or None
    for new zeroed ones; a host frame gives host arrays back.  The sum is added in a fixed order:
    identical bits from call to call."""
    if (labels is None) == (rows is None):
        raise ValueError('spot_take takes a label image with a label, or a pair of rows')
    dev, ctx, d, d_bg, args = _src('spot_take', img, bg, ctx, (labels, fit, mask))
    h, w = d.shape
    ra, rb = (0, 0) if rows is None else (int(rows[0]), int(rows[1]))
    if rows is not None and not (0 <= ra < h and 0 <= rb < h):
        raise IndexError('spot_take: rows %d and %d of a frame of %d rows' % (ra, rb, h))
    d_labels = None
    if labels is not None:
        if int(label) < 1:
            raise ValueError('spot_take: labels start at 1 (got %r)' % (label,))
        d_labels = _labels_dev('spot_take', labels, (h, w), ctx)
    for what, a, dt in (('fit', fit, np.float64), ('mask', mask, np.uint8)):
        if a is not None and (not _is_dev(a) or a.dtype != dt or tuple(a.shape) != (h, w)):
            raise ValueError('spot_take: %s must be a %s DeviceArray of shape %s'
                             % (what, np.dtype(dt).name, (h, w)))
    d_fit = fit if fit is not None else _zeros(ctx, (h, w), np.float64)
    d_mask = mask if mask is not None else _zeros(ctx, (h, w), np.uint8)
    r = (C.c_double * 3)()
    ctx._check(ctx._lib.ipa_spot_take_dev(*(args + (
        d_labels.ptr if d_labels is not None else None, w, int(label), ra, rb, d_fit.ptr, w, d_mask.ptr, w, r))),
        'spot_take')
    return _stage_out(dev, d_fit), _stage_out(dev, d_mask), r[0], r[1], int(r[2])
