"""The noise-level-function and SNR family of ``ops`` (csrc/nlf.hip), re-exported there as
``ops.nlf_signal``, ``ops.nlf_moments``, ``ops.nlf_bins``, ``ops.snr_map`` and ``ops.snr_bg_median``.
Like every family it goes through ``_stage_in`` / ``_stage_out``: host arrays in give host arrays
out, DeviceArrays stay on the device; counts, sums and moments are always small host values.
"""
import numpy as np

from . import _lib as L
from .device import DeviceArray, dtype_id
from ._staging import (PIXEL_DTYPES, _bg, _dev_out, _dptr, _f64_frame, _f64_host, _frame_pair, _p, _px_host,
                       _stage_in, _stage_out)

_nlf_frames = _frame_pair   # the name it had while it lived here


def nlf_signal(img, img2=None, bg=None, ctx=None):
    """the signal of camera/NoiseLevelFunction.py:208-228 and measure/SNR/SNR.py:37-47 as float64:
    median_filter(img, 3), or median_filter(0.5 * (img + img2), 3) for a pair, each frame read as
    `frame - bg` (scalar or (h, w) array; None: as it is).  uint8 / uint16 / float32 / float64
    frames (other host types go to float64); host in, host out, DeviceArray in, DeviceArray out
    (ipa_nlf_signal_dev)."""
    dev, ctx, d, d2, h, w = _frame_pair('nlf_signal', img, img2, ctx, (bg,))
    d_bg, bgp, bg_pitch, bgv = _bg('nlf_signal', bg, (h, w), ctx)   # d_bg: held until after the call
    d_out = DeviceArray(ctx, (h, w), np.float64)
    ctx._check(ctx._lib.ipa_nlf_signal_dev(
        ctx.handle, d.ptr, dtype_id(d.dtype), d2.ptr if d2 is not None else None, h, w, w, w, bgp,
        bg_pitch, bgv, d_out.ptr, w), 'nlf_signal')
    return _stage_out(dev, d_out)


def nlf_moments(img, ctx=None):
    """(min, max, mean, population std, number of NaN values) of a frame, the first four over its
    non-NaN values and in float64: what camera/NoiseLevelFunction.py:162-173 (_getMinMax) reads
    (ipa_nlf_moments_dev; two passes, no float atomics).  uint8 / uint16 / float32 / float64, host
    array or DeviceArray (other host types go to float64)."""
    _, ctx, d, h, w = _stage_in('nlf_moments', img, ctx, PIXEL_DTYPES, _px_host)
    m = np.empty(5, np.float64)
    ctx._check(ctx._lib.ipa_nlf_moments_dev(ctx.handle, d.ptr, dtype_id(d.dtype), h, w, w, _dptr(m)),
               'nlf_moments')
    return float(m[0]), float(m[1]), float(m[2]), float(m[3]), int(m[4])


def nlf_bins(img, signal, edges, step, img2=None, bg=None, factor=1.0, rms=False, ctx=None):
    """the binned reduction of camera/NoiseLevelFunction.py:243-271 -> (counts int64, sums float64),
    small host arrays of len(edges) - 1: bin n holds the pixels with edges[n] <= signal <=
    edges[n + 1] (both ends inclusive), sums[n] is the sum of |diff| (of diff ** 2 with rms) with
    diff = (img - signal) * factor, or (img - img2) / factor for a pair.  `edges` is the table
    e[k + 1] = e[k] + step.  1 to 2048 bins, NotImplementedError above (ipa_nlf_bins_dev)."""
    _, ctx, d, d2, h, w = _frame_pair('nlf_bins', img, img2, ctx, (signal, bg))
    d_sig = _f64_frame('nlf_bins', 'signal', signal, (h, w), ctx)
    d_bg, bgp, bg_pitch, bgv = _bg('nlf_bins', bg, (h, w), ctx)   # d_bg: held until after the call
    e = np.ascontiguousarray(edges, dtype=np.float64).ravel()
    nbins = e.size - 1
    counts, sums = np.zeros(max(nbins, 0), np.uint64), np.zeros(max(nbins, 0), np.float64)
    ctx._check(ctx._lib.ipa_nlf_bins_dev(
        ctx.handle, d.ptr, dtype_id(d.dtype), d2.ptr if d2 is not None else None, h, w, w, w, bgp,
        bg_pitch, bgv, d_sig.ptr, w, _dptr(e), nbins, float(step), float(factor), int(bool(rms)),
        _p(counts), _dptr(sums)), 'nlf_bins')
    return counts.astype(np.int64), sums


def snr_map(signal, nlf=None, noise=None, constant_noise=None, noise_factor=1.0, bg_level=0.0,
            out=None, ctx=None):
    """measure/SNR/SNR.py:59-79 per pixel of a float64 signal (ipa_snr_map_dev).  Exactly one of
    nlf (the (minY, ax, ay) triple, evaluated on the device), noise (an (h, w) array the caller
    evaluated) and constant_noise (a scalar, not clamped to 1).  noise_factor: 0.5 ** 0.5 for
    imgs_to_be_averaged.  Host in, host out; DeviceArray in, DeviceArray out."""
    if (nlf is not None) + (noise is not None) + (constant_noise is not None) != 1:
        raise ValueError('snr_map takes exactly one of nlf, noise and constant_noise')
    dev, ctx, d, h, w = _stage_in('snr_map', signal, ctx, (np.float64,), _f64_host, (noise, out))
    d_noise = None if noise is None else _f64_frame('snr_map', 'noise', noise, (h, w), ctx)
    d_out = _dev_out(ctx, out, (h, w), np.float64) if dev else DeviceArray(ctx, (h, w), np.float64)
    ctx._check(ctx._lib.ipa_snr_map_dev(
        ctx.handle, d.ptr, h, w, w, L.dbl(nlf, 3) if nlf is not None else None,
        d_noise.ptr if d_noise is not None else None, w,
        0.0 if constant_noise is None else float(constant_noise), float(noise_factor),
        float(bg_level), d_out.ptr, w), 'snr_map')
    return _stage_out(dev, d_out)


def snr_bg_median(img, ctx=None):
    """median_filter(img[10:-10:10, 10:-10:10], 3) as float64, the grid under getBackgroundLevel
    (measure/SNR/SNR.py:82-87; ipa_snr_bg_median_dev).  Frames of more than 20 rows and columns."""
    dev, ctx, d, h, w = _stage_in('snr_bg_median', img, ctx, PIXEL_DTYPES, _px_host)
    if h <= 20 or w <= 20:
        raise ValueError('snr_bg_median: img[10:-10:10, 10:-10:10] is empty for shape %s' % ((h, w),))
    gh, gw = -(-(h - 20) // 10), -(-(w - 20) // 10)
    d_out = DeviceArray(ctx, (gh, gw), np.float64)
    ctx._check(ctx._lib.ipa_snr_bg_median_dev(ctx.handle, d.ptr, dtype_id(d.dtype), h, w, w,
                                              d_out.ptr, gw), 'snr_bg_median')
    return _stage_out(dev, d_out)
