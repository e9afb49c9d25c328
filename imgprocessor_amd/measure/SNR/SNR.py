"""Signal-to-noise maps: the reference's measure/SNR/SNR.py.

The signal (3x3 median of the frame, or of the mean of two), the background grid and the map
itself run in HIP kernels (csrc/nlf.hip; ops.nlf_signal, ops.snr_bg_median, ops.snr_map); with
``noise_level_function=None`` the NLF is estimated by camera/NoiseLevelFunction.py, whose frame
passes are kernels too.  Host frames give a host map, DeviceArrays a DeviceArray.
"""
import numpy as np

from ... import ops
from ..._staging import _frame_pair
from ...camera import NoiseLevelFunction as NLF
from ...device import DeviceArray


def SNR(img1, img2=None, bg=None, noise_level_function=None, constant_noise_level=False,
        imgs_to_be_averaged=False):
    """Returns a signal-to-noise map (float64).

    img2 - second exposure of the same scene: the signal is the mean of both.  Needs ``bg``
        (TypeError otherwise, as the reference's subtraction of None).
    bg - dark current, scalar or (h, w) array, subtracted from both frames; None: a background
        level is estimated from img1 (getBackgroundLevel) and subtracted from the signal
    noise_level_function - a (minY, ax, ay) triple of NoiseLevelFunction.boundedFunction or the
        function oneImageNLF returns (both evaluated on the device), any other callable
        (evaluated on the HOST on the signal and uploaded), or None: estimated from the frames
    constant_noise_level - True: the noise is one number, the mean absolute noise of the frame.
        A NaN in the signal then raises ValueError (the reference returns an all-NaN map).
    imgs_to_be_averaged - True: the SNR of average(img1, img2)
    """
    if img2 is not None and bg is None:
        raise TypeError('SNR: a second image needs bg (the reference subtracts it from img2)')
    dev, ctx, d1, d2, _, _ = _frame_pair('SNR', img1, img2, None, (bg,))
    if bg is not None and not isinstance(bg, DeviceArray) and np.ndim(bg) != 0:
        bg = ctx.to_device(np.ascontiguousarray(np.broadcast_to(np.asarray(bg, np.float64), d1.shape)))
    signal = ops.nlf_signal(d1, d2, bg=bg)
    # noise reduction of an average of two frames
    factor = 0.5 ** 0.5 if imgs_to_be_averaged else 1.0
    bg_level = getBackgroundLevel(d1) if bg is None else 0.0
    if constant_noise_level:
        mn, mx, _, _, n_nan = ops.nlf_moments(signal)
        if n_nan:
            raise ValueError('%d NaN values in the signal: no constant noise level' % n_nan)
        # mean |d| over the frame: the binned reduction with one bin spanning [min, max]
        if d2 is not None:
            counts, sums = ops.nlf_bins(d1, signal, [mn, mx], mx - mn, img2=d2, bg=bg, factor=1.0)
            # 0.5**0.5 because of the sum of variances
            noise = 0.5 ** 0.5 * (sums[0] / counts[0]) * NLF.F_RMS2AAD
        else:
            counts, sums = ops.nlf_bins(d1, signal, [mn, mx], mx - mn, bg=bg,
                                        factor=NLF.F_NOISE_WITH_MEDIAN)
            noise = (sums[0] / counts[0]) * NLF.F_RMS2AAD
        snr = ops.snr_map(signal, constant_noise=noise, noise_factor=factor, bg_level=bg_level)
    else:
        fn = noise_level_function
        if fn is None:
            x, y, weights, _ = NLF._calc(d1, d2, signal, None, None, 'AAD', False, bg)
            fn = NLF._evaluate(x, y, weights)[1]
        triple = getattr(fn, 'triple', None)
        if triple is None and not callable(fn):
            triple = tuple(float(v) for v in fn)
            if len(triple) != 3:
                raise TypeError('noise_level_function must be a callable or a (minY, ax, ay) triple')
        if triple is not None:
            snr = ops.snr_map(signal, nlf=triple, noise_factor=factor, bg_level=bg_level)
        else:
            noise = np.broadcast_to(np.asarray(fn(signal.get()), dtype=np.float64), signal.shape)
            snr = ops.snr_map(signal, noise=ctx.to_device(noise), noise_factor=factor,
                              bg_level=bg_level)
    return snr if dev else snr.get()


def getBackgroundLevel(img):
    """the 1 % point of the histogram of the 3x3 median of every 10th pixel (the border of 10
    left out).  Frames of more than 20 rows and columns."""
    return _cdf(np.asarray(_host(ops.snr_bg_median(img))), 0.01)


def _host(a):
    return a.get() if isinstance(a, DeviceArray) else a


def _cdf(arr, pos):
    """utils/cdf.py:7-20: the intensity at position ``pos`` (0 - 1) of the cumulative density"""
    r = (arr.min(), arr.max())
    hist, bin_edges = np.histogram(arr, bins=2 * int(r[1] - r[0]), range=r)
    cdf = np.cumsum(np.asarray(hist, dtype=np.float64) / hist.sum())
    return bin_edges[np.argmax(cdf > pos)]
