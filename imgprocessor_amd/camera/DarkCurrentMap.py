"""Dark current calibration from dark frames: the reference's camera/DarkCurrentMap.py.

Dark frames of several exposure times give, per pixel, the line image(t) = offset + ascent * t:
the frames of one exposure time are averaged without their single-time effects
(``DarkCurrentMap``, a SingleTimeEffectDetection with nStd=3), the averages are cast into the
frames' own type, and one kernel fits the line through them (``getLinearityFunction``,
ops.stack_linregress).  Everything runs in HIP kernels (csrc/ste.hip, csrc/nlf.hip, csrc/dark.hip);
only the fit of the noise level function over ~50 bins is host work, as in NoiseLevelFunction.

Frames are (h, w) arrays, uint8 / uint16 / float32 / float64, host arrays or DeviceArrays.  With
device frames the stack, the per-group STE state and the averages never leave the device and
``getDarkCurrentFunction`` returns three DeviceArrays; host frames are uploaded once per group
and the results come back as numpy arrays.

From the fit to a corrected frame - ``CameraCalibration.calcDarkCurrent`` returns stored data as
they are (its quirk is pinned), so the model is evaluated in front of ``correct``:

    offs, ascent, rmse = getDarkCurrentFunction(exposuretimes, dark_frames)
    bg = ops.dark_current_eval(offs, ascent, t, 2 ** depth - 1)
    out = cal.correct(img, bgImages=bg)          # a host array: bg.get() where offs is a DeviceArray

Differences from the reference:
  - ``noise_level_function=None``: the estimate ``oneImageNLF(min(i1, i2))[0]`` is made here, in
    front of SingleTimeEffectDetection (which refuses None), on the device.  On dark frames -
    constant read noise over a narrow signal range - the square-root fit normally fails and the
    estimate is NoiseLevelFunction's ClippedPolyNLF or ConstantNLF; the STE class evaluates those
    on the device too.
  - ``calcVariance=True``, ``uncertaintyMap()`` and ``uncertainty()`` raise NotImplementedError
    before any device is touched: the variance of fancytools' MaskedMovingAverage cannot be pinned.
  - frames are arrays, not file paths (TypeError).
  - ``addImg(img, raiseIfConvergence=True)`` raises AttributeError, as the reference does: it calls
    ``checkConvergence`` where its base class ``Iteratives`` defines ``checkConverence``.  Both
    names are kept as they are written there.
  - the per-pixel regression (fancytools.math.linRegressUsingMasked2dArrays in the reference) is
    not part of the reference tree: its definition is this project's, see ops.stack_linregress.
"""
from collections import OrderedDict

import numpy as np

from .. import ops, ops_dark
from .._staging import frame_stack
from ..device import DeviceArray, default_context
from ..features.SingleTimeEffectDetection import SingleTimeEffectDetection
from .NoiseLevelFunction import oneImageNLF


class EnoughImages(Exception):
    """the iteration has converged (the reference's imgProcessor.exceptions.EnoughImages)"""


class Iteratives(object):
    """the stop rule of classes that are fed image by image (the reference's
    utils/baseClasses.py): stop after max_iter images, or once the mean deviation falls under
    max_dev or, after the fifth image, rises again"""

    def __init__(self, max_iter=1e4, max_dev=1e-5):
        self._max_iter, self._max_dev = max_iter, max_dev
        self._last_dev = None
        self._n = 0

    def checkConverence(self, arr):
        """(spelled as in the reference) raises EnoughImages when the iteration may stop"""
        dev = np.mean(arr)
        print('residuum: %s' % dev)
        if self._n > self._max_iter:
            raise EnoughImages()
        if self._last_dev and (dev < self._max_dev or (self._n > 4 and dev > self._last_dev)):
            raise EnoughImages()


def _is_path(f):
    return isinstance(f, (str, bytes)) or hasattr(f, '__fspath__')


def _refuse_paths(frames):
    if _is_path(frames) or any(_is_path(f) for f in frames):
        raise TypeError('DarkCurrentMap takes arrays, not file paths')


class DarkCurrentMap(Iteratives):
    """averages background images, removing single-time effects (nStd = 3)"""

    def __init__(self, twoImages, noise_level_function=None, calcVariance=False, **kwargs):
        Iteratives.__init__(self, **kwargs)
        if calcVariance:
            raise NotImplementedError('calcVariance is not part of the HIP path')
        _refuse_paths(twoImages)
        if len(twoImages) < 2:
            raise ValueError('need at least 2 images')
        if noise_level_function is None:
            # SingleTimeEffectDetection.py:41-42, in front of the class that refuses None
            noise_level_function = oneImageNLF(ops.pair_min(twoImages[0], twoImages[1]))[0]
        self.det = SingleTimeEffectDetection(twoImages, noise_level_function, nStd=3)

    def addImg(self, img, raiseIfConvergence=False):
        if _is_path(img):
            raise TypeError('DarkCurrentMap takes arrays, not file paths')
        self.det.addImage(img)
        if raiseIfConvergence:
            # AttributeError, as in the reference: Iteratives spells it checkConverence
            return self.checkConvergence(None)

    def map(self):
        return self.det.noSTE

    def uncertaintyMap(self):
        raise NotImplementedError('the variance of the running mean is not part of the HIP path')

    def uncertainty(self):
        raise NotImplementedError('the variance of the running mean is not part of the HIP path')


def averageSameExpTimes(imgs):
    """the STE-free average of background images of one exposure time (at least two)"""
    _refuse_paths(imgs)
    d = DarkCurrentMap(imgs[:2])
    for i in imgs[2:]:
        d.addImg(i)
    return d.map()


def getLinearityFunction(expTimes, imgs, mxIntensity=65535, min_ascent=0.001):
    """-> offset, ascent, error of image(expTime) = offset + ascent * expTime, per pixel
    (ops.stack_linregress; 2 to 64 images)"""
    return ops.stack_linregress(expTimes, imgs, mx_intensity=mxIntensity, min_ascent=min_ascent)


def sortForSameExpTime(expTimes, imgs):
    """-> exposure times in ascending order, and for each the list of its images in the order
    given"""
    d = {}
    for e, i in zip(expTimes, imgs):
        d.setdefault(e, []).append(i)
    d = OrderedDict(sorted(d.items()))
    return list(d.keys()), list(d.values())


def _check_series(exposuretimes, imgs, fit):
    """the refusals of getDarkCurrentAverages (and, with fit, of the regression behind it), before
    any device is touched -> the frames are DeviceArrays"""
    _refuse_paths(imgs)
    if len(exposuretimes) != len(imgs):
        raise ValueError('%d exposure times for %d images' % (len(exposuretimes), len(imgs)))
    if len(imgs) == 0:
        raise ValueError('no images')
    dev = [isinstance(i, DeviceArray) for i in imgs]
    if any(dev) and not all(dev):
        raise TypeError('mix of host and device frames')
    f0 = imgs[0]
    for f in imgs:
        if len(f.shape) != 2:
            raise TypeError('frames are single-channel (h, w) arrays, got shape %s' % (tuple(f.shape),))
        if tuple(f.shape) != tuple(f0.shape) or f.dtype != f0.dtype:
            raise ValueError('frames must share shape and dtype')
    if np.dtype(f0.dtype) not in ops.STE_DTYPES:
        raise TypeError('frames are uint8 / uint16 / float32 / float64 (got %s)' % np.dtype(f0.dtype))
    n_times = len(set(exposuretimes))
    if fit and n_times < 2:
        raise ValueError('a line needs at least 2 different exposure times (got %d)' % n_times)
    if fit and n_times > ops_dark.MAX_FRAMES:
        raise NotImplementedError('at most %d different exposure times (got %d)'
                                  % (ops_dark.MAX_FRAMES, n_times))
    return all(dev)


def _averages(exposuretimes, imgs, fit=False):
    """-> (dev, exposure times, (T, h, w) DeviceArray of the averages in imgs[0].dtype)"""
    imgs = list(imgs)
    _refuse_paths(imgs)
    imgs = [i if isinstance(i, DeviceArray) else np.asarray(i) for i in imgs]
    dev = _check_series(exposuretimes, imgs, fit)
    x, groups = sortForSameExpTime(exposuretimes, imgs)
    ctx = imgs[0].ctx if dev else default_context()
    h, w = imgs[0].shape
    stack = DeviceArray(ctx, (len(x), h, w), imgs[0].dtype)
    for n, group in enumerate(groups):
        if len(group) == 1:
            stack.frame(n).copy_from(group[0] if dev else ctx.to_device(group[0]))
            continue
        # a host group goes up once, as one stack
        d = frame_stack('getDarkCurrentAverages', group)
        d = d if dev else ctx.to_device(d)
        m = DarkCurrentMap([d.frame(k) for k in range(2)])
        for k in range(2, len(group)):
            m.addImg(d.frame(k))
        ops.cast_trunc(m.map(), stack.dtype, out=stack.frame(n))
    return dev, x, stack


def getDarkCurrentAverages(exposuretimes, imgs):
    """-> exposure times (ascending), (T, h, w) stack of the STE-free average of every exposure
    time, in the type of imgs[0] (truncated, as numpy's assignment into that type); a single
    frame of an exposure time is copied as it is"""
    dev, x, stack = _averages(exposuretimes, imgs)
    return x, (stack if dev else stack.get())


def getDarkCurrentFunction(exposuretimes, imgs, **kwargs):
    """the dark current function from images and exposure times -> offset, ascent, rmse; kwargs:
    mxIntensity, min_ascent of getLinearityFunction.  At least 2 and at most 64 different
    exposure times."""
    dev, x, stack = _averages(exposuretimes, imgs, fit=True)
    out = getLinearityFunction(x, stack, **kwargs)
    return out if dev else tuple(o.get() for o in out)
