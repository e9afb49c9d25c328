"""Single-time-effect (STE) removal: the reference's features/SingleTimeEffectDetection.py:13-95.

STE are one-frame events - cosmic-ray hits and the like - in a stack of two or more equivalent
exposures.  The running mean, the threshold and the neighbour rule run in one HIP kernel
(csrc/ste.hip, ops.ste_update); the state stays on the device between ``addImage`` calls.

Host frames give host results (numpy arrays), device frames (a (n, h, w) DeviceArray or a list
of (h, w) DeviceArrays) give DeviceArrays.

Not on the GPU path (NotImplementedError, raised before any device is touched):
``noise_level_function=None`` (the reference estimates it with oneImageNLF,
camera/NoiseLevelFunction.py:153-271), ``calcVariance=True``, a ``dtype`` other than float64,
``countSTE`` and ``intensityDistributionSTE``.  Colour frames and file paths raise TypeError.
"""
import numbers

import numpy as np

from .. import ops
from .._staging import frame_stack
from ..device import DeviceArray, default_context


def _nlf_triple(nlf):
    if callable(nlf):
        # an estimated NLF (NoiseLevelFunction.oneImageNLF) carries its parameters: device path
        return getattr(nlf, 'triple', None)
    try:
        t = tuple(float(v) for v in nlf)
    except TypeError:
        raise TypeError('noise_level_function must be a callable or a (minY, ax, ay) triple')
    if len(t) != 3:
        raise TypeError('noise_level_function must be a callable or a (minY, ax, ay) triple')
    return t


def _check_frame(f):
    if isinstance(f, (str, bytes)) or hasattr(f, '__fspath__'):
        raise TypeError('SingleTimeEffectDetection takes arrays, not file paths')
    if len(f.shape) != 2:
        raise TypeError('SingleTimeEffectDetection takes single-channel (h, w) frames, got '
                        'shape %s' % (tuple(f.shape),))


class SingleTimeEffectDetection(object):
    """Removes single-time effects from a stack of at least two exposures of the same scene.

    After construction (and after every ``addImage``):
      ``noSTE``       the running mean of every pixel over the frames in which it was not an STE
      ``mask_clean``  True where the last frame added was not an STE
      ``mask_STE``    True where any frame so far was an STE (None unless save_ste_indices)
      ``threshold``   nlf(min(images[0], images[1])) * nStd, fixed by the first pair

    noise_level_function: a (minY, ax, ay) triple of NoiseLevelFunction.boundedFunction or the
    function NoiseLevelFunction.oneImageNLF returns (its ``.triple``, or the ``.poly`` /
    ``.constant`` of its polynomial fallback), evaluated on the device, or any callable.  Any
    other callable is evaluated on the HOST on
    min(images[0], images[1]) (float64, NaN propagating) and its threshold uploaded: a
    compatibility path with a device -> host -> device round trip for device frames.
    """

    def __init__(self, images, noise_level_function=None, nStd=4,
                 save_ste_indices=False, calcVariance=False, dtype=float):
        if noise_level_function is None:
            raise NotImplementedError(
                'estimating the noise level function (NoiseLevelFunction.oneImageNLF) is not '
                'part of the HIP path: pass a (minY, ax, ay) triple or a callable')
        if calcVariance:
            raise NotImplementedError('calcVariance is not part of the HIP path')
        if np.dtype(dtype) != np.float64:
            raise NotImplementedError('the running mean is float64 only (got dtype %s)' % dtype)
        if isinstance(images, (str, bytes)):
            raise TypeError('SingleTimeEffectDetection takes arrays, not file paths')
        triple = _nlf_triple(noise_level_function)
        if isinstance(images, DeviceArray):
            if images.ndim != 3:
                raise TypeError('device images must be a (n, h, w) DeviceArray')
            frames = images
        elif isinstance(images, np.ndarray):
            if images.ndim != 3:
                raise TypeError('images must be a (n, h, w) stack of single-channel frames')
            frames = images
        else:
            frames = list(images)
            for f in frames:
                if isinstance(f, (str, bytes)) or hasattr(f, '__fspath__'):
                    raise TypeError('SingleTimeEffectDetection takes arrays, not file paths')
                _check_frame(f if hasattr(f, 'shape') else np.asarray(f))
        if (frames.shape[0] if isinstance(frames, DeviceArray) else len(frames)) < 2:
            raise ValueError('SingleTimeEffectDetection needs at least 2 images')
        frames = frame_stack('SingleTimeEffectDetection', frames)
        self._dev = isinstance(frames, DeviceArray)
        self.save_ste_indices = save_ste_indices
        self.noise_level_function = noise_level_function
        self._ctx = frames.ctx if self._dev else default_context()
        ctx = self._ctx
        _, h, w = frames.shape
        self._shape = (h, w)
        self._avg = DeviceArray(ctx, (h, w), np.float64)
        self._count = DeviceArray.counts(ctx, (h, w))
        self._thr = DeviceArray(ctx, (h, w), np.float64)
        self._clean = DeviceArray(ctx, (h, w), np.uint8)
        self._ste = None
        if save_ste_indices:
            self._ste = DeviceArray(ctx, (h, w), np.uint8)
            ctx._check(ctx._lib.ipa_memset(ctx.handle, self._ste.ptr, 0, self._ste.nbytes),
                       'memset')
        if triple is None and ops.nlf_params(noise_level_function) is not None:
            # the polynomial or the constant NoiseLevelFunction.smooth falls back to (what dark
            # frames take): min(f0, f1) and the threshold on the device, nothing comes down
            if not self._dev:
                f = np.asarray(frames)
                frames = ctx.to_device(f if f.dtype in ops.STE_DTYPES else f.astype(np.float64))
            m = ops.pair_min(frames.frame(0), frames.frame(1))
            ops.nlf_threshold(m, noise_level_function, nStd, out=self._thr)
        elif triple is None:
            # host-evaluated NLF: threshold of min(f0, f1) in float64, as the reference (:39-44)
            if self._dev:
                f01 = np.stack([frames.frame(0).get(), frames.frame(1).get()])
            else:
                f01 = np.asarray(frames[:2])
            m = np.min(f01.astype(np.float64), axis=0)
            thr = np.asarray(noise_level_function(m) * nStd, dtype=np.float64)
            self._thr.set(np.broadcast_to(thr, (h, w)))
        ops.ste_update(frames, self._avg, self._count, self._thr, first_pair=True, nlf=triple,
                       nstd=nStd, mask_ste=self._ste, mask_clean=self._clean, ctx=ctx)

    def _out(self, d, as_bool=False):
        if self._dev:
            return d
        a = d.get()
        return a.astype(bool) if as_bool else a

    @property
    def noSTE(self):
        return self._out(self._avg)

    @property
    def threshold(self):
        return self._out(self._thr)

    @property
    def mask_clean(self):
        return self._out(self._clean, True)

    @property
    def mask_STE(self):
        return None if self._ste is None else self._out(self._ste, True)

    def addImage(self, image, mask=None):
        """step the running mean through one more frame; ``mask`` (optional, bool host array or
        uint8 DeviceArray) limits the update to its True pixels, STE decisions are unaffected"""
        if isinstance(image, (str, bytes)):
            raise TypeError('addImage takes an array, not a file path')
        if not isinstance(image, DeviceArray):
            image = np.asarray(image)
        _check_frame(image)
        if tuple(image.shape) != self._shape:
            raise ValueError('image shape %s differs from the stack %s' % (image.shape, self._shape))
        if mask is not None and not isinstance(mask, DeviceArray):
            mask = np.asarray(mask, dtype=bool)
        ops.ste_update(image, self._avg, self._count, self._thr, first_pair=False, nlf=None,
                       mask=mask, mask_ste=self._ste, mask_clean=self._clean, ctx=self._ctx)
        return self

    def countSTE(self):
        raise NotImplementedError('countSTE (scipy.ndimage.label) is not part of the HIP path')

    def relativeAreaSTE(self):
        """fraction of the image's pixels that were an STE in some frame"""
        if self._ste is None:
            raise TypeError('relativeAreaSTE needs save_ste_indices=True')
        s = self._shape
        return np.sum(self._ste.get() != 0) / (s[0] * s[1])

    def intensityDistributionSTE(self, bins=10, range=None):
        raise NotImplementedError('intensityDistributionSTE is not part of the HIP path')
