"""The three resampling steps of the reference's
imgProcessor/camera/flatField/vignettingFromRandomSteps.py (ObjectVignettingSeparation):

  :245  ``cv2.warpPerspective(self.flatField, h, (f.shape[1], f.shape[0]))``
        the current flat field seen from the position of one fitted image
  :260  ``cv2.warpPerspective(div, h, (sh[1], sh[0]))`` on ``div = f / object`` with the
        background set to NaN, then ``np.nan_to_num``: the ratio image brought back onto the
        flat-field grid (NaN sources stay out of the interpolation: a footprint that touches a
        NaN gives NaN, and NaN becomes 0 = "no value" for the masked average that follows)
  :309  ``cv2.warpPerspective(img, H_inv, (s[1], s[0]))`` in ``_fitImg``: an input image
        fitted onto the object grid

All three are plain calls (no WARP_INVERSE_MAP): OpenCV inverts the 3x3 matrix and samples
bilinearly with coordinates rounded to 1/32 px, constant border 0.  Here that is
``ops.warp_perspective(..., 'linear_cv_q5')`` with inv(H) - float32 and float64 (the flat
field and the ratio images are float64 in the reference) run in their own precision.
Feature matching and the homography search are host-side work outside the project.

The refinement loop around :245 and :260 (``__iter__`` / ``__next__``, :228-282) is
``ObjectVignettingSeparation`` below: two launches a step (csrc/ovs.hip), the warps, the
divisions and the masked moving averages fused per pixel, for fits and homographies the caller
supplies.  The three functions stay as they are for callers that warp single images.
"""
import numpy as np

from ... import ops
from ..._staging import PIXEL_DTYPES, _ctx_of, _px_host
from ...device import DeviceArray


def _warp(img, H, shape, ctx=None):
    Minv = np.linalg.inv(np.asarray(H, dtype=np.float64))
    dev = isinstance(img, DeviceArray)
    if not dev:
        img = np.asarray(img)
        if img.dtype not in (np.uint8, np.uint16, np.float32, np.float64):
            img = img.astype(np.float64)
    return ops.warp_perspective(img, Minv, (int(shape[0]), int(shape[1])), 'linear_cv_q5',
                                'constant', 0.0, ctx=ctx)


def warpFlatField(flatField, Hinv, fit_shape, ctx=None):
    """:245 - the flat field warped onto a fitted image's grid (`Hinv` is the matrix the
    reference passes: the inverse homography of that image); fit_shape = f.shape"""
    return _warp(flatField, Hinv, fit_shape, ctx)


def warpRatioToFlatField(fit, obj, fit_mask, H, ff_shape, ctx=None):
    """:255-262 - ``div = fit / obj; div[fit_mask] = nan; warp(div, H); nan_to_num``"""
    with np.errstate(divide='ignore', invalid='ignore'):
        div = np.asarray(fit) / np.asarray(obj)
    div[np.asarray(fit_mask, dtype=bool)] = np.nan
    out = _warp(div, H, ff_shape, ctx)
    return np.nan_to_num(out)


def fitToObject(img, H_inv, obj_shape, ctx=None):
    """:309 - an input image warped onto the object grid"""
    return _warp(img, H_inv, obj_shape, ctx)


MAX_FITS = 64   # kOvsMaxN of csrc/ovs.hip
RESIDUUM_STEP = 10   # the residuum of :269-270 reads every tenth pixel of every tenth row


def stopIteration(n, dev, last_dev, maxIter, maxDev):
    """the stop rule of ``__next__`` (:272-275): n steps done, `dev` the residuum of this pass,
    `last_dev` that of the pass before (None on the first)"""
    return bool(n >= maxIter or (last_dev and ((n > 4 and dev > last_dev) or dev < maxDev)))


def residuum(new_sub, old_sub):
    """:269-270 on the two every-tenth-pixel grids: the rms difference, NaN left out"""
    return np.nanmean((new_sub - old_sub) ** 2) ** 0.5


class ObjectVignettingSeparation(object):
    """The refinement loop of the reference's ObjectVignettingSeparation ("Method D" of Bedrich et
    al.: the same object imaged at random positions, :228-282) for fitted images and homographies
    the caller supplies.  One step is two launches (ops.ovs_object, ops.ovs_flatfield); the fitted
    images, their masks, the flat field and the object stay on the device, and only the residuum's
    every-tenth-pixel grid comes down per step.

        s = ObjectVignettingSeparation(ff_shape, obj_shape)
        for fit, mask, H, img, img_mask in ...:
            s.addFit(fit, mask, H, img=img, img_mask=img_mask)
        flatField, obj = s.separate()

    Not built, and NotImplementedError where the name exists: ``addImg`` (pattern recognition: ORB,
    BFMatcher, RANSAC stay outside the project), ``_findObject``, ``smooth()`` (skimage rank filters
    on a uint8 cast), ``error()``, the module function ``vignettingFromRandomSteps()`` and the lens
    handling of the reference's constructor (undistort the images first).  ``separate()`` therefore
    returns (flatField, object) without the smoothed flat field and its mask.

    The running mean is MaskedMovingAverage as the project restates it and the warp is cv2's as
    ``ops.warp_perspective(..., 'linear_cv_q5')`` restates it; neither is pinned against
    fancytools / cv2 here.
    """

    def __init__(self, ff_shape, obj_shape, maxDev=1e-4, maxIter=10, ctx=None):
        self.ff_shape = self._shape2(ff_shape, 'ff_shape')
        self.obj_shape = self._shape2(obj_shape, 'obj_shape')
        self.maxDev = maxDev
        self.maxIter = maxIter
        self.ctx = ctx
        self.lens = None
        self.object = None
        self.Hs = []       # homographies of all fitted images (object pixel -> image pixel)
        self.Hinvs = []    # the same, inverted
        self.fits = []     # all images fitted to the object grid (device)
        self._fit_masks = []
        self._dev = False          # the first fit came as a DeviceArray: results are DeviceArrays
        self._ff = None            # the flat field (device, float64)
        self._ff_sub = None        # ... and its [::10, ::10] on the host
        self._ff_avg = self._ff_n = None   # MaskedMovingAverage of the images (device)
        self._stacks = None
        self._last_dev = None
        self.n = 0

    @staticmethod
    def _shape2(shape, what):
        shape = tuple(int(s) for s in shape)
        if len(shape) != 2 or min(shape) < 1:
            raise ValueError('%s must be (rows, columns) (got %s)' % (what, shape))
        return shape

    def _context(self, *arrs):
        if self.ctx is None:
            self.ctx = _ctx_of(*arrs)
        return self.ctx

    # -- the flat field ---------------------------------------------------------------------
    @property
    def flatField(self):
        if self._ff is None:
            return None
        return self._ff if self._dev else self._ff.get()

    @flatField.setter
    def flatField(self, arr):
        if not isinstance(arr, DeviceArray):
            arr = np.ascontiguousarray(arr, dtype=np.float64)
        if tuple(arr.shape) != self.ff_shape or arr.dtype != np.float64:
            raise ValueError('flatField must be a float64 array of shape %s (got %s %s)'
                             % (self.ff_shape, arr.dtype, tuple(arr.shape)))
        if isinstance(arr, DeviceArray):
            self._context(arr)
            self._ff = arr
            self._ff_sub = np.ascontiguousarray(arr.get()[::RESIDUUM_STEP, ::RESIDUUM_STEP])
        else:
            self._ff = self._context().to_device(arr)
            self._ff_sub = np.ascontiguousarray(arr[::RESIDUUM_STEP, ::RESIDUUM_STEP])

    # -- input ------------------------------------------------------------------------------
    def addFit(self, fit, mask, H, H_inv=None, img=None, img_mask=None):
        """fit: an image already warped onto the object grid (what fitToObject returns); mask: its
        ``_fit_masks`` entry (set = background, left out); H: the homography object pixel -> image
        pixel, H_inv its inverse (default np.linalg.inv(H)).  img / img_mask (:146-151): the image
        itself and where it shows signal - they update the average the initial flat field is made
        of.  Host arrays or DeviceArrays; everything is kept on the device."""
        H = np.asarray(H, dtype=np.float64)
        H_inv = np.linalg.inv(H) if H_inv is None and H.shape == (3, 3) else np.asarray(H_inv, dtype=np.float64)
        if H.shape != (3, 3) or H_inv.shape != (3, 3):
            raise ValueError('addFit: H and H_inv must be 3 x 3 (got %s, %s)' % (H.shape, H_inv.shape))
        for name, a, shape in (('fit', fit, self.obj_shape), ('mask', mask, self.obj_shape),
                               ('img', img, self.ff_shape), ('img_mask', img_mask, self.ff_shape)):
            if a is not None and tuple(np.shape(a) if not isinstance(a, DeviceArray) else a.shape) != shape:
                raise ValueError('addFit: %s must have shape %s' % (name, shape))
        if img_mask is not None and img is None:
            raise ValueError('addFit: img_mask without img')
        if len(self.fits) >= MAX_FITS:
            raise NotImplementedError('addFit: at most %d fitted images' % MAX_FITS)
        dev = isinstance(fit, DeviceArray)
        ctx = self._context(fit, mask, img, img_mask)
        d_fit = fit if dev else ctx.to_device(_px_host(fit))
        if d_fit.dtype not in PIXEL_DTYPES:
            raise TypeError('addFit: fitted images are uint8 / uint16 / float32 / float64 (got %s)' % d_fit.dtype)
        if self.fits and d_fit.dtype != self.fits[0].dtype:
            raise TypeError('addFit: all fitted images must have one element type (%s, got %s)'
                            % (self.fits[0].dtype, d_fit.dtype))
        d_mask = mask if isinstance(mask, DeviceArray) else ctx.to_device(np.ascontiguousarray(mask, dtype=np.uint8))
        if d_mask.dtype != np.uint8:
            raise TypeError('addFit: a device mask must be uint8')
        if not self.fits:
            self._dev = dev
        if img is not None:
            if self._ff_avg is None:
                self._ff_avg = DeviceArray(ctx, self.ff_shape, np.float64)
                self._ff_n = DeviceArray.counts(ctx, self.ff_shape)
                for a in (self._ff_avg, self._ff_n):
                    ctx._check(ctx._lib.ipa_memset(ctx.handle, a.ptr, 0, a.nbytes), 'memset')
            ops.masked_running_mean_update(self._ff_avg, self._ff_n, img, img_mask, ctx=ctx)
        self.Hs.append(H)
        self.Hinvs.append(H_inv)
        self.fits.append(d_fit)
        self._fit_masks.append(d_mask)
        self._stacks = None
        return fit

    def addImg(self, img, maxShear=0.015, maxRot=100, minMatches=12, borderWidth=3):
        raise NotImplementedError('addImg finds the homography by pattern recognition, which is outside this '
                                  'project: fit the image yourself and call addFit(fit, mask, H)')

    def _findObject(self, img):
        raise NotImplementedError('_findObject (signalMinimum + boundingBox) is not built: pass obj_shape')

    def smooth(self):
        raise NotImplementedError('smooth() (skimage rank filters on a uint8 cast) is not built')

    def error(self, nCells=15):
        raise NotImplementedError('error() is not built')

    # -- the loop ---------------------------------------------------------------------------
    def _stacked(self):
        """the fitted images and their masks as (N, oh, ow) device stacks, and the destination ->
        source matrices cv2 would form: inv(Hinvs[k]) for :245, inv(Hs[k]) for :260"""
        if self._stacks is None:
            ctx, n = self.ctx, len(self.fits)
            fits = DeviceArray(ctx, (n,) + self.obj_shape, self.fits[0].dtype)
            masks = DeviceArray(ctx, (n,) + self.obj_shape, np.uint8)
            for k in range(n):
                fits.frame(k).copy_from(self.fits[k])
                masks.frame(k).copy_from(self._fit_masks[k])
            m_obj = np.stack([np.linalg.inv(h) for h in self.Hinvs])
            m_ff = np.stack([np.linalg.inv(h) for h in self.Hs])
            self._stacks = fits, masks, m_obj, m_ff
        return self._stacks

    def _require(self):
        if not self.fits:
            raise ValueError('no fitted images: call addFit first')
        if self._ff is None:
            raise ValueError('no flat field to start from: give addFit the images (img=) or set flatField')

    def __iter__(self):
        self._require()
        self._last_dev = None
        self.n = 0
        return self

    def __next__(self):
        self._require()
        fits, masks, m_obj, m_ff = self._stacked()
        obj, _ = ops.ovs_object(self._ff, fits, m_obj, ctx=self.ctx)
        self.object = obj if self._dev else obj.get()
        new, _, new_sub = ops.ovs_flatfield(obj, fits, masks, m_ff, self.ff_shape, ctx=self.ctx, clip=True,
                                            sub_step=RESIDUUM_STEP)
        dev = residuum(new_sub, self._ff_sub)
        print('residuum: %s' % dev)
        if stopIteration(self.n, dev, self._last_dev, self.maxIter, self.maxDev):
            raise StopIteration
        # remove erroneous values (:278; the kernel stored the clipped flat field)
        self._ff = new
        self._ff_sub = np.clip(new_sub, 0, 1)
        self.n += 1
        self._last_dev = dev
        return self.n

    def _createInitialflatField(self, downscale_size=9):
        """:284-292 on the average of the images given to addFit"""
        from ...filters.fastFilter import fastFilter
        s0, s1 = self.ff_shape
        f = int(max(s0, s1) / downscale_size)
        every = int(f / 3.5)
        if every < 1:
            raise ValueError('the initial flat field needs a flat field of at least %d pixels along one side'
                             % (4 * downscale_size))
        s = fastFilter(self._ff_avg.get(), f, every, ctx=self.ctx)
        s /= s.max()
        return s

    def separate(self):
        """-> (flatField, object) after the refinement; the initial flat field comes from the
        images given to addFit, or is the one the caller set"""
        if not self.fits:
            raise ValueError('no fitted images: call addFit first')
        if self._ff_avg is not None:
            self.flatField = self._createInitialflatField()
        elif self._ff is None:
            raise ValueError('no flat field to start from: give addFit the images (img=) or set flatField')
        for step in self:
            print('iteration step %s/%s' % (step, self.maxIter))
        return self.flatField, self.object


def vignettingFromRandomSteps(imgs, bg, inPlane_scale_factor=None, debugFolder=None, **kwargs):
    raise NotImplementedError('vignettingFromRandomSteps() drives addImg (pattern recognition), which is outside '
                              'this project: use ObjectVignettingSeparation.addFit and separate()')
