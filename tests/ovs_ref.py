"""numpy restatement of csrc/ovs.hip and of the refinement loop of the reference's
camera/flatField/vignettingFromRandomSteps.py (ObjectVignettingSeparation.__next__, :238-282),
line by line, with the warp as a parameter:

    warp(src, M_dst2src, shape) -> float64 array of `shape`

is cv2.warpPerspective(src, inv(M), shape[::-1]) - the CPU tests pass the oracle's
warp_perspective(LINEAR | Q5, CONSTANT, 0.0), the GPU tests the project's own
ops.warp_perspective(float64, 'linear_cv_q5').  With the latter every comparison is bit for bit:
the taps are the same device function and everything after them is correctly rounded IEEE
arithmetic in a fixed order.

The running mean is the stand-in MaskedMovingAverage of tests/golden/gen_ste_golden.py.
"""
import numpy as np


class MaskedMovingAverage(object):
    def __init__(self, shape):
        self.avg = np.zeros(shape, dtype=np.float64)
        self.n = np.zeros(shape, dtype=np.int32)

    def update(self, arr, mask=None):
        if mask is None:
            mask = np.ones(self.avg.shape, dtype=bool)
        mask = np.asarray(mask, dtype=bool)
        self.n[mask] += 1
        n = self.n[mask]
        a = self.avg[mask]
        x = np.asarray(arr)[mask].astype(np.float64)
        with np.errstate(all='ignore'):
            self.avg[mask] = np.where(n == 1, x, a + (x - a) / n)


def masked_running_mean(avg, n, data, mask=None):
    """kernel (c): one update on copies of the state"""
    m = MaskedMovingAverage(avg.shape)
    m.avg[:], m.n[:] = avg, n
    m.update(data, mask)
    return m.avg, m.n


def ovs_object(warp, ff, fits, M):
    """kernel (a), :241-249; M: destination -> source matrices (what cv2 forms from Hinvs)"""
    obj = MaskedMovingAverage(fits[0].shape)
    with np.errstate(all='ignore'):
        for f, m in zip(fits, M):
            w = warp(ff, m, f.shape)
            obj.update(f / w, w != 0)
    return obj.avg, obj.n


def ovs_flatfield(warp, obj, fits, masks, M, ff_shape):
    """kernel (b), :253-265; M: destination -> source matrices (what cv2 forms from Hs)"""
    s = MaskedMovingAverage(ff_shape)
    with np.errstate(all='ignore'):
        for f, mask, m in zip(fits, masks, M):
            div = f / obj
            div[np.asarray(mask, dtype=bool)] = np.nan
            div = warp(div, m, ff_shape)
            div = np.nan_to_num(div)
            s.update(div, div != 0)
    return s.avg, s.n


def residuum(new, old):
    with np.errstate(all='ignore'):
        return np.nanmean((new[::10, ::10] - old[::10, ::10]) ** 2) ** 0.5


def stop(n, dev, last_dev, max_iter, max_dev):
    """:272-275"""
    return bool(n >= max_iter or (last_dev and ((n > 4 and dev > last_dev) or dev < max_dev)))


class Separation(object):
    """the loop: Hs / Hinvs as the reference holds them, cv2's inversion written out"""

    def __init__(self, warp, ff, fits, masks, Hs, Hinvs=None, max_dev=1e-4, max_iter=10):
        self.warp = warp
        self.flatField = np.array(ff, dtype=np.float64)
        self.fits, self.masks = list(fits), list(masks)
        self.Hs = [np.asarray(h, dtype=np.float64) for h in Hs]
        self.Hinvs = [np.linalg.inv(h) for h in self.Hs] if Hinvs is None else list(Hinvs)
        self.max_dev, self.max_iter = max_dev, max_iter
        self.object = None
        self.residua = []
        self.counts = None

    def __iter__(self):
        self._last_dev = None
        self.n = 0
        return self

    def __next__(self):
        self.object, n_obj = ovs_object(self.warp, self.flatField, self.fits,
                                        [np.linalg.inv(h) for h in self.Hinvs])
        new, n_ff = ovs_flatfield(self.warp, self.object, self.fits, self.masks,
                                  [np.linalg.inv(h) for h in self.Hs], self.flatField.shape)
        self.counts = n_obj, n_ff
        dev = residuum(new, self.flatField)
        self.residua.append(dev)
        if stop(self.n, dev, self._last_dev, self.max_iter, self.max_dev):
            raise StopIteration
        self.flatField = np.clip(new, 0, 1)
        self.n += 1
        self._last_dev = dev
        return self.n

    def run(self):
        for _ in self:
            pass
        return self.flatField, self.object


def next_explicit(warp, ff, fits, masks, Hs, Hinvs):
    """one __next__ as the reference writes it: a warped frame per image, a separate
    MaskedMovingAverage -> (object, new flat field)"""
    obj = MaskedMovingAverage(fits[0].shape)
    with np.errstate(all='ignore'):
        for f, h in zip(fits, Hinvs):
            warped = warp(ff, np.linalg.inv(h), f.shape)
            obj.update(f / warped, warped != 0)
        s = MaskedMovingAverage(ff.shape)
        for f, mask, h in zip(fits, masks, Hs):
            div = f / obj.avg
            div[mask] = np.nan
            div = np.nan_to_num(warp(div, np.linalg.inv(h), ff.shape))
            s.update(div, div != 0)
    return obj.avg, s.avg
