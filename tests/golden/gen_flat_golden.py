#!/usr/bin/env python3
"""Generate tests/golden/flat.npz: the flat field from close-distance frames as the reference
computes it (camera/flatField/flatFieldFromCloseDistance.py over transform/imgAverage.py,
utils/getBackground2.py, transformations.toGray, features/SingleTimeEffectDetection.py and
camera/NoiseLevelFunction.py).  Runs only where the reference source exists.

The reference runs unchanged under the throw-away stand-ins of gen_ste_golden.py (numba shim,
constants-only cv2, the running mean) and, as in gen_nlf_golden.py, with ``np.asfarray`` put back.
Two import-only stubs more go to the temp dir (never committed) where the real modules cannot be
imported: ``fancytools.os.PathStr`` and ``fancytools.math.findXAt``, which imgSignal and
FitHistogramPeaks import and no call of these scenes reaches.

The reference's classes are not changed; the generator only listens.  A subclass of its
SingleTimeEffectDetection notes, per frame added, which decisions a last-digit difference in the
host fit cannot flip: the STE decision (|frame - avg - thr| >= 1e-5 * thr) and the lower mask the
caller hands over (|frame - (avg - n)| >= 1e-5 * n with n = nlf(avg) * nstd), and identifies
the frames as they arrive: that is the recorded sort order.  The generator
asserts that the square-root fit succeeded, that at most 1 % of the pixels of any frame fall
outside that stable set, and that no pixel of the [::10, ::10] grid does in any frame - so the
divisor is pinned.

The inputs are the seeded scenes of tests/flat_cases.py; the fixture holds arrays only.

    python tests/golden/gen_flat_golden.py [other/path/flat.npz]
"""
import os
import sys
import warnings

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
sys.path.insert(0, os.path.dirname(HERE))
from gen_golden import install_shim  # noqa: E402
from gen_ste_golden import install_standins  # noqa: E402
import flat_cases as fc  # noqa: E402

warnings.filterwarnings('ignore')

STABLE = 1e-5
SUB = 2   # scene (b)'s frame-sized arrays are stored every SUB-th pixel


def install_stubs():
    """import-only stand-ins for the fancytools modules imgSignal / FitHistogramPeaks pull in"""
    import fancytools
    d = os.path.dirname(list(fancytools.__path__)[0])
    made = []
    for mod, body in (('fancytools.os.PathStr', 'class PathStr(str):\n    pass\n'),
                      ('fancytools.math.findXAt',
                       'def findXAt(*a, **k):\n    raise NotImplementedError("import-only stub")\n')):
        try:
            __import__(mod)
        except ImportError:
            assert 'ste_standins_' in d, 'the stubs go to the temp dir only'
            pkg, name = mod.rsplit('.', 1)
            pdir = os.path.join(d, *pkg.split('.'))
            os.makedirs(pdir, exist_ok=True)
            init = os.path.join(pdir, '__init__.py')
            if not os.path.exists(init):
                open(init, 'w').close()
            with open(os.path.join(pdir, name + '.py'), 'w') as f:
                f.write(body)
            made.append(mod)
    return made


def main(path=os.path.join(HERE, 'flat.npz')):
    if not hasattr(np, 'asfarray'):
        np.asfarray = lambda a, dtype=np.float64: np.asarray(a, dtype=dtype)
    install_shim()
    mma_source = install_standins()
    stubs = install_stubs()
    from imgProcessor.camera.flatField import flatFieldFromCloseDistance as F
    from imgProcessor.camera import NoiseLevelFunction as N
    from imgProcessor.features import SingleTimeEffectDetection as S

    out = {'mma_source': np.array(mma_source), 'stubs': np.array(stubs)}
    # ---- scene (a): nothing in it is fitted
    for dtype in fc.ALL_DTYPES:
        frames, bgs = fc.colour_scene(dtype)
        p = 'a_%s_' % np.dtype(dtype).name
        out[p + 'in_sum'] = np.array([np.asarray(f, np.float64).sum() for f in frames + bgs])
        out[p + 'ff'] = F.flatFieldFromCloseDistance([f.copy() for f in frames], [b.copy() for b in bgs])
        out[p + 'ff_scalar_bg'] = F.flatFieldFromCloseDistance([f.copy() for f in frames], 9.5)
        assert out[p + 'ff'].shape == fc.A_SHAPE[:2] and out[p + 'ff'].dtype == np.float64
    # the reference is defined for colour frames only
    try:
        F.flatFieldFromCloseDistance([f[..., 0].copy() for f in frames], 0.0)
        raise AssertionError('the reference took (h, w) frames')
    except (ValueError, ZeroDivisionError, IndexError, np.exceptions.AxisError):
        pass

    # ---- scene (b)
    fits, dets = [], []
    ref_evaluate = N._evaluate

    def evaluate(x, y, weights):
        res = ref_evaluate(x, y, weights)
        fits.append(res[0])
        return res

    N._evaluate = evaluate

    class Listening(S.SingleTimeEffectDetection):
        def __init__(self, images, nlf, nStd=4, **kwargs):
            self.stable, self.masks, self.added, self.nstd = [], [], [], nStd
            self.first_pair = images
            dets.append(self)
            S.SingleTimeEffectDetection.__init__(self, images, nlf, nStd=nStd, **kwargs)

        def addImage(self, image, mask=None):
            thr = np.broadcast_to(np.asarray(self.threshold, dtype=np.float64), self.noSTE.shape)
            st = np.abs(image - self.noSTE - thr) >= STABLE * thr
            if mask is not None:   # the caller's lower mask: image > noSTE - n
                n = self.noise_level_function(self.noSTE) * self.nstd
                assert np.array_equal(mask, image > self.noSTE - n)
                st &= np.abs(image - (self.noSTE - n)) >= STABLE * n
            self.stable.append(st)
            self.masks.append(mask)
            self.added.append(image)
            return S.SingleTimeEffectDetection.addImage(self, image, mask)

    F.SingleTimeEffectDetection = Listening
    frames, bgs = fc.vignetting_scene()
    ff = F.flatFieldFromCloseDistance2([f.copy() for f in frames], [b.copy() for b in bgs], nstd=fc.B_NSTD)
    assert len(dets) == 1 and len(fits) == 1 and fits[0] is not None, 'scene (b) must take the square root'
    det = dets[0]
    # the constructor's own addImage (the maximum of the pair) and one per frame of images[1:]
    assert len(det.stable) == len(frames)
    # the order the reference sorted the frames into, as its detector saw them arrive: the first
    # pair minus the background, then images[1:] raw
    avg_bg = F.imgAverage([b.copy() for b in bgs])

    def which(a, minus_bg):
        hits = [k for k, f in enumerate(frames) if np.array_equal(a, f.astype(float) - avg_bg if minus_bg else f)]
        assert len(hits) == 1, hits
        return hits[0]
    raw = [which(a, False) for a, m in zip(det.added, det.masks) if m is not None]
    order = [which(det.first_pair[0], True)] + raw
    assert which(det.first_pair[1], True) == raw[0] and sorted(order) == list(range(len(frames)))
    # ... which is the sort by the key in the frames' own type (it wraps for uint16)
    assert order == sorted(range(len(frames)), key=lambda k: -frames[k][::6, ::8].min())
    assert order[-1] == fc.B_DARK[0] and fc.B_DARK[0] not in order[:2]
    worst = 0.0
    for s in det.stable:
        worst = max(worst, 1.0 - s.mean())
        assert s[::10, ::10].all(), 'a pixel of the [::10, ::10] grid is within 1e-5 of a threshold'
    # a condition of the tests that use the stable mask, not a measurement
    assert worst <= 0.01, 'a frame has %.2f %% of its pixels within 1e-5 of a threshold' % (100 * worst)
    stable = np.all(det.stable, axis=0)
    # what the scene is for: the hits and the dark block stay out of the average
    for k, pts in fc.B_HITS:
        for pt in pts:
            assert ff[pt] < 1.05, 'a planted hit reached the flat field'
    assert not det.masks[-1][fc.B_DARK[1]].any() and det.masks[-1].mean() > 0.95, 'the dark block was not masked'
    assert all(m[fc.B_DARK[1]].all() for m in det.masks[1:-1])
    out['b_in_sum'] = np.array([np.asarray(f, np.float64).sum() for f in frames + bgs])
    out['b_order'] = np.array(order)
    out['b_nlf'] = np.array(fits[0], dtype=np.float64)   # (minY, ax, ay)
    out['b_thr'] = np.asarray(det.threshold, np.float64)[::SUB, ::SUB]
    out['b_ff'] = ff[::SUB, ::SUB].copy()
    out['b_stable'] = stable[::SUB, ::SUB]
    out['b_divisor'] = np.array(F.median_filter(det.noSTE[::10, ::10], 3).max())
    out['unstable_worst'] = np.array(worst)
    np.savez_compressed(path, **out)
    size = os.path.getsize(path)
    assert size <= 100 * 1024, size
    print('wrote %s (%d bytes, %d arrays; running mean: %s, stubs: %s; order %s; worst unstable '
          'fraction %.2e)' % (path, size, len(out), mma_source, stubs, order, worst))


if __name__ == '__main__':
    main(*sys.argv[1:2])
