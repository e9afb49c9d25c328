#!/usr/bin/env python3
"""Generate tests/golden/dark.npz: dark current calibration as the reference computes it
(camera/DarkCurrentMap.py over features/SingleTimeEffectDetection.py and
camera/NoiseLevelFunction.py).  Runs only where the reference source exists.

The reference runs unchanged under the throw-away stand-ins of gen_ste_golden.py (numba shim,
constants-only cv2, the running mean) and, as in gen_nlf_golden.py, with ``np.asfarray`` put
back.  One more stand-in is written to the temp dir (never committed) when the real one cannot be
imported: ``fancytools.math.linRegressUsingMasked2dArrays``, the per-pixel least-squares line
through the unmasked samples restated (means, centred sums in frame order, rms residual).  The
fixture records which produced it in ``mma_source`` and ``linreg_source``.

The reference's classes are not changed; the generator only listens: a subclass of its
SingleTimeEffectDetection notes, per frame added, which STE decisions a last-digit difference in
the host fit cannot flip (|image - avg - thr| >= 1e-5 * thr), and wrappers around _evaluate and
smooth note which branch the noise level function took.  The generator asserts the branch per
scene - (a) the polynomial, (b) the bounded square root - and that at most 1 % of the pixels of
any frame fall outside the stable mask.

The inputs are the seeded scenes of tests/dark_cases.py; the fixture holds arrays only.

    python tests/golden/gen_dark_golden.py
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
import dark_cases as dc  # noqa: E402

warnings.filterwarnings('ignore')

STABLE = 1e-5
SUB = 6   # scene (b) is stored every SUB-th pixel

LINREG_STANDIN = '''
import numpy as np


def linRegressUsingMasked2dArrays(xVals, ys, badMask=None):
    """per pixel the least-squares line through the samples that are not masked
    -> ascent, offset, rms residual"""
    ys = [np.asarray(y, dtype=np.float64) for y in ys]
    shape = ys[0].shape
    good = [np.ones(shape, dtype=bool) if badMask is None else ~np.asarray(badMask[k])
            for k in range(len(ys))]
    n, sx, sy = np.zeros(shape), np.zeros(shape), np.zeros(shape)
    for k, x in enumerate(xVals):
        g = good[k]
        n[g] += 1.0
        sx[g] += float(x)
        sy[g] += ys[k][g]
    mx, my = sx / n, sy / n
    sxx, sxy = np.zeros(shape), np.zeros(shape)
    for k, x in enumerate(xVals):
        g = good[k]
        dx = float(x) - mx
        sxx[g] += (dx * dx)[g]
        sxy[g] += (dx * (ys[k] - my))[g]
    ascent = sxy / sxx
    offset = my - ascent * mx
    se = np.zeros(shape)
    for k, x in enumerate(xVals):
        g = good[k]
        r = ys[k] - (offset + ascent * float(x))
        se[g] += (r * r)[g]
    return ascent, offset, np.sqrt(se / n)
'''


def install_linreg():
    try:
        from fancytools.math.linRegressUsingMasked2dArrays import linRegressUsingMasked2dArrays  # noqa: F401
        import fancytools
        return 'fancytools %s' % getattr(fancytools, '__version__', '?')
    except ImportError:
        import fancytools.math
        d = list(fancytools.math.__path__)[0]
        assert 'ste_standins_' in d, 'the stand-in goes to the temp dir only'
        with open(os.path.join(d, 'linRegressUsingMasked2dArrays.py'), 'w') as f:
            f.write(LINREG_STANDIN)
        return 'restatement'


def main():
    if not hasattr(np, 'asfarray'):
        np.asfarray = lambda a, dtype=np.float64: np.asarray(a, dtype=dtype)
    install_shim()
    mma_source = install_standins()
    linreg_source = install_linreg()
    from imgProcessor.camera import NoiseLevelFunction as N
    from imgProcessor.camera import DarkCurrentMap as D
    from imgProcessor.features import SingleTimeEffectDetection as S

    branches, dets = [], []
    ref_evaluate, ref_smooth = N._evaluate, N.smooth

    def evaluate(x, y, weights):
        out = ref_evaluate(x, y, weights)
        if out[0] is not None:
            branches.append('sqrt')
        return out

    def smooth(x, y, weights):
        p = np.polyfit(x, y, w=weights, deg=2)
        branches.append('constant' if np.any(np.isnan(p)) else 'poly')
        return ref_smooth(x, y, weights)

    N._evaluate, N.smooth = evaluate, smooth

    class Listening(S.SingleTimeEffectDetection):
        def __init__(self, *args, **kwargs):
            self.stable = []
            dets.append(self)
            S.SingleTimeEffectDetection.__init__(self, *args, **kwargs)

        def addImage(self, image, mask=None):
            thr = np.broadcast_to(np.asarray(self.threshold, dtype=np.float64), self.noSTE.shape)
            self.stable.append(np.abs(image - self.noSTE - thr) >= STABLE * thr)
            return S.SingleTimeEffectDetection.addImage(self, image, mask)

    D.SingleTimeEffectDetection = Listening

    out = {'mma_source': np.array(mma_source), 'linreg_source': np.array(linreg_source)}
    worst = 0.0
    # ---- scene (a)
    for dtype in dc.DTYPES:
        times, frames = dc.dark_series(dtype)
        del branches[:], dets[:]
        x, avgs = D.getDarkCurrentAverages(times, [f.copy() for f in frames])
        assert avgs.dtype == np.dtype(dtype)
        groups = [t for t in sorted(set(times)) if times.count(t) > 1]
        assert len(dets) == len(groups) == len(branches) == 5, (len(dets), branches)
        assert all(b == 'poly' for b in branches), 'scene (a) must take the polynomial: %s' % branches
        offs, ascent, err = D.getLinearityFunction(x, avgs, mxIntensity=dc.MX_INTENSITY,
                                                   min_ascent=dc.MIN_ASCENT)
        p = 'a_%s_' % np.dtype(dtype).name
        out[p + 'in_sum'] = np.array([np.asarray(f, np.float64).sum() for f in frames])
        out[p + 'times'] = np.array(x, dtype=np.float64)
        out[p + 'avgs'] = avgs
        out[p + 'offset'], out[p + 'ascent'], out[p + 'error'] = offs, ascent, err
        out[p + 'branch'] = np.array(branches)
        out[p + 'thr'] = np.stack([np.broadcast_to(np.asarray(d.threshold, np.float64), avgs.shape[1:])
                                   for d in dets])
        # per exposure time: the pixels all of whose decisions are stable (a single frame: all)
        covered = np.ones(avgs.shape, dtype=bool)
        for d, t in zip(dets, groups):
            assert len(d.stable) == times.count(t) - 1
            for s in d.stable:
                worst = max(worst, 1.0 - s.mean())
            covered[x.index(t)] = np.all(d.stable, axis=0)
        out[p + 'stable'] = covered
        # what the scene is for
        n_valid = np.sum(~(avgs > dc.MX_INTENSITY), axis=0)
        assert n_valid[dc.PX_N0] == 0 and n_valid[dc.PX_N1] == 1 and n_valid[dc.BLOCK].max() == 4
        rest = np.ones(ascent.shape, dtype=bool)
        rest[dc.BAND] = False
        assert np.mean(ascent[dc.BAND] == 0) > 0.9 and np.mean(ascent[rest] == 0) < 0.1
        assert np.isnan(offs[dc.PX_N0]) and np.isnan(err[dc.PX_N1]) and ascent[dc.PX_N1] == 0
    # ---- scene (b)
    f = dc.fit_pair()
    del branches[:], dets[:]
    m = D.DarkCurrentMap([np.asarray(f[0], np.float64), np.asarray(f[1], np.float64)])
    assert branches == ['sqrt'], 'scene (b) must take the bounded square root: %s' % branches
    out['b_in_sum'] = np.array([np.asarray(a, np.float64).sum() for a in f])
    out['b_branch'] = np.array(branches)
    out['b_thr'] = np.asarray(dets[0].threshold, np.float64)[::SUB, ::SUB]
    out['b_map2'] = m.map()[::SUB, ::SUB].copy()
    m.addImg(f[2])
    out['b_map3'] = m.map()[::SUB, ::SUB].copy()
    out['b_stable'] = np.stack(dets[0].stable)[:, ::SUB, ::SUB]
    for s in dets[0].stable:
        worst = max(worst, 1.0 - s.mean())
    # a condition of the tests that use the stable mask, not a measurement
    assert worst <= 0.01, 'a frame has %.2f %% of its pixels within 1e-5 of the threshold' % (100 * worst)
    out['unstable_worst'] = np.array(worst)
    path = os.path.join(HERE, 'dark.npz')
    np.savez_compressed(path, **out)
    print('wrote %s (%d bytes, %d arrays; running mean: %s, regression: %s; worst unstable fraction %.2e)'
          % (path, os.path.getsize(path), len(out), mma_source, linreg_source, worst))


if __name__ == '__main__':
    main()
