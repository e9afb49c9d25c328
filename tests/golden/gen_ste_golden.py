#!/usr/bin/env python3
"""Generate tests/golden/ste.npz: single-time-effect removal and removeSinglePixels as the
reference computes them (features/SingleTimeEffectDetection.py, filters/removeSinglePixels.py,
camera/NoiseLevelFunction.py boundedFunction).  Runs only where the reference source exists.

The reference runs unchanged under three throw-away stand-ins written to a temp dir (never
committed):
  - the identity ``numba`` shim of gen_golden.py (removeSinglePixels is plain Python under @jit);
  - a constants-only ``cv2``: imgIO.imread on an ndarray calls no cv2 function;
  - ``fancytools.math.MaskedMovingAverage`` when the real one cannot be imported: the running mean
    restated (each accepted sample counted once, incremental mean in frame order).  The fixture
    records which one produced it in ``mma_source``.

The fixture holds arrays only.

    python tests/golden/gen_ste_golden.py
"""
import os
import sys
import tempfile
import warnings

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
from gen_golden import install_shim  # noqa: E402

warnings.filterwarnings('ignore')

H, W = 24, 40
SCALE = {np.uint8: 1.0, np.uint16: 16.0, np.float32: 16.0, np.float64: 16.0}

MMA_STANDIN = '''
import numpy as np


class MaskedMovingAverage(object):
    def __init__(self, shape, calcVariance=False, dtype=float):
        self.avg = np.zeros(shape, dtype=dtype)
        self.n = np.zeros(shape, dtype=int)

    def update(self, arr, mask=None):
        if mask is None:
            mask = np.ones(self.avg.shape, dtype=bool)
        self.n[mask] += 1
        n = self.n[mask]
        a = self.avg[mask]
        x = np.asarray(arr)[mask].astype(np.float64)
        self.avg[mask] = np.where(n == 1, x, a + (x - a) / n)
'''


def install_standins():
    d = tempfile.mkdtemp(prefix='ste_standins_')
    with open(os.path.join(d, 'cv2.py'), 'w') as f:
        f.write('IMREAD_GRAYSCALE = 0\nIMREAD_COLOR = 1\nIMREAD_ANYCOLOR = 4\n'
                'IMREAD_ANYDEPTH = 2\n')
    try:
        import fancytools  # noqa: F401
        from fancytools.math.MaskedMovingAverage import MaskedMovingAverage  # noqa: F401
        source = 'fancytools %s' % getattr(fancytools, '__version__', '?')
    except ImportError:
        os.makedirs(os.path.join(d, 'fancytools', 'math'))
        open(os.path.join(d, 'fancytools', '__init__.py'), 'w').close()
        open(os.path.join(d, 'fancytools', 'math', '__init__.py'), 'w').close()
        with open(os.path.join(d, 'fancytools', 'math', 'MaskedMovingAverage.py'), 'w') as f:
            f.write(MMA_STANDIN)
        source = 'restatement'
    sys.path.append(d)
    return source


def frames_for(dtype, n, seed):
    """a gradient scene with noise, noise outliers, planted hits and (float) NaNs"""
    rng = np.random.default_rng(seed)
    sc = SCALE[dtype]
    y, x = np.mgrid[0:H, 0:W].astype(np.float64)
    base = (10 + 210 * x / (W - 1) + 5 * np.sin(y / 3)) * sc
    out = []
    for k in range(n):
        f = base + 2 * sc * rng.standard_normal((H, W))
        f += (rng.random((H, W)) < 0.03) * rng.uniform(4, 14, (H, W)) * sc   # near the threshold
        out.append(f)
    out = np.stack(out)
    hit = 120 * sc
    plants = [[(5, 7)], [(10, 12), (10, 13)], [(3, 30), (4, 30)], [(15, 20), (16, 21)],
              [(0, 0), (0, 1), (1, 0), (1, 1)], [(H - 1, 18), (H - 1, 19)], [(12, W - 1), (13, W - 1)],
              [(H - 1, W - 1), (H - 2, W - 2)], [(0, 34)], [(7, 0), (8, 0), (8, 1)]]
    for j, pts in enumerate(plants):
        k = int(rng.integers(0, n))
        for (py, px) in pts:
            out[k, py, px] += hit
    if np.dtype(dtype).kind == 'f':
        for k in range(n):
            out[k, rng.integers(0, H, 2), rng.integers(0, W, 2)] = np.nan
        return out.astype(dtype)
    info = np.iinfo(dtype)
    return np.clip(np.round(out), 0, info.max).astype(dtype)


def nlf_for(i, dtype):
    sc = SCALE[dtype]
    ay = 2 * np.sqrt(sc) / 10.7
    return [(0.5 * sc, 0.0, ay),               # sqrt branch
            (1.0 * sc, 100.0 * sc, ay),        # x < ax on the left half: NaN -> 0 -> minY
            (3.0 * sc, 0.0, 0.3 * ay)][i % 3]  # minY dominates


def main():
    install_shim()
    source = install_standins()
    from imgProcessor.features.SingleTimeEffectDetection import SingleTimeEffectDetection
    from imgProcessor.camera.NoiseLevelFunction import boundedFunction
    from imgProcessor.filters.removeSinglePixels import removeSinglePixels

    out = {'mma_source': np.array(source)}
    i = 0
    for dtype in (np.uint8, np.uint16, np.float32, np.float64):
        for n in (2, 3, 5):
            fr = frames_for(dtype, n + 1, 1000 + i)
            stack, add = fr[:n], fr[n]
            tri = nlf_for(i, dtype)
            nstd = (4, 2.5)[i % 2]
            rng = np.random.default_rng(2000 + i)
            amask = rng.random((H, W)) < 0.8
            s = SingleTimeEffectDetection(list(stack),
                                          noise_level_function=lambda x, t=tri: boundedFunction(x, *t),
                                          nStd=nstd, save_ste_indices=True)
            p = 'c%d_' % i
            out[p + 'frames'] = stack
            out[p + 'nlf'] = np.array(tri)
            out[p + 'nstd'] = np.array(nstd, dtype=np.float64)
            out[p + 'thr'] = np.array(s.threshold, dtype=np.float64)
            out[p + 'noSTE'] = s.noSTE.copy()
            out[p + 'mask_clean'] = s.mask_clean.copy()
            out[p + 'mask_ste'] = s.mask_STE.copy()
            s.addImage(add, amask)
            out[p + 'add'] = add
            out[p + 'add_mask'] = amask
            out[p + 'noSTE2'] = s.noSTE.copy()
            out[p + 'mask_clean2'] = s.mask_clean.copy()
            out[p + 'mask_ste2'] = s.mask_STE.copy()
            i += 1
    out['n_cases'] = np.array(i)

    rng = np.random.default_rng(7)
    shapes = [((37, 53), 0.02), ((37, 53), 0.2), ((37, 53), 0.6), ((1, 57), 0.2), ((1, 57), 0.6),
              ((41, 1), 0.2), ((41, 1), 0.6), ((1, 1), 1.0)]
    for j, (shape, dens) in enumerate(shapes):
        a = rng.random(shape) < dens
        b = a.copy()
        removeSinglePixels(b)
        out['rsp%d_in' % j] = a
        out['rsp%d_out' % j] = b
    out['n_rsp'] = np.array(len(shapes))
    path = os.path.join(HERE, 'ste.npz')
    np.savez_compressed(path, **out)
    print('wrote %s (%d bytes, running mean: %s)' % (path, os.path.getsize(path), source))


if __name__ == '__main__':
    main()
