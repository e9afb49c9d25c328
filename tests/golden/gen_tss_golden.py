#!/usr/bin/env python3
"""Generate tests/golden/tss.npz: temporal signal stability as the reference computes it
(uncertainty/temporalSignalStability.py over filters/maskedFilter.py and scipy.ndimage).  Runs only
where the reference source exists.

The reference runs unchanged under the throw-away stand-ins of gen_ste_golden.py (numba shim,
constants-only cv2).  One more stand-in is written to the temp dir (never committed) when the real
one cannot be imported: ``fancytools.math.linRegressUsingMasked2dArrays`` with the ``calcError``
argument the reference passes - the per-pixel least-squares line restated as in
gen_dark_golden.py (means, centred sums in frame order, rms residual).  The fixture records which
produced it in ``linreg_source``.

The reference's function is not changed; the generator only listens: a wrapper around its
_calcAvgLen notes the event cube it is handed and the raw event length it returns.  Beside them
the fixture records the stable-decision mask: the voxels whose |median| - c is not within 1e-9
(relative) of zero, which a last-digit difference of another regression cannot flip.  The
generator asserts that at most 1 % of the voxels fall outside it.

The inputs are the seeded scenes of tests/tss_cases.py (demo, demo16); the fixture holds arrays only.

    python tests/golden/gen_tss_golden.py
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
import tss_cases as tc  # noqa: E402

warnings.filterwarnings('ignore')

STABLE = 1e-9

LINREG_STANDIN = '''
import numpy as np


def linRegressUsingMasked2dArrays(xVals, ys, badMask=None, calcError=False):
    """per pixel the least-squares line through the samples that are not masked
    -> ascent, offset[, rms residual]"""
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
    if not calcError:
        return ascent, offset
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
    install_shim()
    install_standins()
    linreg_source = install_linreg()
    from scipy.ndimage import median_filter
    from imgProcessor.uncertainty import temporalSignalStability as mod

    heard = {}
    ref_avg_len = mod._calcAvgLen

    def listening(arr, out):
        heard['events'] = np.array(arr, dtype=bool)
        res = ref_avg_len(arr, out)
        heard['raw'] = np.array(res, dtype=np.float64)
        return res

    mod._calcAvgLen = listening

    out = {'linreg_source': np.array(linreg_source)}
    worst = 0.0
    for name, (times, frames) in (('demo', tc.demo()), ('demo16', tc.demo16())):
        heard.clear()
        error, avlen, ascent, offset = mod.temporalSignalStability(frames.copy(), times)
        p = name + '_'
        out[p + 'in_sum'] = np.array([np.asarray(f, np.float64).sum() for f in frames])
        out[p + 'times'] = np.asarray(times, dtype=np.float64)
        out[p + 'error'], out[p + 'ascent'], out[p + 'offset'] = error, ascent, offset
        out[p + 'avlen'] = avlen
        out[p + 'events'] = np.packbits(heard['events'], axis=None)
        out[p + 'raw'] = heard['raw']
        # the stable decisions, from the fixture's own fit
        diff = np.stack([f.astype(np.float64) - (offset + t * ascent) for f, t in zip(frames, times)])
        med = np.abs(median_filter(diff, 5))
        c = 0.5 * error[None]
        assert np.array_equal(med > c, heard['events']), 'the restated median decides otherwise'
        stable = np.abs(med - c) > STABLE * c
        out[p + 'stable'] = np.packbits(stable, axis=None)
        worst = max(worst, 1.0 - stable.mean())
        # what the scenes are for
        assert heard['events'].any() and not heard['events'].all()
        assert (avlen > 0).any() and (avlen == 0).any(), name
    # a condition of the tests that use the stable mask, not a measurement
    assert worst <= 0.01, '%.2f %% of the voxels lie within 1e-9 of the threshold' % (100 * worst)
    out['unstable_worst'] = np.array(worst)
    path = os.path.join(HERE, 'tss.npz')
    np.savez_compressed(path, **out)
    print('wrote %s (%d bytes, %d arrays; regression: %s; worst unstable fraction %.2e)'
          % (path, os.path.getsize(path), len(out), linreg_source, worst))


if __name__ == '__main__':
    main()
