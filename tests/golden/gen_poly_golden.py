#!/usr/bin/env python3
"""Generate tests/golden/poly.npz: polyfit2dGrid and the POLY repair loop as the reference computes
them (interpolate/polyfit2d.py, camera/flatField/postprocessing/polynomial.py).  Runs only where the
reference source exists.

The two reference files are executed unchanged, loaded by path (their packages' __init__ import half
of the reference).  The generator only listens: polyfit2d is wrapped to record the condition number of
the raw-monomial design matrix of every fit, _highGrad to record how far every |laplace| is from its
threshold and the size of the mask, and the module's print to record the residuum it reports.

The reference is a usable yardstick only while that design matrix is well conditioned: the generator
asserts cond <= COND_MAX (5e6) for every fit of every case, which keeps lstsq's own error near
cond * 2.2e-16 ~ 1e-9 on values in [0, 1], and asserts that no decision of a loop is closer than 1e-9 to
its threshold: no ||laplace| - 0.01| and no |residuum - 1e-5|.  These are conditions on the seeded
inputs of tests/poly_cases.py; the fixture holds arrays only.

    python tests/golden/gen_poly_golden.py [other/path/poly.npz]
"""
import importlib.util
import itertools
import os
import sys
import types
import warnings

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
sys.path.insert(0, os.path.dirname(HERE))
from gen_golden import REF  # noqa: E402
import poly_cases as pc  # noqa: E402

warnings.filterwarnings('ignore')


def load(name, rel):
    spec = importlib.util.spec_from_file_location(name, os.path.join(REF, 'imgProcessor', rel))
    mod = importlib.util.module_from_spec(spec)
    sys.modules[name] = mod
    spec.loader.exec_module(mod)
    return mod


def reference():
    """-> (polyfit2d module, polynomial module, the listeners' log)"""
    import scipy.ndimage
    for pkg in ('imgProcessor', 'imgProcessor.interpolate'):
        sys.modules.setdefault(pkg, types.ModuleType(pkg))
    try:
        import scipy.ndimage.filters  # noqa: F401
    except ImportError:
        sys.modules['scipy.ndimage.filters'] = scipy.ndimage
    P = load('imgProcessor.interpolate.polyfit2d', 'interpolate/polyfit2d.py')
    Q = load('imgProcessor_polynomial', 'camera/flatField/postprocessing/polynomial.py')
    log = {'cond': [], 'res': [], 'm': [], 'lap_margin': []}
    fit = P.polyfit2d

    def polyfit2d(x, y, z, order=3):
        x64, y64 = np.asarray(x, dtype=np.float64), np.asarray(y, dtype=np.float64)
        G = np.stack([x64 ** i * y64 ** j for i, j in itertools.product(range(order + 1), repeat=2)], 1)
        log['cond'].append(np.linalg.cond(G))
        return fit(x, y, z, order)

    high = Q._highGrad

    def _highGrad(arr):
        lap = scipy.ndimage.laplace(arr, mode='reflect')
        log['lap_margin'].append(np.abs(np.abs(lap) - pc.LAP_THRESHOLD).min())
        mask = high(arr)
        log['m'].append(int(mask.sum()))
        return mask

    def listen(*a):
        assert a[0] == 'residuum: '
        log['res'].append(float(a[1]))

    P.polyfit2d, Q._highGrad, Q.print = polyfit2d, _highGrad, listen
    return P, Q, log


def main(path=os.path.join(HERE, 'poly.npz')):
    P, Q, log = reference()
    out = {}

    def reset():
        for v in log.values():
            del v[:]

    for name, (arr, mask, kw) in pc.fit_cases().items():
        reset()
        got = P.polyfit2dGrid(arr.copy(), None if mask is None else mask.copy(), **kw)
        assert len(log['cond']) == 1 and log['cond'][0] <= pc.COND_MAX, (name, log['cond'])
        assert np.isfinite(got).all(), name
        out[name + '_out'] = got
        out[name + '_cond'] = np.array(log['cond'])
        print('%-18s cond %.3g' % (name, log['cond'][0]))

    for name, (img, mask, kw, why) in pc.loop_cases().items():
        reset()
        got = Q.polynomial(img.copy(), mask.copy(), **kw)
        res, m = log['res'], log['m']
        assert max(log['cond']) <= pc.COND_MAX, (name, log['cond'])
        assert all(abs(r - pc.MAX_DEV) > pc.STABLE for r in res), (name, res)
        assert all(g > pc.STABLE for g in log['lap_margin']), (name, log['lap_margin'])
        if res[-1] < pc.MAX_DEV:
            took = 'res'
        elif m[-1] == (m[-2] if len(m) > 1 else 0):
            took = 'same'
        elif m[-1] == img.size:
            took = 'all'
        else:
            took = 'max_iter'
        assert took == why, (name, took, res, m)
        if why == 'res':
            assert len(res) >= 3, (name, res)
        out[name + '_out'] = got
        out[name + '_res'] = np.array(res)
        out[name + '_m'] = np.array(m, dtype=np.int64)
        out[name + '_cond'] = np.array(log['cond'])
        print('%-18s exit %-5s iterations %d, cond <= %.3g, residua %s, m %s, |lap| margin >= %.2g'
              % (name, took, len(res), max(log['cond']), ['%.3g' % r for r in res], m,
                 min(log['lap_margin'] or [np.inf])))
    np.savez_compressed(path, **out)
    print('wrote %s (%d arrays, %d bytes)' % (path, len(out), os.path.getsize(path)))


if __name__ == '__main__':
    main(*sys.argv[1:])
