#!/usr/bin/env python3
"""Generate tests/golden/fn2d.npz: the Kang-Weiss and angle-of-view models and the flat-field
post-processing that fits them, as the reference computes them (equations/vignetting.py,
equations/angleOfView.py, camera/flatField/postprocessing/function.py).  Runs only where the reference
source exists.

The three reference files are executed unchanged, loaded by path.  function.py imports
fancytools.fit.fit2dArrayToFn, which is not installed: the generator supplies a stand-in of its own - a
least-squares fit of fn((rows, cols), *params) to the valid pixels by scipy.optimize.curve_fit from the
guess, rebuilt on the frame's index grid or at fn((yy, xx), *params) for an outgrid - and records what
curve_fit returned.

The generator asserts its own conditions on the seeded inputs of tests/fn2d_cases.py: curve_fit
converged, the scaled J^T J at the solution has a condition number below COND_MAX, and no fitted centre
lies within CENTRE_MARGIN of a pixel when alpha != 0.  The fixture holds arrays only.

    python tests/golden/gen_fn2d_golden.py [other/path/fn2d.npz]
"""
import importlib.util
import math
import os
import sys
import types
import warnings

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
sys.path.insert(0, os.path.dirname(HERE))
from gen_golden import REF  # noqa: E402
import fn2d_cases as fc  # noqa: E402

warnings.filterwarnings('ignore')


def load(name, rel):
    spec = importlib.util.spec_from_file_location(name, os.path.join(REF, 'imgProcessor', rel))
    mod = importlib.util.module_from_spec(spec)
    sys.modules[name] = mod
    spec.loader.exec_module(mod)
    return mod


def reference():
    """-> (vignetting module, angleOfView module, function module, the stand-in's log)"""
    from scipy.optimize import curve_fit
    log = []

    def fit2dArrayToFn(arr, fn, mask=None, down_scale_factor=None, output_shape=None, guess=None, outgrid=None):
        assert down_scale_factor in (None, 1) and output_shape is None
        valid = np.ones(arr.shape, bool) if mask is None else mask
        xy = np.where(valid)
        z = arr[valid]
        p, _, info, msg, ier = curve_fit(fn, xy, z, p0=guess, full_output=True)
        assert ier in (1, 2, 3, 4), msg
        log.append((p, math.fsum((fn(xy, *p) - z.astype(np.float64)) ** 2)))
        if outgrid is not None:
            return fn((outgrid[0], outgrid[1]), *p), p
        return np.fromfunction(lambda x, y: fn((x, y), *p), arr.shape), p

    for pkg in ('imgProcessor', 'imgProcessor.equations', 'fancytools', 'fancytools.fit'):
        sys.modules.setdefault(pkg, types.ModuleType(pkg))
    stand_in = types.ModuleType('fancytools.fit.fit2dArrayToFn')
    stand_in.fit2dArrayToFn = fit2dArrayToFn
    sys.modules['fancytools.fit.fit2dArrayToFn'] = stand_in
    V = load('imgProcessor.equations.vignetting', 'equations/vignetting.py')
    A = load('imgProcessor.equations.angleOfView', 'equations/angleOfView.py')
    F = load('imgProcessor_function', 'camera/flatField/postprocessing/function.py')
    return V, A, F, log


def scaled_cond(J):
    JtJ = J.T @ J
    s = np.sqrt(np.diag(JtJ))
    return np.linalg.cond(JtJ / s[:, None] / s[None, :])


def jacobian(fn, xy, p):
    """central differences: only the condition number is read from it"""
    cols = []
    for i in range(len(p)):
        h = 1e-6 * max(abs(p[i]), 1e-3)
        lo, hi = np.array(p, float), np.array(p, float)
        lo[i] -= h
        hi[i] += h
        cols.append((fn(xy, *hi) - fn(xy, *lo)) / (2 * h))
    return np.stack(cols, 1)


def main(path=os.path.join(HERE, 'fn2d.npz')):
    V, A, F, log = reference()
    out = {}
    X, Y = fc.index_grid(fc.VALUE_SHAPE)
    for k, (f, alpha, cx, cy) in enumerate(fc.KW_VALUE_PARAMS):
        out['kw_value_%d' % k] = V.vignetting((X, Y), f=f, alpha=alpha, cx=cx, cy=cy)
    for k, a in enumerate(fc.AOV_VALUE_PARAMS):
        out['aov_value_%d' % k] = A.angleOfView((X, Y), fc.VALUE_SHAPE, a=a)
    out['guess_48x64'] = np.array(V.guessVignettingParam((48, 64)), dtype=np.float64)
    out['tilt_factor'] = V.tiltFactor((X, Y), 120.0, 0.2, 0.3)
    out['kw_value_tilted'] = V.vignetting((X, Y), f=120.0, alpha=1e-3, rot=0.3, tilt=0.2, cx=14.5, cy=30.25)

    for name in fc.PINNED:
        img, mask, model = fc.scene(name)
        shape = img.shape
        if model == 'KW':
            kw = {}

            def fn(xy, f, alpha, cx, cy):
                return V.vignetting(xy, f=f, alpha=alpha, cx=cx, cy=cy)
        else:
            def fn(xy, a):
                return A.angleOfView(xy, shape, a=a)
            # the lambdas of camera/flatField/postProcessing.py:66-74, `method.shape` read as arr.shape
            kw = dict(fn=fn, guess=(0.01), down_scale_factor=1)
        for what, args in (('replace', dict(replace_all=True)), ('repair', dict(replace_all=False)),
                           ('outgrid', dict(outgrid=fc.outgrid(shape)))):
            if what == 'repair' and mask is None:
                continue                      # function.py:17-19: no mask is a replace
            del log[:]
            m = None if mask is None else mask.copy()
            got = F.function(img.copy(), m, **args, **kw)
            (p, S), = log
            assert np.isfinite(got).all(), (name, what)
            out['%s_%s' % (name, what)] = np.asarray(got, dtype=np.float64)
        valid = np.ones(shape, bool) if mask is None else ~mask
        cond = scaled_cond(jacobian(fn, np.where(valid), p))
        assert cond < fc.COND_MAX, (name, cond)
        if model == 'KW' and p[1] != 0:
            off = np.abs(np.array(p[2:]) - np.round(p[2:]))
            assert max(off) > fc.CENTRE_MARGIN or not (0 <= round(p[2]) < shape[0] and 0 <= round(p[3]) < shape[1]), \
                (name, p)
        out[name + '_params'] = np.array(p, dtype=np.float64)
        out[name + '_S'] = np.float64(S)
        out[name + '_cond'] = np.float64(cond)
        print('%-18s params %s  S %.6g  cond %.3g' % (name, np.array2string(np.array(p), precision=6), S, cond))
    np.savez_compressed(path, **out)
    print('wrote %s (%d arrays, %d bytes)' % (path, len(out), os.path.getsize(path)))


if __name__ == '__main__':
    main(*sys.argv[1:])
