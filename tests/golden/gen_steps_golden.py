#!/usr/bin/env python3
"""Generate tests/golden/steps.npz: the flat field from discrete steps as the reference computes it
(camera/flatField/vignettingFromDiscreteSteps.py with array/subCell2D.py, interpolate/polyfit2d.py and
interpolate/offsetMeshgrid.py).  Runs only where the reference source exists.

The four reference files are executed unchanged, loaded by path.  What they import and this machine
lacks gets import-only stand-ins: cv2 (an empty module), imgIO.imread (the array itself; a float64 copy
for dtype=float), equations.angleOfView and camera.flatField.interpolationMethods (names that are
never called: the scenes run 'POLY replace').  The generator only listens: subCell2DFnArray is wrapped
to record the grid of every frame, and the module's np.nanmean to count the iterations and to record
every deviation.

Asserted here, as conditions on the seeded scenes of tests/steps_cases.py:
  * every scene converges below max_iter;
  * no deviation lies within 1e-6 relative of max_dev, so a last-digit difference in it cannot change
    the iteration count;
  * every branch of _DeviceAndGridSlice.iter() that does not raise occurs in some scene;
  * the restatement (tests/steps_ref.py) on the reference's own grids gives the reference's ff,
    avgobj and pointdensity bit for bit and its iteration count.
Printed: the largest relative difference between the reference's ff / avgobj and the restatement's with
its own grids (cell sums through math.fsum instead of numpy's pairwise sums) - the MEASURED_REL of
tests/steps_cases.py.

    python tests/golden/gen_steps_golden.py [other/path/steps.npz]
"""
import importlib.util
import os
import sys
import types
import warnings

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
sys.path.insert(0, os.path.dirname(os.path.dirname(HERE)))
from gen_golden import REF  # noqa: E402
from tests import steps_cases as sc  # noqa: E402
from tests import steps_ref as ref  # noqa: E402

warnings.filterwarnings('ignore')


def load(name, rel):
    spec = importlib.util.spec_from_file_location(name, os.path.join(REF, 'imgProcessor', rel))
    mod = importlib.util.module_from_spec(spec)
    sys.modules[name] = mod
    spec.loader.exec_module(mod)
    return mod


class ListeningNumpy(object):
    """numpy with a nanmean that reports: the module under test sees it as `np`"""

    def __init__(self, log):
        self._log = log

    def __getattr__(self, name):
        return getattr(np, name)

    def nanmean(self, a, *args, **kw):
        out = np.nanmean(a, *args, **kw)
        self._log['nanmean'].append(None if (args or kw) else float(out))
        return out


def reference():
    """-> (the module, the listeners' log)"""
    def stub(name, **attrs):
        m = sys.modules.setdefault(name, types.ModuleType(name))
        for k, v in attrs.items():
            setattr(m, k, v)
        return m

    for pkg in ('imgProcessor', 'imgProcessor.array', 'imgProcessor.interpolate', 'imgProcessor.camera',
                'imgProcessor.camera.flatField', 'imgProcessor.equations'):
        stub(pkg)
    stub('cv2')

    def imread(img, dtype=None):
        return img if dtype is None else np.array(img, dtype=dtype)

    def never(*a, **k):
        raise AssertionError('a stand-in was called')

    stub('imgProcessor.imgIO', imread=imread)
    stub('imgProcessor.equations.angleOfView', angleOfView=never)
    stub('imgProcessor.camera.flatField.interpolationMethods', function=never)
    load('imgProcessor.array.subCell2D', 'array/subCell2D.py')
    load('imgProcessor.interpolate.polyfit2d', 'interpolate/polyfit2d.py')
    load('imgProcessor.interpolate.offsetMeshgrid', 'interpolate/offsetMeshgrid.py')
    V = load('imgProcessor_vignettingFromDiscreteSteps', 'camera/flatField/vignettingFromDiscreteSteps.py')
    log = {'grids': [], 'nanmean': [], 'branches': set()}
    fn_array = V.subCell2DFnArray

    def subCell2DFnArray(*a, **k):
        g = fn_array(*a, **k)
        log['grids'].append(np.array(g))
        return g

    it = V._DeviceAndGridSlice.iter

    def iter_(self):
        for i in range(self.n):
            p0, p1 = self.cell_positions[i]
            log['branches'].add((0, -1 < p0, p0 + self.n0 <= self.g0))
            log['branches'].add((1, -1 < p1, p1 + self.n1 <= self.g1))
        return it(self)

    V.subCell2DFnArray = subCell2DFnArray
    V._DeviceAndGridSlice.iter = iter_
    V.np = ListeningNumpy(log)
    return V, log


def rel(a, b):
    ok = ~np.isnan(b)
    assert np.array_equal(np.isnan(a), ~ok)
    return float(np.max(np.abs(a[ok] - b[ok]) / np.abs(b[ok]))) if ok.any() else 0.0


def main(path=os.path.join(HERE, 'steps.npz')):
    V, log = reference()
    out, worst, branches = {}, 0.0, set()
    for name, s in sc.all_scenes().items():
        log['grids'], log['nanmean'] = [], []
        log['branches'].clear()
        if 'corners' in s:
            positions = V.positionsFromTopLeftCorner(s['corners'], s['cell_size'])
        else:
            positions = s['positions']
        assert positions[0] == s['positions'][0] and list(positions[1]) == list(s['positions'][1]) \
            and tuple(positions[2]) == tuple(s['positions'][2]), name
        frames = s['frames']
        kw = dict(s['kw'])
        ff, _, avgobj, density = V.vignettingFromDiscreteSteps(
            [f.copy() for f in frames], s['n_cells_device'], positions, postprocessing_method='POLY replace',
            max_iter=sc.MAX_ITER, max_dev=sc.MAX_DEV, **{k: (v.copy() if hasattr(v, 'copy') else v)
                                                           for k, v in kw.items()})
        branches |= log['branches']
        devs = [v ** 0.5 for v in log['nanmean'] if v is not None]
        iters = len(devs)
        assert len(log['nanmean']) == 1 + 3 * iters, name
        assert iters < sc.MAX_ITER and devs[-1] < sc.MAX_DEV, (name, iters, devs[-1])
        assert all(abs(d - sc.MAX_DEV) > 1e-6 * sc.MAX_DEV for d in devs), (name, devs)
        grid = np.stack(log['grids'])
        n1, n0 = s['n_cells_device']
        # the restatement on the reference's grids: bit for bit
        bgv = None if 'bg_img' in kw else kw.get('bg_value', 0)
        r_ff, r_obj, r_den, r_it, r_devs = ref.separate(grid, (n0, n1), positions[1], bgv, sc.MAX_ITER, sc.MAX_DEV)
        assert np.array_equal(r_ff, ff, equal_nan=True) and np.array_equal(r_obj, avgobj, equal_nan=True), name
        assert np.array_equal(r_den, density) and r_it == iters, (name, r_it, iters)
        # the restatement with its own grids: the measured difference
        m = ref.run(frames, s['n_cells_device'], positions, kw.get('bg_img'), kw.get('bg_value', 0), kw.get('thresh'),
                    sc.MAX_ITER, sc.MAX_DEV)
        assert np.array_equal(np.isnan(m[0]), np.isnan(grid)) and m[4] == iters, name
        d = max(rel(m[1], ff), rel(m[2], avgobj))
        worst = max(worst, d)
        out[name + '_in_sum'] = np.array([np.asarray(f, np.float64).sum() for f in frames])
        out[name + '_grid'] = grid
        out[name + '_ff'] = ff
        out[name + '_avgobj'] = avgobj
        out[name + '_pointdensity'] = np.asarray(density)
        out[name + '_iterations'] = np.array(iters)
        print('%-16s %2d frames, grid %s, %2d iterations, last dev %.3g, NaN cells %d, grids vs fsum %.3g, '
              'ff / avgobj vs fsum %.3g' % (name, len(frames), grid.shape[1:], iters, devs[-1],
                                            int(np.isnan(grid).sum()), rel(m[0], grid), d))
    want = {(0, True, True), (0, False, True), (0, True, False), (0, False, False),
            (1, True, True), (1, False, True), (1, True, False)}
    assert branches == want, sorted(want ^ branches)
    np.savez_compressed(path, **out)
    size = os.path.getsize(path)
    assert size <= 100 * 1024, size
    print('MEASURED_REL = %.3g' % worst)
    print('wrote %s (%d arrays, %d bytes)' % (path, len(out), size))


if __name__ == '__main__':
    main(*sys.argv[1:])
