"""GPU: the flat field from discrete steps (csrc/steps.hip, ops_steps.py,
camera/flatField/vignettingFromDiscreteSteps.py) against the numpy restatement (tests/steps_ref.py) and
the reference's own results (tests/golden/steps.npz).

cell_means against the restatement's exactly rounded sums (math.fsum): the NaN pattern exact, every value
within 1e-12 * mean|x| of its cell - the kernel's sum is a tree over at most 2^24 terms with a serial run of
at most 32 per lane, which errs by about 1e-14 of mean|x|; the factor of 100 above it is the tolerance of
the NLF moments too - and identical bits on a second call.  steps_separate is correctly rounded IEEE
arithmetic in numpy's order: bit for bit.  offset_meshgrid bit for bit.  The whole routine against the
fixture within steps_cases.ROUTINE_TOL, which the fixture's generator measured.
"""
import importlib

import numpy as np
import pytest

from .conftest import load_golden
from . import steps_cases as sc
from . import steps_ref as ref
from .test_cpu_dark import same
from .test_gpu_dark import ERR_BAD_ARG, ERR_UNSUPPORTED, GUARD, padded

pytestmark = pytest.mark.gpu

CELL_TOL = 1e-12


@pytest.fixture(scope='module')
def ctx():
    import imgprocessor_amd
    return imgprocessor_amd.default_context(0)


@pytest.fixture(scope='module')
def g():
    return load_golden('steps.npz')


@pytest.fixture(scope='module')
def scenes():
    return sc.all_scenes()


def _ops():
    from imgprocessor_amd import ops
    return ops


def V():
    return importlib.import_module('imgprocessor_amd.camera.flatField.vignettingFromDiscreteSteps')


def _host(a):
    return a if isinstance(a, np.ndarray) else a.get()


def check_cells(got, frames, re, ce, thresh, bg, what):
    want = ref.cell_means(frames, re, ce, thresh, bg)
    scale = ref.cell_scale(frames, re, ce, thresh, bg)
    assert got.dtype == np.float64 and got.shape == want.shape, what
    assert np.array_equal(np.isnan(got), np.isnan(want)), what
    ok = ~np.isnan(want)
    err = np.abs(got[ok] - want[ok])
    print('%s: %d of %d cells, largest error / mean|x| %.3g' % (what, ok.sum(), ok.size,
                                                               (err / scale[ok]).max() if ok.any() else 0))
    assert np.all(err <= CELL_TOL * scale[ok]), what
    return want


CELL_CASES = sc.cell_cases()


@pytest.mark.parametrize('name', sorted(CELL_CASES))
def test_cell_means(ctx, name):
    ops = _ops()
    frames, re, ce, thresh, bg = CELL_CASES[name]
    got = ops.cell_means(frames, re, ce, thresh, bg=bg, ctx=ctx)
    want = check_cells(got, frames, re, ce, thresh, bg, name)
    assert same(ops.cell_means(frames, re, ce, thresh, bg=bg, ctx=ctx), got), 'a second call differs'
    nan, n = np.isnan(want), want.size
    if name == 'frame_1x1':
        assert got.tolist() == [[[7.0]]]
    if name == 'cells_1px':
        assert 0 < nan.sum() < n and same(got[~nan], frames.astype(np.float64)[~nan])
    if name in ('one_cell', 'wide_offset'):
        assert max(np.diff(ce)) > sc.CHUNK_COLS and not nan.all()
    if name == 'tall_70':
        assert max(np.diff(re)) > 2 * sc.SEG_ROWS and not nan.any()
    if name == 'outside':
        empty = (np.diff(re) == 0)[:, None] | (np.diff(ce) == 0)[None]
        assert empty[0, 0] and empty[-1, -1] and nan[:, empty].all() and not nan[:, ~empty].all()
        assert re[0] == 0 and re[-1] == 60 and ce[0] == 0 and ce[-1] == 84
    if name == 'majority':
        assert got[0, 0, 0] == 9.0 and np.isnan(got[0, 0, 1])
    if name == 'on_thresh':
        assert got[0, 0, 0] == 1.5 and np.isnan(got[0, 0, 1])
    if name.startswith('nan_'):
        assert np.isnan(frames).any() and (name != 'nan_f32' or 0 < nan.sum()) and nan.sum() < n / 2
    if name == 'n64':
        assert got.shape[0] == 64


@pytest.mark.parametrize('dtype', sc.ALL_DTYPES, ids=lambda d: np.dtype(d).name)
def test_cell_means_types(ctx, dtype):
    ops = _ops()
    k = sc.ALL_DTYPES.index(dtype)
    for bg_dtype in (None, sc.ALL_DTYPES[(k + 1) % 4], sc.ALL_DTYPES[(k + 2) % 4]):
        frames, re, ce, thresh, bg = sc.dtype_case(dtype, bg_dtype)
        assert frames.dtype == dtype and (bg is None or bg.dtype == bg_dtype)
        got = ops.cell_means(frames, re, ce, thresh, bg=bg, ctx=ctx)
        want = check_cells(got, frames, re, ce, thresh, bg, '%s - %s' % (np.dtype(dtype).name, bg_dtype))
        assert 0 < np.isnan(want).sum() < want.size
        # N = 1; a list of device frames with a device background
        one = ops.cell_means(frames[:1], re, ce, thresh, bg=bg, ctx=ctx)
        assert same(one, got[:1])
        d = ops.cell_means([ctx.to_device(f) for f in frames], re, ce, thresh,
                           bg=None if bg is None else ctx.to_device(bg))
        assert not isinstance(d, np.ndarray) and same(d.get(), got)


def test_cell_means_pitched_and_refusals(ctx):
    from imgprocessor_amd import DeviceArray
    frames, re, ce, thresh, bg = sc.dtype_case(np.uint16, np.float32)
    n, h, w = frames.shape
    re, ce = np.ascontiguousarray(re, np.int32), np.ascontiguousarray(ce, np.int32)
    g0, g1 = len(re) - 1, len(ce) - 1
    want = _ops().cell_means(frames, re, ce, thresh, bg=bg, ctx=ctx)
    fp, bp = w + 3, w + 5
    d_f = ctx.to_device(padded(frames, fp, 60000))
    d_bg = ctx.to_device(padded(bg, bp, -1e6))
    ip = lambda a: a.ctypes.data_as(importlib.import_module('imgprocessor_amd._lib')._ip)   # noqa: E731

    def call(n_=n, dtype=1, pitch=fp, re_=re, ce_=ce, g0_=g0, g1_=g1, out=None):
        d_out = DeviceArray(ctx, (n * g0 * g1 + 2,), np.float64)
        d_out.set(np.full(n * g0 * g1 + 2, GUARD))
        rc = ctx._lib.ipa_cell_means_dev(ctx.handle, d_f.ptr, dtype, n_, h, w, pitch, h * fp, d_bg.ptr, 2, bp,
                                         float(thresh), ip(re_), g0_, ip(ce_), g1_,
                                         (d_out if out is None else out).ptr)
        ctx.synchronize()
        return rc, d_out.get()

    rc, out = call()
    assert rc == 0 and same(out[:-2].reshape(want.shape), want) and np.all(out[-2:] == GUARD)
    bad = re.copy()
    bad[2] = bad[1] - 1
    beyond = ce.copy()
    beyond[-1] = w + 1
    for kw, status in ((dict(n_=0), ERR_BAD_ARG), (dict(n_=65), ERR_UNSUPPORTED), (dict(dtype=7), ERR_UNSUPPORTED),
                       (dict(pitch=w - 1), ERR_BAD_ARG), (dict(re_=bad), ERR_BAD_ARG), (dict(ce_=beyond), ERR_BAD_ARG),
                       (dict(g0_=0), ERR_BAD_ARG), (dict(out=d_f), ERR_BAD_ARG)):
        rc, out = call(**kw)
        assert rc == status and np.all(out == GUARD), kw
    ops = _ops()
    with pytest.raises(ValueError):
        ops.cell_means(frames, re, beyond, thresh, ctx=ctx)
    with pytest.raises(ValueError):
        ops.cell_means(frames, re, ce, thresh, bg=bg[:-1], ctx=ctx)
    with pytest.raises(TypeError):
        ops.cell_means([ctx.to_device(frames[0]), frames[1]], re, ce, thresh)
    # frames * cell rows * row segments * cell columns above 2^24
    with pytest.raises(NotImplementedError, match='2\\^24'):
        ops.cell_means(np.zeros((64, 520, 512), np.uint8), np.arange(521), np.arange(513), 0, ctx=ctx)


# ------------------------------------------------------------------------------------ the loop
@pytest.mark.parametrize('name', ('f64_bgvalue', 'u16_bgimg', 'leaves_grid', 'tall_device', 'top_left_corner'))
def test_separate_fixture_grids(ctx, g, scenes, name):
    ops = _ops()
    s = scenes[name]
    n1, n0 = s['n_cells_device']
    bgv = None if 'bg_img' in s['kw'] else s['kw'].get('bg_value', 0)
    grid = g[name + '_grid']
    ff, obj, den, iters, dev = ops.steps_separate(grid, (n0, n1), s['positions'][1], bg_value=bgv,
                                                  max_iter=sc.MAX_ITER, max_dev=sc.MAX_DEV, ctx=ctx)
    assert same(ff, g[name + '_ff']) and same(obj, g[name + '_avgobj'])
    assert den.dtype == np.int32 and np.array_equal(den, g[name + '_pointdensity'])
    assert iters == int(g[name + '_iterations']) and 0 <= dev < sc.MAX_DEV
    d = ops.steps_separate(ctx.to_device(grid), (n0, n1), s['positions'][1], bg_value=bgv, max_iter=sc.MAX_ITER,
                           max_dev=sc.MAX_DEV)
    assert same(d[0].get(), ff) and same(d[1].get(), obj) and np.array_equal(d[2].get(), den) and d[3] == iters


SEP_CASES = sc.separate_cases()


@pytest.mark.parametrize('name', sorted(SEP_CASES))
def test_separate_restatement(ctx, name):
    ops = _ops()
    grid, n_cells, pos, kw, expect = SEP_CASES[name]
    want = ref.separate(grid, n_cells, pos, kw.get('bg_value'), kw.get('max_iter', 100), kw.get('max_dev', 1e-6))
    ff, obj, den, iters, dev = ops.steps_separate(grid, n_cells, pos, ctx=ctx, **kw)
    assert same(ff, want[0]) and same(obj, want[1]) and np.array_equal(den, want[2]) and iters == want[3]
    assert np.isnan(dev) if np.isnan(want[4][-1]) else abs(dev - want[4][-1]) <= 1e-9 * want[4][-1]
    if name == 'cap':
        assert iters == kw['max_iter'] + 2 == expect
    elif name == 'zero_cell':
        assert iters == kw['max_iter'] + 2 and obj[2, 2] == np.inf and ff[3, 4] == 0 and np.isfinite(ff).all()
    else:
        assert iters < 100
    if name == 'all_nan_cell':
        assert np.isnan(ff[1, 2]) and den[1, 2] == 0 and den[0, 0] == len(grid) - 1 and np.isfinite(ff[0, 0])
    if name == 'n1':
        assert len(grid) == 1 and np.isnan(ff).sum() == ff.size - 9


def test_separate_large_grid_uses_the_workspace(ctx):
    """more cells than the kernel's LDS holds (6144 doubles for grid and device together)"""
    rng = np.random.default_rng(50)
    grid = 0.5 + rng.random((3, 70, 90))
    pos = [(0, 0), (1, 2), (-1, 3)]
    want = ref.separate(grid, (68, 85), pos, 0.1, 2, 0.0)
    got = _ops().steps_separate(grid, (68, 85), pos, bg_value=0.1, max_iter=2, max_dev=0.0, ctx=ctx)
    assert same(got[0], want[0]) and same(got[1], want[1]) and np.array_equal(got[2], want[2]) and got[3] == 4


def test_separate_refusals(ctx):
    ops = _ops()
    grid = np.ones((2, 4, 5))
    with pytest.raises(ValueError, match='max_iter'):
        ops.steps_separate(grid, (2, 2), [(0, 0), (1, 1)], max_iter=10001, ctx=ctx)
    with pytest.raises(ValueError):
        ops.steps_separate(grid, (2, 2), [(0, 0)], ctx=ctx)
    with pytest.raises(NotImplementedError):
        ops.steps_separate(np.ones((65, 2, 2)), (1, 1), [(0, 0)] * 65, ctx=ctx)
    with pytest.raises(TypeError):
        ops.steps_separate(ctx.to_device(grid.astype(np.float32)), (2, 2), [(0, 0), (1, 1)])
    rects = np.array([[0, 0, 3, 0, 2, 2], [0, 0, 0, 0, 2, 2]], np.int32)   # rows 3 .. 4 of a grid of 4
    lib = importlib.import_module('imgprocessor_amd._lib')
    d = ctx.to_device(grid)
    out = [ctx.to_device(np.full(s, GUARD)) for s in ((4, 5), (2, 2), (4, 5))]
    import ctypes as C
    it, dv = C.c_int(-5), C.c_double(GUARD)
    rc = ctx._lib.ipa_steps_separate_dev(ctx.handle, d.ptr, 2, 4, 5, 2, 2, rects.ctypes.data_as(lib._ip), 0.0, 0, 100,
                                         1e-6, out[0].ptr, out[1].ptr, out[2].ptr, C.byref(it), C.byref(dv))
    ctx.synchronize()
    assert rc == ERR_BAD_ARG and it.value == -5 and all(np.all(o.get() == GUARD) for o in out)


# ------------------------------------------------------------------------------------ the grids
@pytest.mark.parametrize('case', (((3.0, 5.0), (6, 7), (60, 84)), ((-8.5, -8.25), (6, 7), (61, 83)),
                                  ((0, 0), (1, 4), (1, 9)), ((2.5, 1), (3, 1), (7, 1)), ((14.5, 18.25), (6, 7), (270, 480))))
def test_offset_meshgrid(ctx, case):
    ops = _ops()
    yy, xx = ref.offset_meshgrid(*case)
    for dt in (np.float64, np.float32):
        d_yy, d_xx = ops.offset_meshgrid(*case, dtype=dt, ctx=ctx)
        assert same(d_yy.get(), yy.astype(dt)) and same(d_xx.get(), xx.astype(dt)), (case, dt)
    from imgprocessor_amd.interpolate import offsetMeshgrid
    h_yy, h_xx = offsetMeshgrid(*case, ctx=ctx)
    assert isinstance(h_yy, np.ndarray) and same(h_yy, yy) and same(h_xx, xx)


def test_isnan_mask(ctx):
    ops = _ops()
    rng = np.random.default_rng(60)
    for shape in ((1, 1), (6, 7), (9, 131)):
        for dt in (np.float64, np.float32):
            a = rng.standard_normal(shape).astype(dt)
            a[rng.random(shape) < 0.3] = np.nan
            a[0, 0] = np.inf
            m = ops.isnan_mask(a, ctx=ctx)
            assert m.dtype == np.uint8 and np.array_equal(m, np.isnan(a))
            assert np.array_equal(ops.isnan_mask(ctx.to_device(a)).get(), np.isnan(a))


# ------------------------------------------------------------------------------------ the routine
def _rel(got, want):
    ok = ~np.isnan(want)
    assert np.array_equal(np.isnan(got), ~ok)
    return float(np.max(np.abs(got[ok] - want[ok]) / np.abs(want[ok])))


@pytest.mark.parametrize('method', ('POLY replace', 'POLY repair'))
@pytest.mark.parametrize('name', ('f64_bgvalue', 'u16_bgimg', 'leaves_grid', 'tall_device', 'top_left_corner'))
def test_routine_against_the_fixture(ctx, g, scenes, name, method):
    from imgprocessor_amd import DeviceArray
    from imgprocessor_amd.interpolate import polyfit2dGrid
    ops, v = _ops(), V()
    s = scenes[name]
    kw = dict(s['kw'])
    if 'corners' in s:
        positions = v.positionsFromTopLeftCorner(s['corners'], s['cell_size'])
    else:
        positions = s['positions']
    got = {}
    for dev in (False, True):
        up = ctx.to_device if dev else (lambda a: a)
        k = dict(kw)
        if 'bg_img' in k:
            k['bg_img'] = up(k['bg_img'])
        frames = [up(f) for f in s['frames']] if dev else s['frames']
        ff, ff2, avgobj, den = v.vignettingFromDiscreteSteps(frames, s['n_cells_device'], positions,
                                                             postprocessing_method=method, ctx=ctx, **k)
        for a in (ff, ff2, avgobj, den):
            assert isinstance(a, DeviceArray if dev else np.ndarray)
        got[dev] = [_host(a) for a in (ff, ff2, avgobj, den)]
    for a, b in zip(got[False], got[True]):
        assert same(a, b), 'host frames and device frames differ'
    ff, ff2, avgobj, den = got[False]
    assert np.array_equal(den, g[name + '_pointdensity'])
    r_obj = _rel(avgobj, g[name + '_avgobj'])
    # the grid before the post-processing: 'POLY repair' returns the repaired grid, as the reference does
    grid_ff = ff
    if method == 'POLY repair':
        grid_ff = ops.steps_separate(ops.cell_means(s['frames'], *[
            ops.cell_edges(sc.SHAPE[a], (6, 7)[a], sc.CELL[a], ref.grid_geometry(sc.SHAPE, positions)[1][a])
            for a in (0, 1)], kw.get('thresh', kw.get('bg_value', 0)), bg=kw.get('bg_img'), ctx=ctx), s['n_cells_device'][::-1],
            positions[1], bg_value=None if 'bg_img' in kw else kw['bg_value'], ctx=ctx)[0]
    r_ff = _rel(grid_ff, g[name + '_ff'])
    print('%s %s: ff %.3g, avgobj %.3g relative to the fixture (tolerance %.3g)' % (name, method, r_ff, r_obj,
                                                                                   sc.ROUTINE_TOL))
    assert r_ff <= sc.ROUTINE_TOL and r_obj <= sc.ROUTINE_TOL
    # ff2: the same composition by hand
    (g0, g1), p01, _ = ref.grid_geometry(sc.SHAPE, positions)
    d_ff = ctx.to_device(grid_ff)
    mask = ops.isnan_mask(d_ff)
    assert mask.get().any() == (name not in ('leaves_grid', 'tall_device'))   # the scenes with a dead cell
    if method == 'POLY replace':
        want2 = polyfit2dGrid(d_ff, mask, order=5, outgrid=ops.offset_meshgrid(p01, (g0, g1), sc.SHAPE, ctx=ctx)).get()
    else:
        fitted = polyfit2dGrid(d_ff, mask, order=3)
        assert same(fitted.get(), ff) and not np.isnan(ff).any()
        yy, xx = ops.offset_meshgrid(p01, (g0, g1), sc.SHAPE, dtype=np.float32, ctx=ctx)
        want2 = v.rescaleToGrid(fitted.get(), xx.get(), yy.get())
        assert same(ops.remap(fitted, xx, yy, 'lanczos4', 'reflect', 0.0).get(), want2)
    assert ff2.shape == sc.SHAPE and ff2.dtype == np.float64 and same(ff2, want2) and np.isfinite(ff2).all()
