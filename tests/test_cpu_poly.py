"""CPU-only: 2-D polynomial fits of masked frames (csrc/poly.hip, interpolate/polyfit2d.py,
camera/flatField/postprocessing/polynomial.py, camera/flatField/postProcessing.py) without a device.

  * the binding: the four symbols exist, a NULL context is refused before anything is read (the
    prototypes are compared with the header by tests/test_cpu_host.py), and what ops hands to the C ABI
    fits the prototypes, recorded on a stub context;
  * every refusal that needs no device: orders, dtypes, shapes, masks, unknown and unbuilt methods,
    too few valid pixels, a singular Gram matrix;
  * the numpy restatement (tests/poly_ref.py): its _highGrad equals scipy's laplace / maximum_filter
    exactly on every shape and both dtypes; its Gram assembly equals the sum over the pixels and the
    package's; its evaluation equals numpy's chebval2d; its fits and its whole POLY repair loop equal
    the reference's recorded results (tests/golden/poly.npz) within 1e-9, iteration for iteration.
"""
import numpy as np
import pytest

from . import poly_cases as pc
from . import poly_ref as ref
from .conftest import load_golden
from .test_cpu_ops_calls import StubContext, check_call, run_case


@pytest.fixture(scope='module')
def golden():
    return load_golden('poly.npz')


# ------------------------------------------------------------------ binding
def test_binding_and_exports():
    from imgprocessor_amd import _lib, ops, ops_poly
    from imgprocessor_amd.interpolate import polyfit2dGrid
    from imgprocessor_amd.interpolate.polyfit2d import polyfit2dGrid as direct
    from imgprocessor_amd.camera import flatField
    lib = _lib.lib()
    for n in ('ipa_poly2d_moments_dev', 'ipa_poly2d_eval_dev', 'ipa_high_grad_dev', 'ipa_clip01_dev'):
        assert n in _lib.PROTOTYPES and hasattr(lib, n)
    for n in ('poly2d_moments', 'poly2d_solve', 'poly2d_eval', 'high_grad_mask', 'clip01'):
        assert getattr(ops, n) is getattr(ops_poly, n)
    assert polyfit2dGrid is direct
    assert flatField.postProcessing.__module__.endswith('flatField.postProcessing')
    assert flatField.polynomial.__module__.endswith('postprocessing.polynomial')
    assert (ops_poly.MAX_ORDER, pc.MAX_ORDER) == (5, 5)
    assert (_lib.POLY_FILL, _lib.POLY_ALL, _lib.POLY_GRID) == (0, 1, 2)
    # a NULL context is refused before anything is looked at
    assert lib.ipa_poly2d_moments_dev(None, None, 3, 1, 1, 1, None, 1, 2, None) == _lib.ERR_BAD_ARG
    assert lib.ipa_poly2d_eval_dev(None, None, 2, 0, None, 3, 1, 1, 1, None, 1, None, None, 0, 0, 0, None, 1,
                                   None) == _lib.ERR_BAD_ARG
    assert lib.ipa_high_grad_dev(None, None, 3, 1, 1, 1, 0.01, 3, None, 1, None) == _lib.ERR_BAD_ARG
    assert lib.ipa_clip01_dev(None, None, 3, 1, 1, 1) == _lib.ERR_BAD_ARG


@pytest.mark.parametrize('dev', [False, True], ids=['host', 'device'])
def test_calls_fit_their_prototypes(dev):
    from imgprocessor_amd import ops
    ctx = StubContext()
    rng = np.random.default_rng(3)
    up = ctx.to_device if dev else (lambda a: a)
    coef = rng.random((3, 3))
    yy, xx = np.mgrid[0:4, 0:6].astype(np.float64)
    for dtype in (np.float32, np.float64):
        a, m = rng.random((7, 9)).astype(dtype), (rng.random((7, 9)) < 0.3)
        thunks = {
            'ipa_poly2d_moments_dev': [lambda: ops.poly2d_moments(up(a), up(m.view(np.uint8)), 2, ctx=ctx),
                                       lambda: ops.poly2d_moments(up(a), None, 5, ctx=ctx)],
            'ipa_poly2d_eval_dev': [lambda: ops.poly2d_eval(coef, up(a), up(m.view(np.uint8)), residuum=True, ctx=ctx),
                                    lambda: ops.poly2d_eval(coef, up(a), up(m.view(np.uint8)), inplace=True, ctx=ctx),
                                    lambda: ops.poly2d_eval(coef, up(a), ctx=ctx),
                                    lambda: ops.poly2d_eval(coef, up(a), residuum=True, ctx=ctx),
                                    lambda: ops.poly2d_eval(coef, up(a), outgrid=(up(yy), up(xx)), ctx=ctx)],
            'ipa_high_grad_dev': [lambda: ops.high_grad_mask(up(a), ctx=ctx)],
            'ipa_clip01_dev': [lambda: ops.clip01(up(a), ctx=ctx)],
        }
        for export, ts in thunks.items():
            for t in ts:
                calls = [(n, args) for n, args in run_case(ctx, t) if not n.startswith('ipa_memcpy')]
                assert [n for n, _ in calls] == [export]
                check_call(*calls[0])
    # the fill in place hands the library one frame twice, a copy two different ones
    a = ctx.to_device(rng.random((7, 9)))
    m = ctx.to_device((rng.random((7, 9)) < 0.3).view(np.uint8))
    for inplace in (True, False):
        (_, args), = [c for c in run_case(ctx, lambda: ops.poly2d_eval(coef, a, m, inplace=inplace))
                      if c[0] == 'ipa_poly2d_eval_dev']
        assert (args[4].value == args[16].value) == inplace


# ------------------------------------------------------------------ refusals that need no device
def test_refusals_without_a_device():
    from imgprocessor_amd import ops
    from imgprocessor_amd.interpolate import polyfit2dGrid
    from imgprocessor_amd.camera.flatField import postProcessing, polynomial, ppMETHODS
    a, m = np.ones((6, 8)), np.zeros((6, 8), bool)
    for call in (lambda: ops.poly2d_moments(a, m, 6), lambda: polyfit2dGrid(a, m, order=6),
                 lambda: polynomial(a, m, order=6), lambda: ops.poly2d_eval(np.zeros((7, 7)), a),
                 lambda: ops.high_grad_mask(a, size=32)):
        with pytest.raises(NotImplementedError):
            call()
    for call in (lambda: ops.poly2d_moments(a, m, -1), lambda: polyfit2dGrid(a[0], None),
                 lambda: polyfit2dGrid(a, m[:, :-1]), lambda: polynomial(a[None], m[None]),
                 lambda: polynomial(a, m[:-1]), lambda: polyfit2dGrid(a, outgrid=(np.zeros((2, 3)), np.zeros((3, 2)))),
                 lambda: ops.poly2d_eval(np.zeros((2, 3)), a), lambda: ops.poly2d_eval(np.zeros((3, 3)), a[0]),
                 lambda: ops.poly2d_eval(np.zeros((3, 3)), a, outgrid=(a, a), residuum=True)):
        with pytest.raises(ValueError):
            call()
    for bad in (a.astype(np.uint16), a.astype(np.int64)):
        for call in (lambda: polyfit2dGrid(bad, m), lambda: polynomial(bad, m),
                     lambda: ops.poly2d_eval(np.zeros((3, 3)), bad)):
            with pytest.raises(TypeError):
                call()
    with pytest.raises(AssertionError):
        postProcessing(a, 'POLY', m)
    with pytest.raises(AssertionError):
        postProcessing(a, mask=m)                # the reference's default is not one of its methods
    assert len(ppMETHODS) == 8
    for method in ppMETHODS:
        if not method.startswith('POLY'):
            with pytest.raises(NotImplementedError):
                postProcessing(a, method, m)


def test_solve_refuses_what_the_pixels_do_not_determine():
    from imgprocessor_amd import ops
    for shape, order in (((1, 40), 1), ((40, 1), 2), ((3, 3), 3)):
        a = pc.field(*shape, 1)
        M, R, n, _, _ = ref.moments(a, None, order)
        with pytest.raises(ValueError):
            ops.poly2d_solve(M, R, n, order)
        with pytest.raises(ValueError):
            ref.solve(M, R, n, order)
    a, order = pc.field(5, 7, 1), 2
    M, R, n, _, _ = ref.moments(a, np.ones((5, 7), bool), order)
    assert n == 0
    with pytest.raises(ValueError):
        ops.poly2d_solve(M, R, n, order)
    m = pc.exact_mask((5, 7), 2)
    m[0, 0] = True                               # one pixel short of the coefficients
    with pytest.raises(ValueError):
        ops.poly2d_solve(*ref.moments(a, m, order)[:3], order)
    # exactly (order + 1)^2 pixels on a tensor grid interpolate them; 1 x 1 at order 0 is its pixel
    for order in range(0, 4):
        shape = (9, 11)
        a, m = pc.field(*shape, 2), pc.exact_mask(shape, order)
        M, R, n, _, _ = ref.moments(a, m, order)
        assert n == (order + 1) ** 2
        c = ops.poly2d_solve(M, R, n, order)
        filled, _ = ref.fill(c, a, None)
        assert np.abs(filled[~m] - a[~m]).max() < 1e-9
    M, R, n, _, _ = ref.moments(np.array([[0.25]]), None, 0)
    assert ops.poly2d_solve(M, R, n, 0)[0, 0] == 0.25


# ------------------------------------------------------------------ the restatement
@pytest.mark.parametrize('order', range(0, 6))
def test_gram_assembly(order):
    from imgprocessor_amd import ops
    a, m = pc.scene((13, 17), order)
    M, R, n, _, _ = ref.moments(a, m, order)
    G = ref.gram(M, order)
    assert np.array_equal(G, ops.poly2d_gram(M, order))
    y, x = np.nonzero(~m)
    tu, tv = ref.cheb(ref.coord(x, 17), order), ref.cheb(ref.coord(y, 13), order)
    phi = np.stack([tv[j] * tu[i] for j in range(order + 1) for i in range(order + 1)], 1)
    assert np.abs(G - phi.T @ phi).max() <= 1e-12 * n
    assert np.abs(R.reshape(-1) - phi.T @ a[~m]).max() <= 1e-12 * n
    # the conditioning that makes the normal equations usable: the raw-monomial design matrix of this frame at
    # order 5 is at 2e12, its Gram matrix at the square of that
    assert np.linalg.cond(G) < 1e6


def test_evaluation_is_the_chebyshev_series():
    from numpy.polynomial.chebyshev import chebval2d
    rng = np.random.default_rng(0)
    for order in range(0, 6):
        c = rng.standard_normal((order + 1, order + 1))
        y, x = np.mgrid[-2:9, -3:12].astype(np.float64) * 0.75
        got = ref.evaluate(c, x, y, (7, 9), np.float64)
        want = chebval2d(ref.coord(y, 7), ref.coord(x, 9), c)
        assert np.abs(got - want).max() <= 1e-12 * np.abs(want).max()
    assert np.array_equal(ref.evaluate(np.array([[0.5]]), [[3.0]], [[2.0]], (1, 1), np.float32), [[np.float32(0.5)]])


@pytest.mark.parametrize('dtype', [np.float64, np.float32], ids=['f64', 'f32'])
@pytest.mark.parametrize('shape', pc.GRAD_SHAPES, ids=lambda s: '%dx%d' % s)
def test_high_grad_equals_scipy(shape, dtype):
    from scipy.ndimage import laplace, maximum_filter
    a = pc.grad_scene(shape, shape[0] + shape[1], dtype)
    lap = laplace(a, mode='reflect')
    assert lap.dtype == dtype and np.array_equal(ref.laplace(a), lap)
    s = min(a.shape)
    want = maximum_filter(np.abs(lap) > 0.01, min(max(s // 5, 3), 15))
    got = ref.high_grad(a)
    assert got.dtype == bool and np.array_equal(got, want)
    if min(shape) >= 20:                         # below that the field's own curvature is above the threshold
        b = np.abs(lap) > 0.01
        assert 0 < b.sum() < b.size, 'the scene does not exercise the threshold'
    for size in (1, 2, 4):                       # even windows sit off centre as scipy's do
        assert np.array_equal(ref.high_grad(a, size=size), maximum_filter(np.abs(lap) > 0.01, size))


def test_window_sizes():
    from imgprocessor_amd import ops
    for shape, want in (((130, 70), 14), ((80, 90), 15), ((24, 40), 4), ((5, 7), 3), ((2000, 3000), 15)):
        assert ops.high_grad_window(shape) == ref.window(shape) == want


# ------------------------------------------------------------------ against the reference's recorded results
@pytest.mark.parametrize('name', list(pc.fit_cases()))
def test_restated_fit_equals_the_reference(golden, name):
    arr, mask, kw = pc.fit_cases()[name]
    assert golden[name + '_cond'].max() <= pc.COND_MAX
    got, _ = ref.polyfit2dGrid(arr, mask, **kw)
    want = golden[name + '_out']
    assert got.shape == want.shape and np.isfinite(got).all()
    err = np.abs(got - want).max()
    print('%s: max |restatement - reference| = %.3g (cond %.3g)' % (name, err, golden[name + '_cond'].max()))
    assert err <= pc.PIN_TOL


@pytest.mark.parametrize('name', list(pc.loop_cases()))
def test_restated_loop_equals_the_reference(golden, name):
    img, mask, kw, why = pc.loop_cases()[name]
    assert golden[name + '_cond'].max() <= pc.COND_MAX
    got, trace, took = ref.polynomial(img, mask, **kw)
    res = [r for r, _ in trace]
    ms = [m for _, m in trace if m is not None]
    assert took == why and len(res) == len(golden[name + '_res'])
    assert ms == golden[name + '_m'].tolist()
    assert np.abs(np.array(res) - golden[name + '_res']).max() <= pc.PIN_TOL
    if why == 'res':
        assert len(res) >= 3 and res[-1] < pc.MAX_DEV <= res[-2]
    want = golden[name + '_out']
    err = np.abs(got - want).max()
    print('%s: %d iterations, exit %s, max |restatement - reference| = %.3g' % (name, len(res), took, err))
    assert err <= pc.PIN_TOL
    assert got.min() >= 0.0 and got.max() <= 1.0


def test_loop_in_place_ends_after_one_fit():
    """as the reference is written: polyfit2dGrid(copy=False) returns the array it was given, `out2 - out` is
    zero and the loop ends on its first residuum"""
    img, mask, kw, _ = pc.loop_cases()['loop_res']
    work = img.copy()
    got, trace, took = ref.polynomial(work, mask, inplace=True)
    assert took == 'res' and trace == [(0.0, None)]
    first, _ = ref.polyfit2dGrid(img, mask, order=2)
    assert np.array_equal(got, np.clip(first, 0, 1))
