"""CPU-only: Kang-Weiss and angle-of-view fits of masked flat fields (csrc/fn2d.hip, ops_fn2d.py,
equations/, camera/flatField/postprocessing/function.py) without a device.

  * the binding: the three symbols exist, a NULL context is refused before anything is read (the
    prototypes are compared with the header by tests/test_cpu_host.py), and what ops hands to the C ABI
    fits the prototypes, recorded on a stub context;
  * every refusal that needs no device;
  * the package's equations and the restatement's model values equal the reference's recorded values
    (tests/golden/fn2d.npz) bit for bit;
  * ops.fn2d_fit - the very driver the device runs under - over the restatement's `normal` reaches
    scipy's minimum on every pinned scene, and the field function() makes of it is the reference's within
    FIELD_TOL.
"""
import math

import numpy as np
import pytest

from . import fn2d_cases as fc
from . import fn2d_ref as ref
from .conftest import load_golden
from .test_cpu_ops_calls import StubContext, check_call, run_case


@pytest.fixture(scope='module')
def golden():
    return load_golden('fn2d.npz')


# ------------------------------------------------------------------ binding
def test_binding_and_exports():
    from imgprocessor_amd import _lib, ops, ops_fn2d
    from imgprocessor_amd.camera import flatField
    from imgprocessor_amd.camera.flatField.postprocessing.function import function
    from imgprocessor_amd.equations.vignetting import vignetting, guessVignettingParam, tiltFactor  # noqa: F401
    from imgprocessor_amd.equations.angleOfView import angleOfView  # noqa: F401
    lib = _lib.lib()
    for n in ('ipa_fn2d_normal_dev', 'ipa_fn2d_eval_dev', 'ipa_fn2d_divide_dev'):
        assert n in _lib.PROTOTYPES and hasattr(lib, n)
    for n in ('fn2d_normal', 'fn2d_eval', 'fn2d_fit', 'fn2d_divide'):
        assert getattr(ops, n) is getattr(ops_fn2d, n)
    assert flatField.function is function and function.__module__.endswith('postprocessing.function')
    assert (_lib.FN2D_KW, _lib.FN2D_AOV) == (0, 1)
    assert ops_fn2d.MODELS == {'KW': (0, 4, 4), 'AoV': (1, 1, 3)} and ref.FITTED == {'KW': 4, 'AoV': 1}
    # a NULL context is refused before anything is looked at
    assert lib.ipa_fn2d_normal_dev(None, None, 3, 1, 1, 1, None, 1, 0, None, None) == _lib.ERR_BAD_ARG
    assert lib.ipa_fn2d_eval_dev(None, 0, None, 0, None, 3, 1, 1, 1, None, 1, None, None, 0, 0, 0, None, 1,
                                 None) == _lib.ERR_BAD_ARG
    assert lib.ipa_fn2d_divide_dev(None, None, 3, 1, 1, 1, 2.0) == _lib.ERR_BAD_ARG


@pytest.mark.parametrize('dev', [False, True], ids=['host', 'device'])
def test_calls_fit_their_prototypes(dev):
    from imgprocessor_amd import ops
    ctx = StubContext()
    rng = np.random.default_rng(3)
    up = ctx.to_device if dev else (lambda a: a)
    kw, aov = (5.0, 1e-3, 3.3, 4.4), (0.01, 3.5, 4.5)
    yy, xx = np.mgrid[0:4, 0:6].astype(np.float64)
    for dtype in (np.float32, np.float64):
        a, m = rng.random((7, 9)).astype(dtype), (rng.random((7, 9)) < 0.3)
        thunks = {
            'ipa_fn2d_normal_dev': [lambda: ops.fn2d_normal(up(a), up(m.view(np.uint8)), 'KW', kw, ctx=ctx),
                                    lambda: ops.fn2d_normal(up(a), None, 'AoV', aov, ctx=ctx)],
            'ipa_fn2d_eval_dev': [lambda: ops.fn2d_eval('KW', kw, up(a), up(m.view(np.uint8)), maximum=True, ctx=ctx),
                                  lambda: ops.fn2d_eval('AoV', aov, up(a), up(m.view(np.uint8)), inplace=True, ctx=ctx),
                                  lambda: ops.fn2d_eval('KW', kw, up(a), ctx=ctx),
                                  lambda: ops.fn2d_eval('KW', kw, up(a), maximum=True, ctx=ctx),
                                  lambda: ops.fn2d_eval('AoV', aov, up(a), outgrid=(up(yy), up(xx)), ctx=ctx)],
        }
        for export, ts in thunks.items():
            for t in ts:
                calls = [(n, args) for n, args in run_case(ctx, t) if not n.startswith('ipa_memcpy')]
                assert [n for n, _ in calls] == [export]
                check_call(*calls[0])
        # the division: float64 frames through flat_scale, float32 through the unit's own kernel
        calls = [(n, args) for n, args in run_case(ctx, lambda: ops.fn2d_divide(up(a), 0.75, ctx=ctx))
                 if not n.startswith('ipa_memcpy')]
        assert [n for n, _ in calls] == ['ipa_flat_scale_dev' if dtype == np.float64 else 'ipa_fn2d_divide_dev']
        check_call(*calls[0])
    # the fill in place hands the library one frame twice, a copy two different ones
    a = ctx.to_device(rng.random((7, 9)))
    m = ctx.to_device((rng.random((7, 9)) < 0.3).view(np.uint8))
    for inplace in (True, False):
        (_, args), = [c for c in run_case(ctx, lambda: ops.fn2d_eval('KW', kw, a, m, inplace=inplace))
                      if c[0] == 'ipa_fn2d_eval_dev']
        assert (args[4].value == args[16].value) == inplace
    # the angle goes down as numpy's tangent, the centre as it is
    (_, args), = run_case(ctx, lambda: ops.fn2d_normal(a, None, 'AoV', aov))
    assert [args[9][k] for k in range(3)] == [np.tan(0.01), 3.5, 4.5]


# ------------------------------------------------------------------ refusals that need no device
def test_refusals_without_a_device():
    from imgprocessor_amd import ops
    from imgprocessor_amd.camera.flatField import function
    a, m = np.ones((6, 8)), np.zeros((6, 8), bool)
    for call in (lambda: function(a, m, fn=np.sin), lambda: function(a, m, fn=lambda xy, f: xy[0] * f),
                 lambda: function(a, m, fn='POLY'), lambda: function(a, m, orthogonal=False)):
        with pytest.raises(NotImplementedError):
            call()
    for call in (lambda: function(a[0], None), lambda: function(a[None], m[None]), lambda: function(a, m[:-1]),
                 lambda: function(a, m, outgrid=(np.zeros((2, 3)), np.zeros((3, 2)))),
                 lambda: function(a, m, outgrid=(a, a), inplace=True),
                 lambda: ops.fn2d_normal(a, m, 'POLY', (1, 2, 3, 4)), lambda: ops.fn2d_normal(a, m, 'KW', (1, 2, 3)),
                 lambda: ops.fn2d_eval('AoV', (0.01,), a), lambda: ops.fn2d_eval('KW', (9, 0, 3, 4), a[0]),
                 lambda: ops.fn2d_eval('KW', (9, 0, 3, 4), a, outgrid=(a, a), inplace=True),
                 lambda: ops.fn2d_fit(a, m, 'KW', (1, 2))):
        with pytest.raises(ValueError):
            call()
    for bad in (a.astype(np.uint16), a.astype(np.int64)):
        for call in (lambda: function(bad, m), lambda: ops.fn2d_eval('KW', (9, 0, 3, 4), bad)):
            with pytest.raises(TypeError):
                call()


def test_fit_refuses_what_the_pixels_do_not_determine():
    from imgprocessor_amd import ops

    def fit(img, mask, model, **kw):
        return ops.fn2d_fit(None, None, model, fc.first_guess(model, img.shape), normal=ref.normal(img, mask, model), **kw)
    img, mask, _ = fc.scene('kw_48x64')
    few = np.ones(img.shape, bool)
    few[3, 4] = few[20, 30] = few[40, 50] = False
    with pytest.raises(ValueError, match='3 valid pixels for 4 parameters'):
        fit(img, few, 'KW')
    with pytest.raises(ValueError, match='0 valid pixels'):
        fit(img, np.ones(img.shape, bool), 'AoV')
    bad = img.copy()
    bad[np.nonzero(~mask)[0][0], np.nonzero(~mask)[1][0]] = np.nan
    with pytest.raises(ValueError, match='not finite'):
        fit(bad, mask, 'KW')
    bad[np.isnan(bad)] = np.inf
    with pytest.raises(ValueError, match='not finite'):
        fit(bad, mask, 'AoV')
    # a single row or column of pixels: a valid fit for AoV, nothing the four KW parameters could be read from
    for shape in ((1, 64), (64, 1)):
        line, lmask = fc.noisy(fc.kw_field(shape, 30.0, 2e-3, 0.3, 30.2), 5, 0.01, 0.3)
        with pytest.raises(ValueError, match='singular'):
            fit(line, lmask, 'KW')
        line, lmask = fc.noisy(fc.aov_field(shape, 0.02), 5, 0.01, 0.3)
        p, S, n, calls = fit(line, lmask, 'AoV')
        assert abs(p[0] - 0.02) < 2e-3 and n == int((~lmask).sum()) and calls < 20
    with pytest.raises(RuntimeError, match='no convergence'):
        fit(img, mask, 'KW', max_iter=3)
    # a NaN under the mask enters nothing
    nan_img, _, _ = fc.scene('kw_48x64', nan_under_mask=True)
    assert np.isnan(nan_img).sum() == mask.sum() > 0
    got, want = fit(nan_img, mask, 'KW'), fit(img, mask, 'KW')
    assert np.array_equal(got[0], want[0]) and got[1:] == want[1:]


# ------------------------------------------------------------------ the models, bit for bit
def test_model_values_equal_the_reference(golden):
    from imgprocessor_amd.equations.vignetting import vignetting, guessVignettingParam, tiltFactor
    from imgprocessor_amd.equations.angleOfView import angleOfView
    X, Y = fc.index_grid(fc.VALUE_SHAPE)
    for k, (f, alpha, cx, cy) in enumerate(fc.KW_VALUE_PARAMS):
        want = golden['kw_value_%d' % k]
        assert vignetting((X, Y), f=f, alpha=alpha, cx=cx, cy=cy).tobytes() == want.tobytes()
        assert ref.value('KW', (f, alpha, cx, cy), X, Y).tobytes() == want.tobytes()
    c0, c1 = fc.VALUE_SHAPE[0] / 2, fc.VALUE_SHAPE[1] / 2
    for k, a in enumerate(fc.AOV_VALUE_PARAMS):
        want = golden['aov_value_%d' % k]
        assert angleOfView((X, Y), fc.VALUE_SHAPE, a=a).tobytes() == want.tobytes()
        assert angleOfView((X, Y), a=a, center=(c0, c1)).tobytes() == want.tobytes()
        assert ref.value('AoV', (a, c0, c1), X, Y).tobytes() == want.tobytes()
    assert np.array_equal(np.array(guessVignettingParam((48, 64)), dtype=np.float64), golden['guess_48x64'])
    assert tiltFactor((X, Y), 120.0, 0.2, 0.3).tobytes() == golden['tilt_factor'].tobytes()
    got = vignetting((X, Y), f=120.0, alpha=1e-3, rot=0.3, tilt=0.2, cx=14.5, cy=30.25)
    assert got.tobytes() == golden['kw_value_tilted'].tobytes()
    assert angleOfView((X, Y), fc.VALUE_SHAPE, f=50.0, D=2.0).tobytes() == \
        angleOfView((X, Y), fc.VALUE_SHAPE, a=2 * np.arctan2(1.0, 50.0)).tobytes()


def test_jacobian_is_the_derivative_of_the_value():
    """the kernel's cheaper formulation: its m is the reference's value to rounding, its J the derivative"""
    shape = (12, 18)
    X, Y = fc.index_grid(shape)
    for model, p in (('KW', (11.0, 4e-3, 5.3, 8.6)), ('KW', (9.0, 0.0, 6.0, 9.0)), ('AoV', (0.05, 6.0, 9.0))):
        m, J = ref.model_terms(model, p, shape)
        assert np.abs(m - ref.value(model, p, X, Y)).max() <= 8 * np.finfo(float).eps
        for i, Ji in enumerate(J):
            h = 1e-6 * max(abs(p[i]), 1.0)
            lo, hi = list(p), list(p)
            lo[i] -= h
            hi[i] += h
            num = (ref.value(model, hi, X, Y) - ref.value(model, lo, X, Y)) / (2 * h)
            assert np.abs(Ji - num).max() <= 1e-8 * max(1.0, np.abs(num).max()), (model, i)
    # the centre on a pixel with alpha != 0: the term alpha * dx / d counts 0 there and every sum stays finite
    m, J = ref.model_terms('KW', (9.0, 5e-3, 6.0, 9.0), shape)
    assert all(np.isfinite(j).all() for j in J) and J[2][6, 9] == 0.0 and J[3][6, 9] == 0.0


# ------------------------------------------------------------------ against the reference's recorded results
@pytest.mark.parametrize('name', list(fc.PINNED))
def test_restated_fit_reaches_the_reference_minimum(golden, name):
    img, mask, model = fc.scene(name)
    assert golden[name + '_cond'] < fc.COND_MAX
    out, p, S, calls = ref.function(img, mask, replace_all=True, model=model)
    # S as the fixture's was taken: the reference's expression at the fitted parameters, through fsum
    valid = np.ones(img.shape, bool) if mask is None else ~mask
    x, y = np.nonzero(valid)
    S_ref = math.fsum((ref.value(model, p, x, y) - img[valid]) ** 2)
    print('%s: %d calls, S %.17g (kernel formulation %.17g), scipy %.17g, |p - scipy| %.3g'
          % (name, calls, S_ref, S, golden[name + '_S'], np.abs(p[:ref.FITTED[model]] - golden[name + '_params']).max()))
    assert S_ref <= golden[name + '_S'] * (1 + fc.S_RTOL)
    assert calls <= 40
    worst = 0.0
    cases = [('replace', dict(replace_all=True)), ('outgrid', dict(outgrid=fc.outgrid(img.shape)))]
    if mask is not None:
        cases.append(('repair', dict()))
    for what, kw in cases:
        got = ref.function(img, mask, model=model, **kw)[0]
        want = golden['%s_%s' % (name, what)]
        assert got.shape == want.shape and got.max() == 1.0
        worst = max(worst, np.abs(got - want).max())
    print('%s: max |restated field - reference| = %.3g' % (name, worst))
    assert worst <= fc.FIELD_TOL
