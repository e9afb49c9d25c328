"""GPU: Kang-Weiss and angle-of-view fits of masked flat fields on the device (csrc/fn2d.hip) against the
numpy restatement (tests/fn2d_ref.py) and the reference's recorded results (tests/golden/fn2d.npz).

  * normal equations: every sum within 1e-12 of the sum of |terms| of the fsum restatement; two calls equal
    bits; host and device inputs equal bits; pitched rows with NaN padding equal bits; the order of the
    sums bit for bit (the butterfly restated in fn2d_ref.ordered_sums, stage 2 through tests/reduce_ref.py);
  * evaluation in its three modes, the maximum and the division bit for bit against the restatement;
  * whole fits from device sums against the same driver over the restatement within FIT_TOL;
  * function() against the fixture within the CPU test's FIELD_TOL;
  * the refusals of the C ABI.

Shapes at which the kernels can go wrong: 67 x 259 (no multiple of 64 wide nor of 4 tall), 1 x 64 and 64 x 1,
8200 x 5 (a workgroup takes a second share of rows), an even shape whose guess centre is a pixel.
"""
import ctypes as C

import numpy as np
import pytest

from . import fn2d_cases as fc
from . import fn2d_ref as ref
from .conftest import load_golden

pytestmark = pytest.mark.gpu

DTYPES = (np.float64, np.float32)
DT_IDS = ('f64', 'f32')
_MEMO = {}


@pytest.fixture(scope='module')
def ctx():
    import imgprocessor_amd
    return imgprocessor_amd.default_context(0)


@pytest.fixture(scope='module')
def golden():
    return load_golden('fn2d.npz')


def _ops():
    from imgprocessor_amd import ops
    return ops


def same(a, b):
    a, b = np.asarray(a), np.asarray(b)
    return a.shape == b.shape and a.dtype == b.dtype and a.tobytes() == b.tobytes()


def padded(ctx, a, pitch, guard):
    """a DeviceArray of `pitch` columns holding `a` in its first columns and `guard` in the rest"""
    p = np.full((a.shape[0], pitch), guard, a.dtype)
    p[:, :a.shape[1]] = a
    return ctx.to_device(p)


# name -> (shape, model, true parameters, parameters the sums are taken at, masked fraction or None)
SUM_SCENES = {
    'kw_67x259': ((67, 259), 'KW', (150.0, 1e-3, 30.3, 140.6), (140.0, 2e-3, 33.5, 129.5), 0.3),
    'aov_67x259': ((67, 259), 'AoV', (0.004,), (0.01, 33.5, 129.5), 0.3),
    'kw_1x64': ((1, 64), 'KW', (30.0, 2e-3, 0.3, 30.2), (25.0, 1e-3, 0.5, 32.0), 0.3),
    'kw_64x1': ((64, 1), 'KW', (30.0, 2e-3, 30.2, 0.3), (25.0, 1e-3, 32.0, 0.5), None),
    'aov_8200x5': ((8200, 5), 'AoV', (1e-4,), (2e-4, 4100.0, 2.5), 0.3),
    'kw_8200x5': ((8200, 5), 'KW', (6000.0, 1e-5, 4000.2, 2.3), (5740.0, 2e-5, 4100.0, 2.5), 0.0),
    # an even shape, the guess centre on pixel (24, 32), alpha != 0: alpha * dx / d counts 0 there
    'kw_48x64_centre': ((48, 64), 'KW', (45.0, 2e-3, 22.3, 34.6), (33.6, 1e-3, 24.0, 32.0), None),
}


def sum_scene(name, dtype):
    """-> (img, mask, model, params, fsum sums, sums of |term|), computed once"""
    key = (name, np.dtype(dtype).name)
    if key not in _MEMO:
        shape, model, true, at, frac = SUM_SCENES[name]
        field = fc.kw_field(shape, *true) if model == 'KW' else fc.aov_field(shape, *true)
        img, mask = fc.noisy(field, len(name), 0.01, frac, dtype, nan_under_mask=frac is not None and frac > 0)
        _MEMO[key] = (img, mask, model, at) + ref.flat_sums(img, mask, model, at)
        for v in _MEMO[key]:
            if isinstance(v, np.ndarray):
                v.setflags(write=False)
    return _MEMO[key]


def flat(r):
    """(JtJ, Jtr, S, count) -> the NE numbers the device returned"""
    JtJ, Jtr, S, n = r
    return np.concatenate([JtJ[np.triu_indices(len(Jtr))], Jtr, [S, float(n)]])


# ------------------------------------------------------------------ normal equations
SUM_CASES = [(n, np.float64) for n in SUM_SCENES] + [('kw_67x259', np.float32), ('aov_8200x5', np.float32)]


@pytest.mark.parametrize('name,dtype', SUM_CASES, ids=['%s-%s' % (n, np.dtype(d).name) for n, d in SUM_CASES])
def test_normal_sums(ctx, name, dtype):
    ops = _ops()
    img, mask, model, at, want, awant = sum_scene(name, dtype)
    d_img = ctx.to_device(img)
    d_mask = None if mask is None else ctx.to_device(mask.view(np.uint8))
    got = ops.fn2d_normal(d_img, d_mask, model, at)
    g = flat(got)
    assert np.isfinite(g).all() and got[3] == int(want[-1]) and isinstance(got[3], int)
    assert np.array_equal(got[0], got[0].T)
    print('%s %s: max |device - fsum| / sum |terms| = %.3g' % (name, np.dtype(dtype).name,
                                                               (np.abs(g - want) / awant).max()))
    assert np.all(np.abs(g - want) <= fc.SUM_RTOL * awant)
    assert same(flat(ops.fn2d_normal(d_img, d_mask, model, at)), g)                  # two calls
    assert same(flat(ops.fn2d_normal(img, mask, model, at, ctx=ctx)), g)             # host arrays, a bool mask


def test_normal_masks_pitch_and_refusals(ctx):
    ops = _ops()
    from imgprocessor_amd import _lib
    lib = _lib.lib()
    img, mask, model, at, want, _ = sum_scene('kw_67x259', np.float64)
    assert np.isnan(img).sum() == mask.sum() > 0                # NaN under the mask entered nothing above
    clean = np.nan_to_num(img, nan=0.5)
    # no mask is an all-zero mask; an all-set one leaves nothing
    none, zero = ops.fn2d_normal(clean, None, model, at, ctx=ctx), ops.fn2d_normal(clean, np.zeros(img.shape, bool),
                                                                                   model, at, ctx=ctx)
    assert none[3] == img.size and same(flat(none), flat(zero))
    full = flat(ops.fn2d_normal(img, np.ones(img.shape, bool), model, at, ctx=ctx))
    assert not full.any()
    assert np.isnan(ops.fn2d_normal(img, None, model, at, ctx=ctx)[2])      # a NaN among the valid pixels shows in S
    # pitched rows, NaN / 1 in the padding: the same bits
    g = flat(ops.fn2d_normal(img, mask, model, at, ctx=ctx))
    d_a, d_m = padded(ctx, img, 300, np.nan), padded(ctx, mask.view(np.uint8), 277, 1)
    par = np.array(at, dtype=np.float64)
    pp, out = par.ctypes.data_as(C.POINTER(C.c_double)), np.full(16, -1.0)
    dp = out.ctypes.data_as(C.POINTER(C.c_double))
    assert lib.ipa_fn2d_normal_dev(ctx.handle, d_a.ptr, 3, 67, 259, 300, d_m.ptr, 277, 0, pp, dp) == 0
    assert same(out, g)
    out[:] = -1.0
    assert lib.ipa_fn2d_normal_dev(ctx.handle, d_a.ptr, 3, 67, 259, 300, d_m.ptr, 277, 2, pp, dp) == _lib.ERR_BAD_ARG
    assert lib.ipa_fn2d_normal_dev(ctx.handle, d_a.ptr, 1, 67, 259, 300, d_m.ptr, 277, 0, pp, dp) == _lib.ERR_UNSUPPORTED
    assert lib.ipa_fn2d_normal_dev(ctx.handle, d_a.ptr, 3, 67, 259, 258, d_m.ptr, 277, 0, pp, dp) == _lib.ERR_BAD_ARG
    assert lib.ipa_fn2d_normal_dev(ctx.handle, d_a.ptr, 3, 67, 259, 300, d_m.ptr, 258, 0, pp, dp) == _lib.ERR_BAD_ARG
    assert lib.ipa_fn2d_normal_dev(ctx.handle, d_a.ptr, 3, 0, 259, 300, d_m.ptr, 277, 0, pp, dp) == _lib.ERR_BAD_ARG
    assert lib.ipa_fn2d_normal_dev(ctx.handle, d_a.ptr, 3, 67, 0, 300, d_m.ptr, 277, 0, pp, dp) == _lib.ERR_BAD_ARG
    assert np.all(out == -1.0), 'a refused call wrote'


@pytest.mark.parametrize('name', ['kw_67x259', 'aov_8200x5', 'kw_8200x5'])
def test_normal_sum_order(ctx, name):
    """the order of the sums, bit for bit: a changed grid, butterfly or fold shows here"""
    img, mask, model, at, _, _ = sum_scene(name, np.float64)
    grid, iters = ref.device_grid(img.shape[0], ctx.device_info()['cu_count'])
    assert iters == (2 if img.shape[0] == 8200 else 1)
    got = flat(_ops().fn2d_normal(img, mask, model, at, ctx=ctx))
    want = ref.ordered_sums(img, mask, model, at, grid)
    print(name, [float(v).hex() for v in got[:3]], [float(v).hex() for v in want[:3]])
    assert same(got, want)


# ------------------------------------------------------------------ evaluation, maximum, division
EVAL_PARAMS = (('KW', (46.9, 0.0, 33.5, 129.5)), ('KW', (80.0, 2.5e-3, 20.25, 140.6)),
               ('KW', (150.0, 1e-3, -12.5, 300.0)), ('AoV', (0.3, 33.5, 129.5)))


@pytest.mark.parametrize('dtype', DTYPES, ids=DT_IDS)
@pytest.mark.parametrize('model,params', EVAL_PARAMS, ids=['kw_a0', 'kw', 'kw_outside', 'aov'])
def test_eval_bits(ctx, model, params, dtype):
    ops = _ops()
    for shape in ((1, 1), (1, 64), (64, 1), (5, 7), (67, 259)):
        rng = np.random.default_rng(shape[0])
        a, m = (0.5 + rng.random(shape)).astype(dtype), rng.random(shape) < 0.3
        want, top = ref.evaluate(model, params, a, m)
        whole, wtop = ref.evaluate(model, params, a)
        got, mx = ops.fn2d_eval(model, params, a, m, maximum=True, ctx=ctx)
        assert same(got, want) and same(np.float64(mx), top), (shape, 'fill')
        assert same(ops.fn2d_eval(model, params, a, m, ctx=ctx), want)
        got, mx = ops.fn2d_eval(model, params, a, maximum=True, ctx=ctx)
        assert same(got, whole) and same(np.float64(mx), wtop), (shape, 'all')
        # in place on a DeviceArray: the array itself comes back, the unmasked pixels keep their bits
        d_a, d_m = ctx.to_device(a), ctx.to_device(m.view(np.uint8))
        back = ops.fn2d_eval(model, params, d_a, d_m, inplace=True)
        assert back is d_a and same(d_a.get(), want)
        d_b = ctx.to_device(a)
        out = ops.fn2d_eval(model, params, d_b, d_m)
        assert out is not d_b and same(out.get(), want) and same(d_b.get(), a)
        # the division by the maximum, numpy's in the frame's type
        assert same(ops.fn2d_divide(want, top, ctx=ctx), ref.divide(want, top)), (shape, 'divide')
        assert ops.fn2d_divide(d_a, top) is d_a and same(d_a.get(), ref.divide(want, top))
        # an outgrid between the pixels that reaches outside the frame
        h, w = shape
        yy, xx = np.mgrid[-1:2 * h + 1, -2:2 * w + 2].astype(np.float64) * 0.5
        gwant, gtop = ref.evaluate(model, params, a, outgrid=(yy, xx))
        got, mx = ops.fn2d_eval(model, params, a, outgrid=(yy, xx), maximum=True, ctx=ctx)
        assert got.shape == yy.shape and same(got, gwant) and same(np.float64(mx), gtop), (shape, 'grid')
        got = ops.fn2d_eval(model, params, d_b, outgrid=(ctx.to_device(yy), ctx.to_device(xx)))
        assert same(got.get(), gwant)


def test_eval_nan_pitch_and_refusals(ctx):
    ops = _ops()
    from imgprocessor_amd import _lib
    lib = _lib.lib()
    model, params = 'KW', (80.0, 2.5e-3, 20.25, 140.6)
    rng = np.random.default_rng(2)
    a, m = 0.5 + rng.random((67, 259)), rng.random((67, 259)) < 0.3
    # numpy's maximum: a NaN among the kept pixels gives NaN, one under the mask is replaced and gives none
    kept = a.copy()
    kept[np.nonzero(~m)[0][5], np.nonzero(~m)[1][5]] = np.nan
    got, mx = ops.fn2d_eval(model, params, kept, m, maximum=True, ctx=ctx)
    assert np.isnan(mx) and same(got, ref.evaluate(model, params, kept, m)[0])
    under = a.copy()
    under[m] = np.nan
    want, top = ref.evaluate(model, params, under, m)
    got, mx = ops.fn2d_eval(model, params, under, m, maximum=True, ctx=ctx)
    assert same(got, want) and mx == top and np.isfinite(top)
    # pitched rows with guards: only the frame is written
    d_in, d_m, d_out = padded(ctx, a, 300, -7.0), padded(ctx, m.view(np.uint8), 261, 1), padded(ctx, a * 0, 270, -9.0)
    want, top = ref.evaluate(model, params, a, m)
    par = np.array(params, dtype=np.float64)
    pp, res = par.ctypes.data_as(C.POINTER(C.c_double)), C.c_double()

    def call(mode, d_i, pin, d_o, pout, r=None, mdl=0, dt=3, h=67):
        return lib.ipa_fn2d_eval_dev(ctx.handle, mdl, pp, mode, d_i, dt, h, 259, pin, d_m.ptr, 261, None, None,
                                     0, 0, 0, d_o, pout, r)
    assert call(_lib.POLY_FILL, d_in.ptr, 300, d_out.ptr, 270, C.byref(res)) == 0
    o = d_out.get()
    assert np.all(o[:, 259:] == -9.0) and same(o[:, :259].copy(), want) and res.value == top
    assert call(_lib.POLY_FILL, d_in.ptr, 300, d_in.ptr, 300) == 0          # in place, pitched
    i = d_in.get()
    assert np.all(i[:, 259:] == -7.0) and same(i[:, :259].copy(), want)
    assert lib.ipa_fn2d_divide_dev(ctx.handle, d_in.ptr, 3, 67, 259, 300, float(top)) == 0
    i = d_in.get()
    assert np.all(i[:, 259:] == -7.0) and same(i[:, :259].copy(), ref.divide(want, top))
    assert call(_lib.POLY_FILL, d_in.ptr, 300, d_in.ptr, 299) == _lib.ERR_BAD_ARG   # overlapping, not in place
    assert call(_lib.POLY_FILL, None, 300, d_out.ptr, 270) == _lib.ERR_BAD_ARG
    assert call(_lib.POLY_FILL, d_in.ptr, 258, d_out.ptr, 270) == _lib.ERR_BAD_ARG
    assert call(_lib.POLY_ALL, None, 300, d_out.ptr, 258) == _lib.ERR_BAD_ARG
    assert call(3, d_in.ptr, 300, d_out.ptr, 270) == _lib.ERR_BAD_ARG
    assert call(_lib.POLY_FILL, d_in.ptr, 300, d_out.ptr, 270, mdl=2) == _lib.ERR_BAD_ARG
    assert call(_lib.POLY_FILL, d_in.ptr, 300, d_out.ptr, 270, dt=0) == _lib.ERR_UNSUPPORTED
    assert call(_lib.POLY_FILL, d_in.ptr, 300, d_out.ptr, 270, h=0) == _lib.ERR_BAD_ARG
    assert lib.ipa_fn2d_divide_dev(ctx.handle, d_out.ptr, 1, 67, 259, 270, 2.0) == _lib.ERR_UNSUPPORTED
    assert lib.ipa_fn2d_divide_dev(ctx.handle, d_out.ptr, 3, 67, 259, 258, 2.0) == _lib.ERR_BAD_ARG
    assert lib.ipa_fn2d_divide_dev(ctx.handle, d_out.ptr, 3, 0, 259, 270, 2.0) == _lib.ERR_BAD_ARG
    assert same(d_out.get(), o), 'a refused call wrote'


# ------------------------------------------------------------------ whole fits
def restated(name, dtype=np.float64):
    """the driver over the restatement on a pinned scene, once: (img, mask, model, {what: field}, params, S, calls)"""
    key = ('fit', name, np.dtype(dtype).name)
    if key not in _MEMO:
        img, mask, model = fc.scene(name, dtype)
        fields = {}
        cases = [('replace', dict(replace_all=True)), ('outgrid', dict(outgrid=fc.outgrid(img.shape)))]
        if mask is not None:
            cases.append(('repair', dict()))
        for what, kw in cases:
            fields[what], p, S, calls = ref.function(img, mask, model=model, **kw)
        _MEMO[key] = (img, mask, model, fields, p, S, calls)
    return _MEMO[key]


FIT_CASES = [(n, np.float64) for n in fc.PINNED] + [('kw_48x64', np.float32), ('aov_48x64', np.float32)]


@pytest.mark.parametrize('name,dtype', FIT_CASES, ids=['%s-%s' % (n, np.dtype(d).name) for n, d in FIT_CASES])
def test_fit_from_device_sums(ctx, name, dtype):
    ops = _ops()
    img, mask, model, _, want, S_want, calls_want = restated(name, dtype)
    p, S, n, calls = ops.fn2d_fit(img, mask, model, fc.first_guess(model, img.shape), ctx=ctx)
    P = ref.FITTED[model]
    # the distance in units of the parameters' own size (f and the centre are tens of pixels, alpha 1e-3)
    dist = (np.abs(p[:P] - want[:P]) / np.maximum(np.abs(want[:P]), 1e-3)).max()
    print('%s %s: %d calls (restatement %d), max relative |device fit - restated fit| = %.3g, S %.17g vs %.17g'
          % (name, np.dtype(dtype).name, calls, calls_want, dist, S, S_want))
    assert n == (img.size if mask is None else int((~mask).sum()))
    assert same(p[P:], np.asarray(want[P:]))
    assert dist <= fc.FIT_TOL
    # DeviceArrays: the same bits
    d_mask = None if mask is None else ctx.to_device(mask.view(np.uint8))
    again = ops.fn2d_fit(ctx.to_device(img), d_mask, model, fc.first_guess(model, img.shape))
    assert same(again[0], p) and again[1:] == (S, n, calls)


def test_fit_refusals_on_the_device(ctx):
    ops = _ops()
    img, mask, model = fc.scene('kw_48x64')
    with pytest.raises(ValueError, match='0 valid pixels'):
        ops.fn2d_fit(img, np.ones(img.shape, bool), 'KW', fc.first_guess('KW', img.shape), ctx=ctx)
    for shape in ((1, 64), (64, 1)):
        line, lmask = fc.noisy(fc.kw_field(shape, 30.0, 2e-3, 0.3, 30.2), 5, 0.01, 0.3)
        with pytest.raises(ValueError, match='singular'):
            ops.fn2d_fit(line, lmask, 'KW', fc.first_guess('KW', shape), ctx=ctx)
        line, lmask = fc.noisy(fc.aov_field(shape, 0.02), 5, 0.01, 0.3)
        got = ops.fn2d_fit(line, lmask, 'AoV', fc.first_guess('AoV', shape), ctx=ctx)
        want = ops.fn2d_fit(None, None, 'AoV', fc.first_guess('AoV', shape), normal=ref.normal(line, lmask, 'AoV'))
        print('aov %s: relative |device fit - restated fit| = %.3g' % (shape, abs(got[0][0] / want[0][0] - 1)))
        assert abs(got[0][0] - want[0][0]) <= fc.FIT_TOL * abs(want[0][0]) and got[2] == want[2]
    bad = img.copy()
    bad[np.nonzero(~mask)[0][0], np.nonzero(~mask)[1][0]] = np.nan
    with pytest.raises(ValueError, match='not finite'):
        ops.fn2d_fit(bad, mask, 'KW', fc.first_guess('KW', img.shape), ctx=ctx)


@pytest.mark.parametrize('name', list(fc.PINNED))
def test_function_pinned(ctx, golden, name):
    from imgprocessor_amd.camera.flatField import function
    img, mask, model, fields, _, _, _ = restated(name)
    worst = 0.0
    for what, rest in fields.items():
        args = dict(replace=dict(replace_all=True), repair={}, outgrid=dict(outgrid=fc.outgrid(img.shape)))[what]
        got = function(img.copy(), None if mask is None else mask.copy(), fn=model, ctx=ctx, **args)
        want = golden['%s_%s' % (name, what)]
        assert got.dtype == img.dtype and got.shape == want.shape and got.max() == 1.0
        worst = max(worst, np.abs(got - want).max())
        print('%s %s: |device - reference| %.3g, |device - restatement| %.3g'
              % (name, what, np.abs(got - want).max(), np.abs(got - rest).max()))
    assert worst <= fc.FIELD_TOL


def test_function_surface(ctx):
    """the reference's call surface: the default fn, device frames, in place, float32, a NaN under the mask"""
    from imgprocessor_amd.camera.flatField import function
    from imgprocessor_amd.device import DeviceArray
    from imgprocessor_amd.equations.vignetting import vignetting
    img, mask, _ = fc.scene('kw_48x64')
    want = function(img, mask, ctx=ctx)
    assert same(function(img, mask, fn=vignetting, ctx=ctx), want) and same(function(img, mask, fn='KW', ctx=ctx), want)
    d_img, d_mask = ctx.to_device(img), ctx.to_device(mask.view(np.uint8))
    out = function(d_img, d_mask)
    assert isinstance(out, DeviceArray) and out is not d_img and same(out.get(), want) and same(d_img.get(), img)
    assert function(d_img, d_mask, inplace=True) is d_img and same(d_img.get(), want)
    work = img.copy()
    assert function(work, mask, inplace=True, ctx=ctx) is work and same(work, want)
    nan_img, _, _ = fc.scene('kw_48x64', nan_under_mask=True)
    assert same(function(nan_img, mask, ctx=ctx), want)
    # no mask is a replace; a given guess is where the fit starts
    assert same(function(img, None, ctx=ctx), function(img, np.zeros(img.shape, bool), replace_all=True, ctx=ctx))
    near = function(img, mask, guess=(40.0, 1e-3, 20.0, 30.0), ctx=ctx)
    assert np.abs(near - want).max() <= fc.FIELD_TOL
    f32, _, _ = fc.scene('kw_48x64', np.float32)
    got = function(f32, mask, ctx=ctx)
    rest = ref.function(f32, mask, model='KW')[0]
    assert got.dtype == np.float32 and np.abs(got - rest).max() <= 2 * np.finfo(np.float32).eps
    aov, amask, _ = fc.scene('aov_48x64')
    assert same(function(aov, amask, fn='AoV', ctx=ctx), function(aov, amask, fn='AoV', guess=(0.01), ctx=ctx))
    with pytest.raises(ValueError):
        function(img, np.ones(img.shape, bool), ctx=ctx)
