"""GPU: 2-D polynomial fits of masked frames (csrc/poly.hip and the layers above it) against the numpy
restatement (tests/poly_ref.py) and, where the reference is a usable yardstick, against its recorded
results (tests/golden/poly.npz).

  * moments within 1e-12 * sum |terms| of the exact sums (printed: the measured ratio), counts exact,
    two calls equal bits, pitched rows with NaN padding equal bits;
  * the evaluation bit for bit in all three modes, both element types, orders 0 .. 5, in place and
    into pitched rows; the residuum within 1e-12 relative of the exact sum;
  * the high-gradient mask and its count exactly, both element types;
  * polyfit2dGrid, polynomial and postProcessing within 1e-9 of the restatement and of the fixture,
    with the same iterations, mask counts and exits.
"""
import ctypes as C

import numpy as np
import pytest

from . import poly_cases as pc
from . import poly_ref as ref
from .conftest import load_golden

pytestmark = pytest.mark.gpu

DTYPES = [np.float64, np.float32]
DT_IDS = ['f64', 'f32']
_MEMO = {}


@pytest.fixture(scope='module')
def ctx():
    import imgprocessor_amd
    return imgprocessor_amd.default_context(0)


@pytest.fixture(scope='module')
def golden():
    return load_golden('poly.npz')


def _ops():
    from imgprocessor_amd import ops
    return ops


def ref_moments(shape, order, dtype):
    """the exact sums of a scene, computed once"""
    key = (shape, order, np.dtype(dtype).name)
    if key not in _MEMO:
        a, m = pc.scene(shape, sum(shape), dtype)
        _MEMO[key] = (a, m) + ref.moments(a, m, order)
        for v in _MEMO[key]:
            if isinstance(v, np.ndarray):
                v.setflags(write=False)
    return _MEMO[key]


def padded(ctx, a, pitch, guard):
    """a DeviceArray of `pitch` columns holding `a` in its first columns and `guard` in the rest"""
    p = np.full((a.shape[0], pitch), guard, a.dtype)
    p[:, :a.shape[1]] = a
    return ctx.to_device(p)


def same(a, b):
    a, b = np.asarray(a), np.asarray(b)
    return a.shape == b.shape and a.dtype == b.dtype and a.tobytes() == b.tobytes()


# ------------------------------------------------------------------ moments
MOMENT_CASES = [(s, o, np.float64) for s in pc.MOMENT_SHAPES[1:-1] for o in (0, 2, 5)]
MOMENT_CASES += [((1, 1), 0, np.float64), ((8200, 3), 2, np.float64)]
MOMENT_CASES += [((24, 40), o, np.float64) for o in (1, 3, 4)]
MOMENT_CASES += [(s, o, np.float32) for s, o in (((5, 7), 2), ((67, 259), 3), ((9, 1100), 5))]


@pytest.mark.parametrize('shape,order,dtype', MOMENT_CASES,
                         ids=['%dx%d-o%d-%s' % (s + (o, np.dtype(d).name)) for s, o, d in MOMENT_CASES])
def test_moments(ctx, shape, order, dtype):
    ops = _ops()
    a, m, M, R, n, aM, aR = ref_moments(shape, order, dtype)
    d_a, d_m = ctx.to_device(a), ctx.to_device(m.view(np.uint8))
    gM, gR, gn = ops.poly2d_moments(d_a, d_m, order)
    assert gn == n and isinstance(gn, int)
    tiny = np.finfo(np.float64).tiny
    worst = max((np.abs(gM - M) / np.maximum(aM, tiny)).max(), (np.abs(gR - R) / np.maximum(aR, tiny)).max())
    print('moments %s order %d %s: max |device - exact| / sum |terms| = %.3g' % (shape, order, np.dtype(dtype).name,
                                                                              worst))
    assert np.all(np.abs(gM - M) <= pc.MOMENT_RTOL * aM)
    assert np.all(np.abs(gR - R) <= pc.MOMENT_RTOL * aR)
    again = ops.poly2d_moments(d_a, d_m, order)
    assert same(again[0], gM) and same(again[1], gR) and again[2] == gn
    host = ops.poly2d_moments(a, m, order, ctx=ctx)           # host arrays, a bool mask
    assert same(host[0], gM) and same(host[1], gR) and host[2] == gn


def test_moments_masks_and_pitch(ctx):
    ops = _ops()
    from imgprocessor_amd import _lib
    a, m, M, R, n, _, _ = ref_moments((67, 259), 2, np.float64)
    # an all-valid mask is no mask; an all-masked one leaves nothing, whatever lies under it
    none = ops.poly2d_moments(a, None, 2, ctx=ctx)
    zero = ops.poly2d_moments(a, np.zeros(a.shape, bool), 2, ctx=ctx)
    assert none[2] == a.size and same(none[0], zero[0]) and zero[2] == a.size
    assert np.isnan(none[1]).all()                            # the scene has NaN under its mask
    full = ops.poly2d_moments(a, np.ones(a.shape, bool), 2, ctx=ctx)
    assert full[2] == 0 and not full[0].any() and not full[1].any()
    # pitched rows, NaN / 1 in the padding: the same bits
    want = ops.poly2d_moments(a, m, 2, ctx=ctx)
    d_a, d_m = padded(ctx, a, 300, np.nan), padded(ctx, m.view(np.uint8), 277, 0)
    out = np.empty(25 + 9 + 1)
    rc = _lib.lib().ipa_poly2d_moments_dev(ctx.handle, d_a.ptr, 3, 67, 259, 300, d_m.ptr, 277, 2,
                                           out.ctypes.data_as(C.POINTER(C.c_double)))
    assert rc == 0
    assert same(out[:25].reshape(5, 5), want[0]) and same(out[25:34].reshape(3, 3), want[1]) and out[34] == n
    lib = _lib.lib()
    dp = out.ctypes.data_as(C.POINTER(C.c_double))
    assert lib.ipa_poly2d_moments_dev(ctx.handle, d_a.ptr, 3, 67, 259, 300, d_m.ptr, 277, 6, dp) == _lib.ERR_UNSUPPORTED
    assert lib.ipa_poly2d_moments_dev(ctx.handle, d_a.ptr, 1, 67, 259, 300, d_m.ptr, 277, 2, dp) == _lib.ERR_UNSUPPORTED
    assert lib.ipa_poly2d_moments_dev(ctx.handle, d_a.ptr, 3, 67, 259, 258, d_m.ptr, 277, 2, dp) == _lib.ERR_BAD_ARG
    assert lib.ipa_poly2d_moments_dev(ctx.handle, d_a.ptr, 3, 0, 259, 300, d_m.ptr, 277, 2, dp) == _lib.ERR_BAD_ARG


# ------------------------------------------------------------------ evaluation
@pytest.mark.parametrize('dtype', DTYPES, ids=DT_IDS)
@pytest.mark.parametrize('order', range(0, 6))
def test_eval_bits(ctx, order, dtype):
    ops = _ops()
    rng = np.random.default_rng(order)
    coef = rng.standard_normal((order + 1, order + 1)) * 0.3
    for shape in ((1, 1), (1, 9), (9, 1), (5, 7), (67, 259)):
        a, m = pc.scene(shape, 3 + order, dtype)
        a = np.nan_to_num(a, nan=0.25).astype(dtype)
        want, rsum = ref.fill(coef, a, m)
        whole, rall = ref.fill(coef, a, None)
        got, res = ops.poly2d_eval(coef, a, m, residuum=True, ctx=ctx)
        assert same(got, want), (shape, 'fill')
        assert abs(res - rsum) <= 1e-12 * rsum
        assert same(ops.poly2d_eval(coef, a, m, ctx=ctx), want)
        got, res = ops.poly2d_eval(coef, a, residuum=True, ctx=ctx)
        assert same(got, whole) and abs(res - rall) <= 1e-12 * rall, (shape, 'all')
        assert same(ops.poly2d_eval(coef, a, ctx=ctx), whole)
        # in place on a DeviceArray: the array itself comes back, the unmasked pixels keep their bits
        d_a, d_m = ctx.to_device(a), ctx.to_device(m.view(np.uint8))
        back = ops.poly2d_eval(coef, d_a, d_m, inplace=True)
        assert back is d_a and same(d_a.get(), want)
        d_b = ctx.to_device(a)
        out = ops.poly2d_eval(coef, d_b, d_m)
        assert out is not d_b and same(out.get(), want) and same(d_b.get(), a)
        # an outgrid of half pixels that reaches outside the frame
        h, w = shape
        yy, xx = np.mgrid[-1:2 * h + 1, -2:2 * w + 2].astype(np.float64) * 0.5
        got = ops.poly2d_eval(coef, a, outgrid=(yy, xx), ctx=ctx)
        assert got.shape == yy.shape and same(got, ref.evaluate(coef, xx, yy, shape, dtype)), (shape, 'grid')
        got = ops.poly2d_eval(coef, d_a, outgrid=(ctx.to_device(yy), ctx.to_device(xx)))
        assert same(got.get(), ref.evaluate(coef, xx, yy, shape, dtype))


def test_eval_nan_pitch_and_refusals(ctx):
    ops = _ops()
    from imgprocessor_amd import _lib
    lib = _lib.lib()
    rng = np.random.default_rng(1)
    coef = np.ascontiguousarray(rng.standard_normal((3, 3)) * 0.3)
    a, m = pc.scene((67, 259), 9)                               # NaN under the mask
    got, res = ops.poly2d_eval(coef, a, m, residuum=True, ctx=ctx)
    assert np.isnan(res) and same(got, ref.fill(coef, a, m)[0])  # as the reference's mean of |out2 - out| is
    # pitched rows with guards: only the frame is written
    a = np.nan_to_num(a, nan=0.5)
    want, rsum = ref.fill(coef, a, m)
    d_in, d_m, d_out = padded(ctx, a, 300, -7.0), padded(ctx, m.view(np.uint8), 261, 1), padded(ctx, a * 0, 270, -9.0)
    res = C.c_double()
    cp = coef.ctypes.data_as(C.POINTER(C.c_double))

    def call(mode, d_i, pin, d_o, pout, r=None, order=2, dt=3):
        return lib.ipa_poly2d_eval_dev(ctx.handle, cp, order, mode, d_i, dt, 67, 259, pin, d_m.ptr, 261, None, None,
                                       0, 0, 0, d_o, pout, r)
    assert call(_lib.POLY_FILL, d_in.ptr, 300, d_out.ptr, 270, C.byref(res)) == 0
    o = d_out.get()
    assert np.all(o[:, 259:] == -9.0) and same(o[:, :259].copy(), want) and abs(res.value - rsum) <= 1e-12 * rsum
    assert call(_lib.POLY_FILL, d_in.ptr, 300, d_in.ptr, 300) == 0          # in place, pitched
    i = d_in.get()
    assert np.all(i[:, 259:] == -7.0) and same(i[:, :259].copy(), want)
    assert call(_lib.POLY_FILL, d_in.ptr, 300, d_in.ptr, 299) == _lib.ERR_BAD_ARG   # overlapping, not in place
    assert call(_lib.POLY_FILL, None, 300, d_out.ptr, 270) == _lib.ERR_BAD_ARG
    assert call(_lib.POLY_ALL, None, 300, d_out.ptr, 270, C.byref(res)) == _lib.ERR_BAD_ARG
    assert call(3, d_in.ptr, 300, d_out.ptr, 270) == _lib.ERR_BAD_ARG
    assert call(_lib.POLY_FILL, d_in.ptr, 300, d_out.ptr, 270, order=6) == _lib.ERR_UNSUPPORTED
    assert call(_lib.POLY_FILL, d_in.ptr, 300, d_out.ptr, 270, dt=0) == _lib.ERR_UNSUPPORTED
    assert same(d_out.get(), o), 'a refused call wrote'


# ------------------------------------------------------------------ high gradients, clip
@pytest.mark.parametrize('dtype', DTYPES, ids=DT_IDS)
@pytest.mark.parametrize('shape', pc.GRAD_SHAPES, ids=lambda s: '%dx%d' % s)
def test_high_grad(ctx, shape, dtype):
    ops = _ops()
    a = pc.grad_scene(shape, shape[0] + shape[1], dtype)
    want = ref.high_grad(a)
    got, n = ops.high_grad_mask(a, ctx=ctx)
    assert got.dtype == np.uint8 and np.array_equal(got, want.astype(np.uint8)) and n == int(want.sum())
    d_got, n2 = ops.high_grad_mask(ctx.to_device(a))
    assert same(d_got.get(), got) and n2 == n
    for size in (1, 2, 4, 31):
        g, k = ops.high_grad_mask(a, size=size, ctx=ctx)
        w = ref.high_grad(a, size=size)
        assert np.array_equal(g, w.astype(np.uint8)) and k == int(w.sum()), size


def test_high_grad_nan_pitch_and_clip(ctx):
    ops = _ops()
    from imgprocessor_amd import _lib
    a = pc.grad_scene((67, 259), 5)
    a[10, 20] = np.nan                                         # |NaN| > 0.01 is False: five pixels less, none more
    want = ref.high_grad(a)
    got, n = ops.high_grad_mask(a, ctx=ctx)
    assert np.array_equal(got, want.astype(np.uint8)) and n == int(want.sum())
    d_a, d_m = padded(ctx, a, 263, 1e9), padded(ctx, np.zeros(a.shape, np.uint8), 300, 7)
    cnt = C.c_double()
    assert _lib.lib().ipa_high_grad_dev(ctx.handle, d_a.ptr, 3, 67, 259, 263, 0.01, ref.window(a.shape), d_m.ptr, 300,
                                        C.byref(cnt)) == 0
    o = d_m.get()
    assert np.all(o[:, 259:] == 7) and np.array_equal(o[:, :259], got) and cnt.value == n
    for dtype in DTYPES:
        b = (pc.field(67, 259, 1, noise=0.3) * 1.2 - 0.1).astype(dtype)
        b[3, 4] = np.nan
        assert np.nanmin(b) < 0 and np.nanmax(b) > 1
        assert same(ops.clip01(b, ctx=ctx), np.clip(b, 0, 1))
        d_b = ctx.to_device(b)
        assert ops.clip01(d_b) is d_b and same(d_b.get(), np.clip(b, 0, 1))


# ------------------------------------------------------------------ polyfit2dGrid
def close(got, want, what):
    got, want = np.asarray(got, dtype=np.float64), np.asarray(want, dtype=np.float64)
    assert got.shape == want.shape, what
    err = np.abs(got - want).max()
    assert err <= pc.PIN_TOL, '%s: %.3g' % (what, err)
    return err


@pytest.mark.parametrize('name', list(pc.fit_cases()))
def test_polyfit2dGrid_pinned(ctx, golden, name):
    from imgprocessor_amd.interpolate import polyfit2dGrid
    arr, mask, kw = pc.fit_cases()[name]
    want, _ = ref.polyfit2dGrid(arr, mask, **kw)
    got = polyfit2dGrid(arr.copy(), mask, ctx=ctx, **kw)
    e1, e2 = close(got, want, 'restatement'), close(got, golden[name + '_out'], 'reference')
    print('%s: |device - restatement| %.3g, |device - reference| %.3g' % (name, e1, e2))
    d_mask = None if mask is None else ctx.to_device(mask.view(np.uint8))
    if 'outgrid' in kw:
        kw = dict(kw, outgrid=tuple(ctx.to_device(g) for g in kw['outgrid']))
    d_got = polyfit2dGrid(ctx.to_device(arr), d_mask, **kw)
    assert same(d_got.get(), got)


@pytest.mark.parametrize('order', range(0, 6))
def test_polyfit2dGrid_orders(ctx, order):
    """beyond what the reference can be pinned at: against the restatement alone"""
    from imgprocessor_amd.interpolate import polyfit2dGrid
    for shape, dtype in (((24, 40), np.float64), ((67, 259), np.float64), ((24, 40), np.float32)):
        a, m = pc.scene(shape, order, dtype)
        want, _ = ref.polyfit2dGrid(a, m, order=order)
        got = polyfit2dGrid(a, m, order=order, ctx=ctx)
        assert got.dtype == dtype and same(got[~m], a[~m])
        if dtype == np.float32:      # values below 2 that agree to 1e-9, each rounded once into float32
            assert np.abs(got.astype(np.float64) - want).max() <= pc.PIN_TOL + 2.0 ** -23
        else:
            close(got, want, (shape, order))
        whole = polyfit2dGrid(a, m, order=order, replace_all=True, ctx=ctx)
        assert same(whole[m], got[m])
    # exactly (order + 1)^2 valid pixels: the polynomial through them
    a, m = pc.field(24, 40, order), pc.exact_mask((24, 40), order)
    got = polyfit2dGrid(a, m, order=order, ctx=ctx)
    close(got, ref.polyfit2dGrid(a, m, order=order)[0], 'exact')
    assert (~m).sum() == (order + 1) ** 2
    fitted = polyfit2dGrid(a, m, order=order, replace_all=True, ctx=ctx)
    assert np.abs(fitted[~m] - a[~m]).max() <= 1e-9


def test_polyfit2dGrid_branches(ctx):
    from imgprocessor_amd.interpolate import polyfit2dGrid
    a, m = pc.scene((24, 40), 1)
    d_a, d_m = ctx.to_device(a), ctx.to_device(m.view(np.uint8))
    empty = np.zeros(a.shape, bool)
    assert polyfit2dGrid(a, empty, ctx=ctx) is a                     # :43-45
    assert polyfit2dGrid(d_a, ctx.to_device(empty.view(np.uint8))) is d_a
    want, _ = ref.polyfit2dGrid(a, m, order=3)
    out = polyfit2dGrid(d_a, d_m)                                    # a copy: the input keeps its bits
    assert out is not d_a and same(d_a.get(), a)
    close(out.get(), want, 'copy')
    assert polyfit2dGrid(d_a, d_m, copy=False) is d_a                # in place
    assert same(d_a.get(), out.get())
    host = a.copy()
    assert polyfit2dGrid(host, m, copy=False, ctx=ctx) is host and same(host, out.get())
    clean = np.nan_to_num(a, nan=0.5)
    close(polyfit2dGrid(clean, None, order=2, ctx=ctx), ref.polyfit2dGrid(clean, None, order=2)[0], 'mask None')
    # what the pixels do not determine
    for shape in ((1, 40), (40, 1)):
        row = pc.field(*shape, 2)
        with pytest.raises(ValueError):
            polyfit2dGrid(row, None, order=1, ctx=ctx)
        close(polyfit2dGrid(row, None, order=0, ctx=ctx), np.full(shape, row.mean()), 'order 0')
    with pytest.raises(ValueError):
        polyfit2dGrid(a, np.ones(a.shape, bool), ctx=ctx)
    with pytest.raises(ValueError):
        polyfit2dGrid(pc.field(3, 3, 1), None, order=3, ctx=ctx)
    assert polyfit2dGrid(np.array([[0.25]]), None, order=0, ctx=ctx)[0, 0] == 0.25
    close(polyfit2dGrid(pc.field(3, 3, 1), None, order=2, ctx=ctx), pc.field(3, 3, 1), '3 x 3 interpolates')
    with pytest.raises(NotImplementedError):
        polyfit2dGrid(d_a, d_m, order=6)


# ------------------------------------------------------------------ the POLY repair loop
@pytest.mark.parametrize('name', list(pc.loop_cases()))
def test_polynomial_pinned(ctx, golden, name):
    from imgprocessor_amd.camera.flatField import polynomial, postProcessing
    img, mask, kw, why = pc.loop_cases()[name]
    want, rtrace, took = ref.polynomial(img, mask, **kw)
    assert took == why
    trace = []
    got = polynomial(img.copy(), mask, ctx=ctx, trace=trace, **kw)
    assert len(trace) == len(rtrace) == len(golden[name + '_res'])
    assert [m for _, m in trace] == [m for _, m in rtrace]
    assert [m for _, m in trace if m is not None] == golden[name + '_m'].tolist()
    for (r, _), (rr, _), gr in zip(trace, rtrace, golden[name + '_res']):
        assert abs(r - rr) <= pc.PIN_TOL and abs(r - gr) <= pc.PIN_TOL
    e1, e2 = close(got, want, 'restatement'), close(got, golden[name + '_out'], 'reference')
    print('%s: %d iterations, exit %s, |device - restatement| %.3g, |device - reference| %.3g'
          % (name, len(trace), took, e1, e2))
    d_img = ctx.to_device(img)
    d_got = polynomial(d_img, ctx.to_device(mask.view(np.uint8)), **kw)
    assert d_got is not d_img and same(d_got.get(), got) and same(d_img.get(), img)
    assert same(postProcessing(img, 'POLY repair', mask, ctx=ctx), got)


def test_polynomial_in_place_and_post_processing(ctx):
    from imgprocessor_amd.camera.flatField import polynomial, postProcessing
    img, mask, kw, _ = pc.loop_cases()['loop_res']
    want, rtrace, _ = ref.polynomial(img.copy(), mask, inplace=True)
    d_img, trace = ctx.to_device(img), []
    got = polynomial(d_img, ctx.to_device(mask.view(np.uint8)), inplace=True, trace=trace)
    assert got is d_img and trace == rtrace == [(0.0, None)]          # as the reference is written
    close(d_img.get(), want, 'in place')
    host = img.copy()
    assert polynomial(host, mask, inplace=True, ctx=ctx) is host and same(host, d_img.get())
    # float32 frames run the same loop
    f32 = polynomial(img.astype(np.float32), mask, ctx=ctx)
    assert f32.dtype == np.float32 and np.abs(f32 - ref.polynomial(img.astype(np.float32), mask)[0]).max() <= 1e-6
    # replace_all: one fit, every pixel; 'POLY replace' is that at order 2 without the clip
    whole = polynomial(img, mask, replace_all=True, ctx=ctx)
    fit, _ = ref.polyfit2dGrid(img, mask, order=2, replace_all=True)
    close(whole, np.clip(fit, 0, 1), 'replace_all')
    close(postProcessing(img, 'POLY replace', mask, ctx=ctx), fit, 'POLY replace')
    d_out = postProcessing(ctx.to_device(img), 'POLY replace', ctx.to_device(mask.view(np.uint8)))
    close(d_out.get(), fit, 'POLY replace on the device')
    # a NaN under the first mask: the first residuum is NaN and the loop goes on
    nan = img.copy()
    nan[mask] = np.nan
    trace = []
    got = polynomial(nan, mask, ctx=ctx, trace=trace)
    assert np.isnan(trace[0][0]) and len(trace) >= 2 and np.isfinite(got).all()
    close(got, ref.polynomial(nan, mask)[0], 'NaN under the mask')
