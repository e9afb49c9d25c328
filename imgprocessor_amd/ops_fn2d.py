"""The vignetting-function fit family of ``ops`` (csrc/fn2d.hip), re-exported there as
``ops.fn2d_normal``, ``ops.fn2d_eval``, ``ops.fn2d_fit`` and ``ops.fn2d_divide``.  Like every family
it goes through ``_stage_in`` / ``_stage_out``: host arrays in give host arrays out, DeviceArrays stay
on the device.

Two models of the pixel position (x = row, y = column), the first P parameters fitted, the others
constants of the frame:
  'KW'   (f, alpha, cx, cy), P = 4   equations/vignetting.py, orthogonal (tilt = 0)
  'AoV'  (a, c0, c1),        P = 1   equations/angleOfView.py with center (c0, c1)
The fit is a Levenberg-Marquardt loop on the host in float64; per trial point the device sums the
normal equations over the frame and 16 (KW) or 4 (AoV) doubles come down.
"""
import ctypes as C

import numpy as np

from . import _lib as L
from .device import DeviceArray, dtype_id
from ._staging import _ctx_of, _dptr, _f64_frame, _is_dev, _stage_in, _stage_out, _u8_frame
from .ops_flat import flat_scale
from .ops_poly import FLOAT_DTYPES, _finish, _float_host

# model -> (id, fitted parameters, all parameters)
MODELS = {'KW': (L.FN2D_KW, 4, 4), 'AoV': (L.FN2D_AOV, 1, 3)}
MAX_CALLS = 200          # normal-equation calls of one fit
# the stopping rules, far tighter than curve_fit's 1.49e-8: an accepted step that lowers S by less than
# REL_DECREASE of itself, or a step that moves the model by less than SCALED_STEP rms (both models are <= 1)
REL_DECREASE = 1e-14
SCALED_STEP = 1e-12
# J^T J scaled to a unit diagonal counts as singular where its smallest eigenvalue is below this fraction of its
# largest: the normal equations then leave a step fewer than six digits, and what the pixels say about the
# parameters is lost in the rest (a single row of pixels walks the Kang-Weiss fit down to 1e-11; fields that
# determine it sit near 1e-2)
SINGULAR_RCOND = 1e-10


def _model(name, model):
    if model not in MODELS:
        raise ValueError("%s: the model is 'KW' or 'AoV' (got %r)" % (name, model))
    return MODELS[model]


def _params(name, model, params):
    """-> (model id, P, the parameters as float64, the doubles the kernels take)"""
    mid, P, n = _model(name, model)
    p = np.array(params, dtype=np.float64).reshape(-1)
    if p.size != n:
        raise ValueError('%s: model %s has %d parameters (got %d)' % (name, model, n, p.size))
    k = p.copy()
    if mid == L.FN2D_AOV:
        k[0] = np.tan(p[0])          # numpy's tangent, as the reference takes it
    return mid, P, p, k


def fn2d_normal(img, mask, model, params, ctx=None):
    """camera/flatField/postprocessing/function.py:35-37, one evaluation of the least-squares problem
    -> (JtJ (P, P) symmetric, Jtr (P,), S, count) over the pixels of `img` (float32 / float64) where
    `mask` (uint8 / bool, None: nowhere) is NOT set: with the model value m, its Jacobian J by the
    fitted parameters and r = img - m, J^T J, J^T r, sum r^2 and the number of those pixels
    (ipa_fn2d_normal_dev).  Host float64 values, whatever `img` is."""
    mid, P, _, k = _params('fn2d_normal', model, params)
    dev, ctx, d, h, w = _stage_in('fn2d_normal', img, ctx, FLOAT_DTYPES, _float_host, (mask,))
    d_mask = None if mask is None else _u8_frame('fn2d_normal', 'the mask', mask, (h, w), ctx)
    nt = P * (P + 1) // 2
    out = np.empty(nt + P + 2)
    ctx._check(ctx._lib.ipa_fn2d_normal_dev(
        ctx.handle, d.ptr, dtype_id(d.dtype), h, w, w, d_mask.ptr if d_mask is not None else None, w, mid,
        _dptr(k), _dptr(out)), 'fn2d_normal')
    JtJ = np.zeros((P, P))
    JtJ[np.triu_indices(P)] = out[:nt]
    JtJ = JtJ + np.triu(JtJ, 1).T
    return JtJ, out[nt:nt + P].copy(), float(out[nt + P]), int(out[nt + P + 1])


def fn2d_eval(model, params, arr, mask=None, outgrid=None, inplace=False, maximum=False, ctx=None):
    """the model on the frame of `arr` (float32 / float64; its shape is the coordinate map, its dtype
    the result's), computed in double in the reference's operation order and rounded once
    (ipa_fn2d_eval_dev).
      outgrid=(yy, xx)  float64 positions, any 2-D shape, the row position from yy -> the values
                        there; arr's values are not read
      mask=None         every pixel rewritten -> a new array
      mask              the pixels where it is set replaced -> a copy, or `arr` itself with
                        inplace=True (a host array is written too)
    maximum=True returns (result, np.max of the whole result - NaN if any pixel is)."""
    mid, _, _, k = _params('fn2d_eval', model, params)
    mx = C.c_double(0.0)
    pmx = C.byref(mx) if maximum else None
    if outgrid is not None or mask is None:
        others = tuple(outgrid) if outgrid is not None else ()
        if outgrid is not None and inplace:
            raise ValueError('fn2d_eval: an outgrid has no in-place result')
        dev = _is_dev(arr)
        if inplace or dev:
            dev, ctx, d, h, w = _stage_in('fn2d_eval', arr, ctx, FLOAT_DTYPES, _float_host, others)
            dt = d.dtype
        else:   # a host frame gives its shape and type only: nothing goes up
            a = np.asarray(arr)
            if a.dtype not in FLOAT_DTYPES:
                raise TypeError('fn2d_eval needs float32 / float64 arrays (got %s)' % a.dtype)
            if a.ndim != 2:
                raise ValueError('fn2d_eval works on 2-D arrays (got shape %s)' % (a.shape,))
            ctx, d, (h, w), dt = _ctx_of(*others, ctx=ctx), None, a.shape, a.dtype
        if h < 1 or w < 1:
            raise ValueError('fn2d_eval: empty frame')
        if outgrid is not None:
            yy, xx = outgrid
            shape = tuple(yy.shape)
            if len(shape) != 2 or shape[0] < 1 or shape[1] < 1:
                raise ValueError('fn2d_eval: the outgrid must be two 2-D arrays (got shape %s)' % (shape,))
            d_gy = _f64_frame('fn2d_eval', 'outgrid[0]', yy, shape, ctx)
            d_gx = _f64_frame('fn2d_eval', 'outgrid[1]', xx, shape, ctx)
            d_out = DeviceArray(ctx, shape, dt)
            ctx._check(ctx._lib.ipa_fn2d_eval_dev(
                ctx.handle, mid, _dptr(k), L.POLY_GRID, None, dtype_id(dt), h, w, w, None, w, d_gy.ptr, d_gx.ptr,
                shape[0], shape[1], shape[1], d_out.ptr, shape[1], pmx), 'fn2d_eval')
            out = _stage_out(dev, d_out)
            return (out, mx.value) if maximum else out
        d_out = d if inplace else DeviceArray(ctx, (h, w), dt)
        ctx._check(ctx._lib.ipa_fn2d_eval_dev(
            ctx.handle, mid, _dptr(k), L.POLY_ALL, None, dtype_id(dt), h, w, w, None, w, None, None, 0, 0, 0,
            d_out.ptr, w, pmx), 'fn2d_eval')
        out = _finish(dev, arr, d_out, inplace)
        return (out, mx.value) if maximum else out
    dev, ctx, d, h, w = _stage_in('fn2d_eval', arr, ctx, FLOAT_DTYPES, _float_host, (mask,))
    d_mask = _u8_frame('fn2d_eval', 'the mask', mask, (h, w), ctx)
    d_out = d if inplace else DeviceArray(ctx, (h, w), d.dtype)
    ctx._check(ctx._lib.ipa_fn2d_eval_dev(
        ctx.handle, mid, _dptr(k), L.POLY_FILL, d.ptr, dtype_id(d.dtype), h, w, w, d_mask.ptr, w, None, None, 0, 0, 0,
        d_out.ptr, w, pmx), 'fn2d_eval')
    out = _finish(dev, arr, d_out, inplace)
    return (out, mx.value) if maximum else out


def fn2d_divide(arr, div, ctx=None):
    """arr /= div as numpy divides an array of its type by a scalar of its type (function.py:42): a
    DeviceArray in place, a host array as a new array.  float64 frames through ``flat_scale``, which is
    exactly that division; float32 frames through ipa_fn2d_divide_dev."""
    dev, ctx, d, h, w = _stage_in('fn2d_divide', arr, ctx, FLOAT_DTYPES, _float_host)
    if d.dtype == np.float64:
        flat_scale(d, div=div, out=d, ctx=ctx)
    else:
        ctx._check(ctx._lib.ipa_fn2d_divide_dev(ctx.handle, d.ptr, dtype_id(d.dtype), h, w, w, float(div)),
                   'fn2d_divide')
    return _stage_out(dev, d)


def _regular(model, JtJ):
    """ValueError where the scaled J^T J is singular: the valid pixels do not determine the parameters"""
    D = np.diag(JtJ)
    ok = np.isfinite(JtJ).all() and (D > 0).all()
    if ok:
        s = np.sqrt(D)
        ev = np.linalg.eigvalsh(JtJ / s[:, None] / s[None, :])
        ok = ev[0] > SINGULAR_RCOND * ev[-1]
    if not ok:
        raise ValueError('%s fit: the valid pixels do not determine the parameters (J^T J is singular)' % model)


def fn2d_fit(img, mask, model, guess, normal=None, max_iter=MAX_CALLS, ctx=None):
    """fancytools' fit2dArrayToFn as camera/flatField/postprocessing/function.py:35-37 uses it: the
    least-squares fit of the model to the pixels of `img` where `mask` is NOT set, from `guess` (all
    parameters of the model; the first P are fitted) -> (params, S, count, n_calls): the parameters,
    the sum of squared residuals and the number of valid pixels there, and the calls of `normal`.

    Levenberg-Marquardt on the normal equations, the damping scaled by diag(J^T J), one `normal`
    call per trial point; an accepted trial's sums are the next iteration's.  `normal(params)` ->
    (JtJ, Jtr, S, count) defaults to ``fn2d_normal`` on the frame staged to the device once.
    ValueError: fewer valid pixels than fitted parameters, a non-finite S (a NaN or an infinity among
    the valid pixels), a singular J^T J at the guess or at a point the loop accepts.  RuntimeError: `max_iter` calls without convergence."""
    _, P, p, _ = _params('fn2d_fit', model, guess)
    if normal is None:
        _, ctx, d, h, w = _stage_in('fn2d_fit', img, ctx, FLOAT_DTYPES, _float_host, (mask,))
        d_mask = None if mask is None else _u8_frame('fn2d_fit', 'the mask', mask, (h, w), ctx)

        def normal(q):
            return fn2d_normal(d, d_mask, model, q, ctx=ctx)
    JtJ, Jtr, S, n = normal(p)
    calls = 1
    if n < P:
        raise ValueError('%s fit: %d valid pixels for %d parameters' % (model, n, P))
    if not np.isfinite(S):
        raise ValueError('%s fit: the valid pixels or the guess are not finite' % model)
    _regular(model, JtJ)
    lam = 1e-3
    while S > 0.0:
        if calls >= max_iter:
            raise RuntimeError('%s fit: no convergence after %d evaluations' % (model, calls))
        D = np.diag(JtJ)
        step = np.linalg.solve(JtJ + lam * np.diag(D), Jtr)
        small = np.sqrt((step * step * D).max() / n) < SCALED_STEP
        trial = p.copy()
        trial[:P] += step
        JtJ2, Jtr2, S2, _ = normal(trial)
        calls += 1
        if np.isfinite(S2) and S2 <= S and np.isfinite(JtJ2).all() and (np.diag(JtJ2) > 0).all():
            done = small or S - S2 < REL_DECREASE * S
            p, JtJ, Jtr, S = trial, JtJ2, Jtr2, S2
            _regular(model, JtJ)
            lam = max(lam * 0.1, 1e-15)
            if done:
                break
        else:
            if small:
                break
            lam *= 10.0
    return p, S, n, calls
