"""``polyfit2dGrid`` — reference: imgProcessor/interpolate/polyfit2d.py:31-65 ("replace all masked
values with polynomial fitted ones"): a least-squares fit of a 2-D polynomial of the given order (all
x**i * y**j with i, j <= order) to the unmasked pixels of an array, evaluated at the masked pixels, at
every pixel or at an ``outgrid`` of positions.

The reference builds the (n_valid, (order+1)^2) design matrix of raw pixel monomials and hands it to
``np.linalg.lstsq``.  Its condition number grows like (image size)^(2 order): 3e10 for 270 x 480 at
order 2, 1e19 for 64 x 96 at order 5, where lstsq cuts singular values off and the "fit" misses a field
that lies in [0.6, 1] by 0.4 rms.  Here the same polynomial space is spanned by products of Chebyshev
polynomials of the pixel position mapped to [-1, 1]; the device sums the moments of the normal equations
in one pass over the frame (csrc/poly.hip: ipa_poly2d_moments_dev), the (order+1)^2-square system is
solved on the host in float64 and the device evaluates the polynomial (ipa_poly2d_eval_dev).  Where the
reference is well conditioned (cond <= 5e6: small frames, orders <= 3) the two agree to 1e-9; beyond
that this is the least-squares fit and the reference is not.

Deviations, all on purpose:
* arrays are float32 / float64 (TypeError otherwise; the reference evaluates into any dtype); the
  polynomial is evaluated in double and rounded once, the reference accumulates in the array's type;
* fewer valid pixels than coefficients, or valid pixels that do not determine the polynomial (a single
  row or column at order >= 1), raise ValueError; the reference returns lstsq's minimum-norm answer;
* orders above 5 raise NotImplementedError;
* the unstructured ``polyfit2d`` / ``polyval2d`` on point lists are not built: they are plain numpy on
  a handful of points, and this package has no CPU fallbacks.
"""
import numpy as np

from .. import ops
from .._staging import _ctx_of, _is_dev
from ..ops_poly import FLOAT_DTYPES, _order


def stage(name, arr, mask, order, ctx, others=()):
    """Every check that needs no device, then the frame and its mask on the device ->
    (dev, ctx, d_arr, d_mask); dev: the frame came as a DeviceArray."""
    _order(name, order)
    dev = _is_dev(arr)
    if not dev:
        arr = np.asarray(arr)
    if len(arr.shape) != 2 or arr.shape[0] < 1 or arr.shape[1] < 1:
        raise ValueError('%s works on non-empty 2-D arrays (got shape %s)' % (name, tuple(arr.shape)))
    if arr.dtype not in FLOAT_DTYPES:
        raise TypeError('%s needs float32 / float64 arrays (got %s)' % (name, arr.dtype))
    if mask is not None:
        if not _is_dev(mask):
            mask = np.ascontiguousarray(mask, dtype=np.uint8)
        if tuple(mask.shape) != tuple(arr.shape) or mask.dtype != np.uint8:
            raise ValueError('%s: the mask must be a uint8 / bool array of shape %s (got %s %s)'
                             % (name, tuple(arr.shape), mask.dtype, tuple(mask.shape)))
    ctx = _ctx_of(arr, mask, *others, ctx=ctx)
    d_arr = arr if dev else ctx.to_device(arr)
    d_mask = mask if mask is None or _is_dev(mask) else ctx.to_device(mask)
    return dev, ctx, d_arr, d_mask


def fit_on_device(d_arr, d_mask, order, replace_all, copy, outgrid):
    """polyfit2dGrid on DeviceArrays -> (result, residuum): the sum of |new - old| over the pixels a
    fill replaced (camera/flatField/postprocessing/polynomial.py:37 times the size); None where
    nothing was filled (replace_all with a mask, an outgrid), 0.0 where `d_arr` itself comes back."""
    M, R, count = ops.poly2d_moments(d_arr, d_mask, order)
    if d_mask is not None and count == d_arr.size and not replace_all and outgrid is None:
        return d_arr, 0.0                     # :43-45, an empty mask
    coef = ops.poly2d_solve(M, R, count, order)
    if outgrid is not None:
        return ops.poly2d_eval(coef, d_arr, outgrid=outgrid), None
    if d_mask is None:                        # :38-41 fits and rewrites everything
        return ops.poly2d_eval(coef, d_arr, residuum=True)
    if replace_all:
        return ops.poly2d_eval(coef, d_arr), None
    return ops.poly2d_eval(coef, d_arr, d_mask, inplace=not copy, residuum=True)


def polyfit2dGrid(arr, mask=None, order=3, replace_all=False, copy=True, outgrid=None, ctx=None):
    """The reference's branches: mask None without an outgrid fits every pixel and returns the fitted
    frame; an empty mask without replace_all returns `arr` itself; replace_all returns the fitted
    frame; otherwise the masked pixels are replaced, in a copy or (copy=False) in `arr`.  outgrid =
    (yy, xx): the fit evaluated at those float64 pixel positions.  Host arrays in give host arrays out
    (copy=False writes the host array), DeviceArrays stay on the device; mask: uint8 / bool, non-zero =
    invalid."""
    if outgrid is not None:
        yy, xx = outgrid
        outgrid = tuple(g if _is_dev(g) else np.ascontiguousarray(g, dtype=np.float64) for g in (yy, xx))
        if len(outgrid[0].shape) != 2 or tuple(outgrid[0].shape) != tuple(outgrid[1].shape):
            raise ValueError('polyfit2dGrid: the outgrid must be two 2-D arrays of one shape')
    dev, ctx, d_arr, d_mask = stage('polyfit2dGrid', arr, mask, order, ctx, outgrid or ())
    if outgrid is not None:
        outgrid = tuple(g if _is_dev(g) else ctx.to_device(g) for g in outgrid)
    d_out, _ = fit_on_device(d_arr, d_mask, order, replace_all, copy, outgrid)
    if dev:
        return d_out
    if d_out is d_arr:                        # the empty mask, or a fill in place
        if outgrid is None and d_mask is not None and not replace_all and not copy:
            arr[...] = d_out.get()
        return arr
    return d_out.get()
