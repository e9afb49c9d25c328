"""``function`` — reference: imgProcessor/camera/flatField/postprocessing/function.py:9-43 ("KW replace",
"KW repair" and, with the angle-of-view model, "AoV replace" / "AoV repair" of
camera/flatField/postProcessing.py:50-74): fit a vignetting function to the valid pixels of a measured
flat field, replace the invalid pixels (or all of them) by it and divide by the maximum.

    if outgrid is not None or mask is None: replace_all = True
    guess = guessVignettingParam(shape) reduced to (f, alpha, cx, cy)       # fn == vignetting
    img2 = fit2dArrayToFn(img, fn, mask=~mask, guess=guess, outgrid=outgrid)[0]
    if not replace_all: img[mask] = img2[mask]; img2 = img
    img2 /= img2.max()

The reference's `~mask.sum() > 1000` negates an integer and is never true: it fits at full resolution,
and so does this.  ``fancytools.fit.fit2dArrayToFn`` is not part of this package; it is taken to be the
least-squares fit of fn((rows, cols), *params) to the valid pixels, started at `guess`, rebuilt on the
frame's own index grid or at fn((yy, xx), *params) for an outgrid = (yy, xx).  The fit, the rebuild,
the maximum and the division run on the device (csrc/fn2d.hip); per Levenberg-Marquardt trial 16 (KW)
or 4 (AoV) doubles come to the host (ops.fn2d_fit).

Deviations: the result has the frame's type (the reference returns float64 for replace_all); the input
is untouched unless inplace=True (the reference's repair writes `img`); ValueError where curve_fit
would return a meaningless answer - fewer valid pixels than parameters, a NaN among them, pixels that
do not determine the parameters; the tilt and rotation of the Kang-Weiss model (orthogonal=False) and
any other callable are a NotImplementedError - this package has no CPU fallback.
"""
import numpy as np

from .... import ops
from ...._staging import _is_dev
from ....equations.vignetting import vignetting, guessVignettingParam
from ....interpolate.polyfit2d import stage


def function(img, mask=None, replace_all=False, outgrid=None, fn=vignetting, guess=None, orthogonal=True,
             inplace=False, ctx=None):
    """-> the post-processed flat field, its maximum 1: a host array for a host array (inplace=True
    writes `img`), a DeviceArray for a DeviceArray.  img: float32 / float64; mask: uint8 / bool,
    non-zero = invalid, or None.  fn: ``vignetting`` or 'KW' (guess: (f, alpha, cx, cy), None: from the
    shape) or 'AoV' (guess: the angle a, None: 0.01; the centre is shape / 2, as the lambdas of
    camera/flatField/postProcessing.py:66-74 have it).  outgrid: (yy, xx), float64 positions of any 2-D
    shape - the fitted function there."""
    if fn is vignetting or fn == 'KW':
        model = 'KW'
    elif isinstance(fn, str) and fn == 'AoV':
        model = 'AoV'
    else:
        raise NotImplementedError('function: fn is vignetting, \'KW\' or \'AoV\' - the fit runs on the device, '
                                  'another callable cannot (got %r)' % (fn,))
    if not orthogonal:
        raise NotImplementedError('function: the tilt and rotation of the Kang-Weiss model are not fitted')
    if outgrid is not None or mask is None:
        replace_all = True
    if outgrid is not None:
        if inplace:
            raise ValueError('function: an outgrid has no in-place result')
        outgrid = tuple(g if _is_dev(g) else np.ascontiguousarray(g, dtype=np.float64) for g in outgrid)
        if len(outgrid[0].shape) != 2 or tuple(outgrid[0].shape) != tuple(outgrid[1].shape):
            raise ValueError('function: the outgrid must be two 2-D arrays of one shape')
    # every check that needs no device, then the frame and its mask on the device
    dev, ctx, d_img, d_mask = stage('function', img, mask, 0, ctx, outgrid or ())
    h, w = d_img.shape
    if model == 'KW':
        if guess is None:
            f, alpha, _rot, _tilt, cx, cy = guessVignettingParam((h, w))
            guess = (f, alpha, cx, cy)
    else:
        guess = (0.01 if guess is None else float(np.ravel(guess)[0]), h / 2, w / 2)
    params = ops.fn2d_fit(d_img, d_mask, model, guess, ctx=ctx)[0]
    if outgrid is not None:
        out, top = ops.fn2d_eval(model, params, d_img, outgrid=outgrid, maximum=True, ctx=ctx)
    else:
        # the upload of a host array is a copy already
        out, top = ops.fn2d_eval(model, params, d_img, mask=None if replace_all else d_mask,
                                 inplace=inplace or not dev, maximum=True, ctx=ctx)
    out = ops.fn2d_divide(out, top, ctx=ctx)
    if dev:
        return out
    if inplace:
        img[...] = out.get()
        return img
    return out.get()
