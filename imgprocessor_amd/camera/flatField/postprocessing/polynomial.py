"""``polynomial`` — reference: imgProcessor/camera/flatField/postprocessing/polynomial.py:17-50 ("POLY
repair"): replace the masked pixels of a measured flat field by a 2-D polynomial fit, then again
every area whose Laplacian is high, until the field stops changing.

The loop is the reference's, with its three exits, and runs on the device: per iteration the moments
of the fit, the residuum and the number of high-gradient pixels come to the host - 3 (order+1)^2 + 2
numbers or so - and nothing else (csrc/poly.hip).

    for _ in range(max_iter):
        out2 = polyfit2dGrid(out, mask, order, copy=not inplace, replace_all)
        if replace_all: out = out2; break
        res = mean |out2 - out|            # the unmasked pixels do not change: sum over the filled / size
        if res < max_dev: out = out2; break
        out = out2
        mask = _highGrad(out)              # |laplace| > 0.01, dilated by min(max(min(shape) // 5, 3), 15)
        m = mask.sum()
        if m == lastm or m == img.size: break
        lastm = m
    clip to [0, 1]

As written there, and kept: with inplace=True (or an empty mask) polyfit2dGrid returns the array it
was given, ``out2 - out`` is that array minus itself, and the loop ends after its first fit; a NaN
under the first mask makes the first residuum NaN, which is not below max_dev, so the loop goes on.
The fit itself deviates from the reference as interpolate/polyfit2d.py says.
"""
from ....interpolate.polyfit2d import fit_on_device, stage
from .... import ops
from ....device import DeviceArray


def polynomial(img, mask, inplace=False, replace_all=False, max_dev=1e-5, max_iter=20, order=2, ctx=None,
               trace=None):
    """-> the repaired flat field, clipped to [0, 1]: a host array for a host array (inplace=True
    writes `img`), a DeviceArray for a DeviceArray.  img: float32 / float64; mask: uint8 / bool,
    non-zero = invalid, or None.  trace: a list that receives one (residuum, high-gradient count)
    per iteration - None for a value the iteration did not compute."""
    dev, ctx, d_img, d_mask = stage('polynomial', img, mask, order, ctx)
    if inplace or not dev:   # the upload of a host array is a copy already
        out = d_img
    else:
        out = DeviceArray(ctx, d_img.shape, d_img.dtype).copy_from(d_img)
    lastm = 0
    for _ in range(int(max_iter)):
        out2, rsum = fit_on_device(out, d_mask, order, replace_all, not inplace, None)
        if replace_all:
            out = out2
            if trace is not None:
                trace.append((None, None))
            break
        res = 0.0 if out2 is out else rsum / out.size
        if res < max_dev:
            out = out2
            if trace is not None:
                trace.append((res, None))
            break
        out = out2
        d_mask, m = ops.high_grad_mask(out)
        if trace is not None:
            trace.append((res, m))
        if m == lastm or m == out.size:
            break
        lastm = m
    out = ops.clip01(out)
    if dev:
        return out
    if inplace:
        img[...] = out.get()
        return img
    return out.get()
