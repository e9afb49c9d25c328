"""Angle-of-view vignetting model — reference: imgProcessor/equations/angleOfView.py:12-40 (M. Koentges,
M. Siebert, D. Hinken, "Quantitative analysis of PV-modules by electroluminescence images for quality
control", 2009).  A host numpy function under the reference's name and signature; its values equal the
reference's bit for bit (tests/golden/fn2d.npz).  The device evaluates it in the same operation order:
csrc/fn2d.hip, IPA_FN2D_AOV.
"""
import numpy as np


def angleOfView(XY, shape=None, a=None, f=None, D=None, center=None):
    """1 / sqrt(1 + tan(a) r^2 / c0) at the positions XY = (x, y), r the distance to the centre
    a: angular aperture, or from the focal length f and the aperture's diameter D (same unit);
    center: the optical centre (c0, c1), or that of a frame of `shape`"""
    if a is None:
        assert f is not None and D is not None
        a = 2 * np.arctan2(D / 2, f)
    x, y = XY
    if center is not None:
        c0, c1 = center
    else:
        c0, c1 = shape[0] / 2, shape[1] / 2
    r2 = (x - c0) ** 2 + (y - c1) ** 2
    return 1 / (1 + np.tan(a) * (r2 / c0)) ** 0.5
