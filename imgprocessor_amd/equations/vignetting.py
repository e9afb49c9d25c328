"""Kang-Weiss vignetting model — reference: imgProcessor/equations/vignetting.py:5-52 (S. B. Kang and
R. Weiss, "Can we calibrate a camera using an image of a flat, textureless Lambertian surface?",
ECCV 2000).  Host numpy functions under the reference's names and signatures; every value equals the
reference's bit for bit (tests/golden/fn2d.npz).  The device evaluates the orthogonal form (tilt = 0) in
the same operation order: csrc/fn2d.hip, IPA_FN2D_KW.
"""
import numpy as np


def guessVignettingParam(shape):
    """the start of a fit on a frame of `shape`: (f, alpha, rot, tilt, cx, cy)"""
    s0, s1 = shape[0], shape[1]
    return (s0 * 0.7, 0, 0, 0, s0 / 2, s1 / 2)


def vignetting(xy, f=100, alpha=0, rot=0, tilt=0, cx=50, cy=50):
    """off-axis illumination * geometric factor * tilt factor at the positions xy = (x, y)
    f: focal length [px]; alpha: coefficient of the geometric factor; tilt, rot: angles of a planar
    scene [radian]; cx, cy: the optical centre along x and y"""
    x, y = xy
    dist = ((x - cx) ** 2 + (y - cy) ** 2) ** 0.5
    off_axis = 1.0 / (1 + (dist / f) ** 2) ** 2
    geometric = (1 - alpha * dist) if alpha != 0 else 1
    tilted = tiltFactor((x, y), f, tilt, rot, (cy, cx)) if tilt != 0 else 1
    return off_axis * geometric * tilted


def tiltFactor(xy, f, tilt, rot, center=None):
    """the vignetting a tilted planar scene adds through perspective alone; `center` is accepted and,
    as in the reference, not used"""
    x, y = xy
    return np.cos(tilt) * (1 + (np.tan(tilt) / f) * (x * np.sin(rot) - y * np.cos(rot))) ** 3
