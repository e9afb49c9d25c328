"""Seeded scenes of the vignetting-function fit tests (csrc/fn2d.hip, ops_fn2d.py,
camera/flatField/postprocessing/function.py): a Kang-Weiss or angle-of-view field with Gaussian noise
and a random mask.  tests/golden/gen_fn2d_golden.py runs the reference on the PINNED ones (with
scipy.optimize.curve_fit standing in for fancytools' fit2dArrayToFn) and asserts on each that curve_fit
converged, that the scaled J^T J at its solution has a condition number below COND_MAX and that no
fitted centre lies within CENTRE_MARGIN of a pixel (where the Kang-Weiss model has a kink for
alpha != 0).  numpy only."""
import numpy as np

COND_MAX = 1e8
CENTRE_MARGIN = 1e-6
SUM_RTOL = 1e-12         # of sum |terms|: the project's bound for cell means and poly moments
S_RTOL = 1e-9            # a least-squares minimum cannot lie above the yardstick's but by its stopping tolerance
# the distance of a fitted field to the fixture.  curve_fit stops at 1.49e-8, nothing tighter follows from it;
# measured on the CPU with the restatement: at most 3.9e-9 over the pinned scenes -> ten times that
FIELD_TOL = 3.9e-8
assert FIELD_TOL <= 1e-6
# whole fits from device sums against the same driver over the restatement, as the largest relative distance of a
# fitted parameter (relative to max(|p|, 1e-3)): measured on the GPU at most 5.42e-17 -> 100 times that;
# beyond 1e-9 it would test the stopping rule, not the sums
FIT_TOL = 5.42e-15
assert FIT_TOL <= 1e-9


def index_grid(shape):
    """(rows, cols) of every pixel as float64: the model's (x, y)"""
    x, y = np.mgrid[0:shape[0], 0:shape[1]]
    return x.astype(np.float64), y.astype(np.float64)


def kw_field(shape, f, alpha, cx, cy):
    x, y = index_grid(shape)
    d = np.sqrt((x - cx) ** 2 + (y - cy) ** 2)
    return (1 - alpha * d) / (1 + (d / f) ** 2) ** 2


def aov_field(shape, a):
    x, y = index_grid(shape)
    c0, c1 = shape[0] / 2, shape[1] / 2
    return 1 / np.sqrt(1 + np.tan(a) * (((x - c0) ** 2 + (y - c1) ** 2) / c0))


def noisy(field, seed, noise, frac, dtype=np.float64, nan_under_mask=False):
    """-> (img, mask): Gaussian noise on the field, `frac` of the pixels masked (None for frac None)"""
    rng = np.random.default_rng(seed)
    img = field + noise * rng.standard_normal(field.shape)
    mask = None if frac is None else rng.random(field.shape) < frac
    img = img.astype(dtype)
    if nan_under_mask:
        img[mask] = np.nan
    return img, mask


# name -> (shape, model, true parameters, noise, masked fraction (None: no mask), seed)
PINNED = {
    'kw_48x64': ((48, 64), 'KW', (45.0, 2e-3, 22.3, 34.6), 0.01, 0.3, 11),
    'kw_37x131': ((37, 131), 'KW', (90.0, 1e-3, 15.4, 70.7), 0.05, 0.5, 12),
    'kw_64x96_clean': ((64, 96), 'KW', (70.0, 3e-3, 30.6, 50.2), 0.0, 0.0, 13),
    'kw_64x96_nomask': ((64, 96), 'KW', (60.0, 0.0, 33.7, 45.4), 0.02, None, 14),
    'aov_48x64': ((48, 64), 'AoV', (0.02,), 0.01, 0.3, 15),
    'aov_37x131': ((37, 131), 'AoV', (0.005,), 0.03, None, 16),
}


def scene(name, dtype=np.float64, nan_under_mask=False):
    """-> (img, mask, model)"""
    shape, model, p, noise, frac, seed = PINNED[name]
    field = kw_field(shape, *p) if model == 'KW' else aov_field(shape, *p)
    img, mask = noisy(field, seed, noise, frac, dtype, nan_under_mask)
    return img, mask, model


def outgrid(shape):
    """positions between and beyond the pixels: steps of 2.1 from -3 on, past the frame's far edges"""
    n0, n1 = int(shape[0] * 0.6), int(shape[1] * 0.6)
    yy, xx = np.mgrid[0:n0, 0:n1].astype(np.float64)
    return yy * 2.1 - 3.0, xx * 2.1 - 3.0


def first_guess(model, shape):
    """what function() starts from: guessVignettingParam reduced to (f, alpha, cx, cy); 0.01 and shape / 2"""
    if model == 'KW':
        return (shape[0] * 0.7, 0.0, shape[0] / 2, shape[1] / 2)
    return (0.01, shape[0] / 2, shape[1] / 2)


# parameter sets at which the model VALUES are pinned, on a 31 x 67 grid: (f, alpha, cx, cy) with alpha = 0 and
# a centre outside the frame among them; the angles a
VALUE_SHAPE = (31, 67)
KW_VALUE_PARAMS = ((21.7, 0.0, 15.5, 33.5), (80.0, 2.5e-3, 20.25, 40.6), (150.0, 1e-3, -12.5, 90.0))
AOV_VALUE_PARAMS = (0.01, 0.3, 1.2)
