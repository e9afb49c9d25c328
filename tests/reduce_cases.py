"""Seeded inputs of the order tests (tests/test_cpu_reduce_ref.py, tests/test_gpu_reduce_order.py):
the smallest frames at which each stage of the calibration units' two-stage sums (csrc/reduce.hpp,
tests/reduce_ref.py) takes a second trip.  Every case carries the samples the device adds up, the
lanes that add them and the number of workgroups, so that the CPU test can check that the case tells
the device's order from others.  The seeds were chosen for that: float64 samples uniform in
[0, 4000) carry fractional bits down to the last place and their sums round in every order.  numpy
only."""
import numpy as np

from . import poly_ref
from . import reduce_ref as rr

SPOT_MAX_GRID = 1024      # kSpotMaxGrid of csrc/spot.hip
NLF_MAX_GRID = 4096       # kNlfMaxGrid of csrc/nlf.hip; the cap per compute unit lies far above these frames
TAKE_BG = 0.1             # a scalar background that no float64 holds exactly: uint16 - bg has fractional bits


# case -> the seed of its frame, each the first from 1 up with which tests/test_cpu_reduce_ref.py passes.  In the
# 1025 x 1 frames a tile holds four pixels and the last tile one: one workgroup fewer moves a single addition, and
# only about one frame in two thousand shows that in the last place of the total.
SEEDS = {
    'take_rows_3x257_float64': 9,
    'take_rows_3x257_uint16': 8,
    'take_label_3x257_float64': 5,
    'take_label_3x257_uint16': 4,
    'take_label_1030x1_float64': 5,
    'take_label_1030x1_uint16': 29,
    'moments_2x257_grid4': 2,
    'moments_5x300_grid3': 1,
    'poly_fill_5x65': 4,
    'poly_all_5x65': 6,
    'poly_fill_1025x1': 2562,
    'poly_all_1025x1': 2040,
}


def _frame(rng, shape, dtype):
    a = rng.uniform(0, 4000, shape)
    return np.round(a).astype(dtype) if np.dtype(dtype).kind == 'u' else a.astype(dtype)


def take_cases():
    """ops.spot_take -> name: dict(img, bg, labels, label, rows; values, live, grid)"""
    out = {}
    for form, shape in (('rows', (3, 257)), ('label', (3, 257)), ('label', (1030, 1))):
        for dtype in (np.float64, np.uint16):
            name = 'take_%s_%dx%d_%s' % (form, shape[0], shape[1], np.dtype(dtype).name)
            rng = np.random.default_rng(SEEDS[name])
            img = _frame(rng, shape, dtype)
            x = np.asarray(img, dtype=np.float64) - TAKE_BG
            c = dict(img=img, bg=TAKE_BG, labels=None, label=0, rows=None)
            if form == 'rows':         # the second unit of each row has one live lane
                c['rows'] = (0, 2)
                c['values'], c['live'] = x[[0, 2]], np.ones((2, shape[1]), bool)
            else:
                # 1030 x 1: 1030 units against the cap of 1024 - six workgroups make a second trip, and the
                # second stage folds four partials per lane
                labels = np.ones(shape, np.int32) if shape[1] == 1 else rng.integers(0, 3, shape).astype(np.int32)
                c['labels'], c['label'] = labels, 1
                c['values'], c['live'] = x, labels == 1
            c['grid'] = rr.capped_grid(rr.row_units(*c['values'].shape), SPOT_MAX_GRID)
            out[name] = c
    return out


def moments_cases():
    """ops.nlf_moments -> name: dict(img, nlf_grid (0: the default); values, live, grid).  float64
    with one NaN: an integer frame's sum is exact in every order and pins none."""
    out = {}
    for shape, knob in (((2, 257), 0), ((5, 300), 3)):   # 5 x 300 on 3 workgroups: 4, 3 and 3 units
        grid = knob if knob else rr.capped_grid(rr.row_units(*shape), NLF_MAX_GRID)
        name = 'moments_%dx%d_grid%d' % (shape[0], shape[1], grid)
        rng = np.random.default_rng(SEEDS[name])
        img = _frame(rng, shape, np.float64)
        img[shape[0] - 1, 7] = np.nan
        out[name] = dict(
            img=img, nlf_grid=knob, values=np.nan_to_num(img), live=~np.isnan(img), grid=grid)
    return out


def poly_cases():
    """ops.poly2d_eval(residuum=True) -> name: dict(coef, arr, mask (None: ALL); values, live, grid).
    `values` is |new - old| with the restated evaluation of tests/poly_ref.py, which equals the
    device's bit for bit (tests/test_gpu_poly.py); the GPU test forms it from the frame the device
    returned.  5 x 65: 2 x 2 ragged tiles; 1025 x 1: 257 tiles, lane 0 of the second stage takes two."""
    out = {}
    for shape in ((5, 65), (1025, 1)):
        for mode in ('fill', 'all'):
            name = 'poly_%s_%dx%d' % (mode, shape[0], shape[1])
            rng = np.random.default_rng(SEEDS[name])
            arr = _frame(rng, shape, np.float64)
            coef = rng.uniform(-300, 300, (3, 3))
            mask = (rng.random(shape) < 0.6).astype(np.uint8) if mode == 'fill' else None
            y, x = np.mgrid[0:shape[0], 0:shape[1]]
            new = poly_ref.evaluate(coef, x, y, shape, arr.dtype)
            out[name] = dict(
                coef=coef, arr=arr, mask=mask, values=residuum_values(new, arr, mask),
                live=np.ones(shape, bool) if mask is None else mask != 0,
                grid=((shape[0] + 3) // 4) * ((shape[1] + 63) // 64))
    return out


def residuum_values(new, old, mask):
    """what the lanes of poly_eval_kernel hold: |new - old| where the pixel was replaced, else 0.0"""
    d = np.abs(np.asarray(new, dtype=np.float64) - np.asarray(old, dtype=np.float64))
    return d if mask is None else np.where(np.asarray(mask) != 0, d, 0.0)
