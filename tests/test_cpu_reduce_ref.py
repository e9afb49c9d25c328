"""CPU-only: every input of tests/test_gpu_reduce_order.py can tell the device's order of a sum from
other orders.  For each case the restated two-stage sum (tests/reduce_ref.py)
  * differs in bits from np.sum of the same samples in row-major order,
  * differs in bits from the restatement with one workgroup fewer,
  * lies within n * 2**-53 * sum|x| of math.fsum - the bound of any summation order.
A case that fails the first two pins nothing on the GPU: pick another seed in tests/reduce_cases.py.
"""
import math

import numpy as np
import pytest

from . import reduce_cases as rc
from . import reduce_ref as rr

TAKE, MOMENTS, POLY = rc.take_cases(), rc.moments_cases(), rc.poly_cases()


def check(samples, restated, fewer):
    """samples: what is added, in row-major order"""
    assert rr.bits(restated) != rr.bits(np.sum(samples)), 'np.sum gives the same bits'
    assert rr.bits(restated) != rr.bits(fewer), 'one workgroup fewer gives the same bits'
    exact = math.fsum(samples)
    assert abs(restated - exact) <= len(samples) * 2.0 ** -53 * math.fsum(np.abs(samples))


@pytest.mark.parametrize('c', list(TAKE.values()) + list(MOMENTS.values()), ids=list(TAKE) + list(MOMENTS))
def test_row_unit_cases_pin_the_order(c):
    assert c['grid'] >= 2
    check(c['values'][c['live']], rr.row_unit_sum(c['values'], c['live'], c['grid']),
          rr.row_unit_sum(c['values'], c['live'], c['grid'] - 1))


@pytest.mark.parametrize('c', list(POLY.values()), ids=list(POLY))
def test_tile_cases_pin_the_order(c):
    assert c['grid'] >= 2
    check(c['values'].ravel(), rr.tile_sum(c['values']), rr.tile_sum(c['values'], c['grid'] - 1))


def test_the_cases_take_the_second_trips():
    t = TAKE['take_label_1030x1_float64']
    assert rr.row_units(1030, 1) == 1030 and t['grid'] == rc.SPOT_MAX_GRID      # six workgroups take two units
    assert rr.row_units(3, 257) == 6 and TAKE['take_rows_3x257_float64']['grid'] == 4
    m = MOMENTS['moments_5x300_grid3']
    assert m['nlf_grid'] == 3 and rr.row_units(5, 300) == 10                     # 4, 3 and 3 units
    assert MOMENTS['moments_2x257_grid4']['nlf_grid'] == 0
    assert all(np.isnan(c['img']).sum() == 1 for c in MOMENTS.values())
    assert POLY['poly_fill_5x65']['grid'] == 4 and POLY['poly_all_1025x1']['grid'] == 257  # lane 0 of stage 2 takes two


def test_tree_and_fold_order():
    # the tree pairs lane t with lane t + s, top down: 1 + 2**-53 survives only in one pairing
    lanes = np.zeros(rr.LANES)
    lanes[0], lanes[128], lanes[1] = 1.0, 2.0 ** -53, 2.0 ** -53
    # step 128: lane 0 = 1 + 2**-53 -> 1 (ties to even); lane 1 keeps 2**-53 and reaches lane 0 last
    assert rr.tree(lanes) == 1.0
    lanes[128], lanes[129] = 0.0, 2.0 ** -53
    # step 128: lane 1 = 2**-52; last step: 1 + 2**-52
    assert rr.tree(lanes) == 1.0 + 2.0 ** -52
    parts = np.zeros(513)
    parts[0], parts[256], parts[512] = 1.0, 2.0 ** -53, 2.0 ** -53
    assert rr.fold_partials(parts) == 1.0     # lane 0: ((0 + 1) + 2**-53) + 2**-53; the reverse gives 1 + 2**-52
