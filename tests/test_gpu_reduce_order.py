"""GPU: the ORDER of the calibration units' fixed-order sums (csrc/reduce.hpp: block_merge and
merge_partials under the kernels of spot.hip, nlf.hip and poly.hip), bit for bit against the numpy
restatement of the two stages (tests/reduce_ref.py).  The other tests hold these sums to 1e-12 of
the exact sum and to "a second call repeats the bits"; here a changed grid, tree or fold shows.

The frames (tests/reduce_cases.py) are the smallest at which each stage takes a second trip;
tests/test_cpu_reduce_ref.py checks that each of them tells this order from np.sum's and from the
order of one workgroup fewer.  Bits are compared as bytes, never with ==.
"""
import numpy as np
import pytest

from . import reduce_cases as rc
from . import reduce_ref as rr

pytestmark = pytest.mark.gpu

TAKE, MOMENTS, POLY = rc.take_cases(), rc.moments_cases(), rc.poly_cases()


@pytest.fixture(scope='module')
def ctx():
    import imgprocessor_amd
    return imgprocessor_amd.default_context(0)


def _ops():
    from imgprocessor_amd import ops
    return ops


@pytest.mark.parametrize('name', list(TAKE))
def test_spot_take_sum_and_count(ctx, name):
    c = TAKE[name]
    kw = dict(labels=c['labels'], label=c['label'], rows=c['rows'], bg=c['bg'], ctx=ctx)
    _, _, _, total, count = _ops().spot_take(c['img'], **kw)
    want = rr.row_unit_sum(c['values'], c['live'], c['grid'])
    print(name, float(total).hex(), float(want).hex(), count)
    assert rr.bits(total) == rr.bits(want)
    assert count == int(c['live'].sum())
    again = _ops().spot_take(c['img'], **kw)
    assert rr.bits(again[3]) == rr.bits(total) and again[4] == count


@pytest.mark.parametrize('name', list(MOMENTS))
def test_nlf_moments(ctx, name):
    c = MOMENTS[name]
    old = ctx.set_tuning(nlf_grid=c['nlf_grid'])
    try:
        got = _ops().nlf_moments(c['img'], ctx=ctx)
        again = _ops().nlf_moments(c['img'], ctx=ctx)
    finally:
        ctx.set_tuning(**old)
    v, live = c['values'], c['live']
    n = float(live.sum())
    mean = rr.row_unit_sum(v, live, c['grid']) / n
    d = v - mean
    std = np.sqrt(rr.row_unit_sum(d * d, live, c['grid']) / n)
    print(name, [float(x).hex() for x in got[:4]], float(mean).hex(), float(std).hex())
    assert rr.bits(got[0]) == rr.bits(v[live].min()) and rr.bits(got[1]) == rr.bits(v[live].max())
    assert rr.bits(got[2]) == rr.bits(mean)
    assert rr.bits(got[3]) == rr.bits(std)
    assert got[4] == 1 and got[4] == int((~live).sum())
    assert [rr.bits(x) for x in again[:4]] == [rr.bits(x) for x in got[:4]] and again[4] == got[4]


@pytest.mark.parametrize('name', list(POLY))
def test_poly2d_eval_residuum(ctx, name):
    c = POLY[name]
    out, res = _ops().poly2d_eval(c['coef'], c['arr'], mask=c['mask'], residuum=True, ctx=ctx)
    want = rr.tile_sum(rc.residuum_values(out, c['arr'], c['mask']))
    print(name, float(res).hex(), float(want).hex())
    assert rr.bits(res) == rr.bits(want)
    assert rr.bits(res) == rr.bits(rr.tile_sum(c['values']))   # the case the CPU test looked at
    again = _ops().poly2d_eval(c['coef'], c['arr'], mask=c['mask'], residuum=True, ctx=ctx)
    assert rr.bits(again[1]) == rr.bits(res) and again[0].tobytes() == out.tobytes()
