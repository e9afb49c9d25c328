"""GPU: the plain remap path by path (tests/remap_cases.py).  Every case (1) must report the kernels its
row of the table names - ctx.get_tuning('remap_path'), set at the launch sites of csrc/remap_impl.hpp,
remap.hip and fused.hip -, (2) must give the oracle's values at the tolerances of test_gpu_parity.py
(float32: rtol 1e-5 + 1e-5 x the value range; float64: 1e-12; integers: equal), and (3), where anything
but the plain gather kernel ran, must have the bits of a second run under the gather-only knobs, which
itself must report GATHER (with FRAMES_INNER or without)."""
import numpy as np
import pytest

from . import remap_cases as rc
from .conftest import assert_close
from .gpu_helpers import fresh_ring_hint, path_names as names

pytestmark = pytest.mark.gpu


@pytest.fixture(scope='module')
def ia():
    import imgprocessor_amd
    imgprocessor_amd.default_context(0)
    return imgprocessor_amd


def launch(ctx, case, dev):
    """the case's call on device arrays -> (result (n, dh, dw), remap_path)"""
    from imgprocessor_amd import ops
    from imgprocessor_amd.device import dtype_id
    kind = case.coords[0]
    dh, dw = case.dst_hw
    args = (case.interp, case.border, case.cval)
    odt = np.dtype(case.ddt)
    if case.pad:
        n, (sh, sw), dp = case.n, case.src_hw, dw + case.pad
        big = ctx.to_device(np.full((n, dh + 1, dp), 99, odt))
        head = (ctx.handle, dev['src'].ptr, dtype_id(np.dtype(case.sdt)), sh, sw, sw)
        tail = (big.ptr, dtype_id(odt), dh, dw, dp, n, sh * sw, (dh + 1) * dp, ops.interp_id(case.interp),
                ops.border_id(case.border), float(case.cval))
        if kind == 'maps':
            ctx._check(ctx._lib.ipa_remap_dev(*head, dev['mx'].ptr, dev['my'].ptr, dw, *tail), 'remap')
        else:
            assert kind == 'hom'
            ctx._check(ctx._lib.ipa_warp_perspective_dev(*head, ops._mat3(dev['M']), *tail), 'warp_perspective')
        path = ctx.get_tuning('remap_path')
        got = big.get()
        assert (got[:, dh:, :] == 99).all() and (got[:, :, dw:] == 99).all(), 'wrote outside the result'
        return np.ascontiguousarray(got[:, :dh, :dw]), path
    if kind == 'maps':
        out = ops.remap(dev['src'], dev['mx'], dev['my'], *args, out_dtype=odt)
    elif kind == 'lens':
        out = ops.undistort(dev['src'], dev['K'], dev['dist'], dev['newK'], *args, out_dtype=odt, out_shape=case.dst_hw)
    elif kind == 'hom':
        out = ops.warp_perspective(dev['src'], dev['M'], case.dst_hw, *args, out_dtype=odt)
    else:
        out = ops.warp_grid(dev['src'], dev['rects'], dev['Ms'], case.dst_hw, *args, out_dtype=odt)
    path = ctx.get_tuning('remap_path')
    return out.get(), path


def run(ctx, case, dev, knobs):
    if knobs.get('ring_remap', 1):
        fresh_ring_hint(ctx)
    old = ctx.set_tuning(**knobs)
    try:
        return launch(ctx, case, dev)
    finally:
        ctx.set_tuning(**old)


def same(got, ref, what):
    assert got.shape == ref.shape and got.dtype == ref.dtype, what
    u = {1: np.uint8, 2: np.uint16, 4: np.uint32, 8: np.uint64}[got.dtype.itemsize]
    bad = got.view(u) != ref.view(u)
    if got.dtype.kind == 'f':
        bad &= ~(np.isnan(got) & np.isnan(ref))
    assert not bad.any(), '%s: %d of %d values differ, first at %s (%r vs %r)' % (
        what, bad.sum(), got.size, np.argwhere(bad)[0], got[bad][0], ref[bad][0])


@pytest.mark.parametrize('cid', [c.id for c in rc.CASES])
def test_remap_path(ia, oracle, cid):
    case = rc.BY_ID[cid]
    ctx = ia.default_context(0)
    inp = rc.inputs(case, oracle)
    dev = {k: (ctx.to_device(v) if k in ('src', 'mx', 'my') else v) for k, v in inp.items()}
    got, path = run(ctx, case, dev, case.knobs)
    assert got.dtype == np.dtype(case.ddt) and got.shape == (case.n,) + case.dst_hw
    assert path == case.expect, 'launched %s, the table says %s' % (names(path), names(case.expect))
    worst = 0.0
    for f in (range(case.n) if case.oracle_frames is None else case.oracle_frames):
        want = rc.oracle_frame(case, inp, oracle, f)
        tol = rc.tolerance(case, inp['src'][f])
        if tol is None:
            print('%s frame %d: %d of %d integers differ' % (cid, f, (got[f] != want).sum(), want.size))
            assert np.array_equal(got[f], want), '%s frame %d: integers differ from the oracle' % (cid, f)
        else:
            err = np.abs(got[f].astype(np.float64) - want)
            worst = max(worst, float(np.nanmax(err / (tol[1] + tol[0] * np.abs(want)))))
            print('%s frame %d: worst error / tolerance %.3g' % (cid, f, worst))
            assert_close(got[f], want, tol[0], tol[1], '%s frame %d vs oracle' % (cid, f))
    if case.expect & ~(rc.GATHER | rc.FRAMES_INNER):
        ref, rpath = run(ctx, case, dev, dict(case.knobs, **rc.GATHER_ONLY))
        assert rpath in (rc.GATHER, rc.GATHER | rc.FRAMES_INNER), 'the gather-only run launched ' + names(rpath)
        same(got, ref, cid + ' against the gather kernel alone')
    if case.inner0:
        ref, rpath = run(ctx, case, dev, dict(case.knobs, frames_inner=0))
        assert rpath == rc.GATHER, 'frames_inner=0 launched ' + names(rpath)
        same(got, ref, cid + ' against frames_inner=0')
