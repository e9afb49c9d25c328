"""GPU: the remap -> filter chains route by route (tests/chain_cases.py).  Every case (1) must leave the launch
record its row of the table names - ctx.get_tuning('chain_path'), set where fused.hip decides and where
fused_impl.hpp, fused_big.hip and wave_sep.hpp launch -, (2) must give, frame by frame, the oracle's remap
(float32) filtered by tests/conv_ref.py in float64, at the tolerance the suite holds the chains to (rtol 1e-5 +
1e-5 x the frames' value range), and (3), where the record has FRAMES_WG, SPLIT, STORED or LENS_MAP, runs once
more under the knobs that take those away: that run must report the plain form, must be right as well, and -
where it ran the same kernel - must give the same bits.  The exports are called straight through ctypes, as
tests/test_gpu_chain_borders.py does, so that one case can put source and result into one allocation."""
import ctypes as C

import numpy as np
import pytest

from . import chain_cases as cc
from .conftest import assert_close
from .gpu_helpers import same_bits

pytestmark = pytest.mark.gpu

SLACK = 64        # elements between the source frames of the overlap cases


@pytest.fixture(scope='module')
def ia():
    import imgprocessor_amd
    imgprocessor_amd.default_context(0)
    return imgprocessor_amd


@pytest.fixture(scope='module')
def resident(ia):
    """device copies shared by the cases: the frames per dtype, the maps per geometry"""
    return {}


def device_inputs(ctx, resident, case, inp):
    key = ('src', case.sdt)
    if key not in resident:
        resident[key] = ctx.to_device(np.ascontiguousarray(cc.source(case._replace(n=cc.NMAX))))
    dev = {'src': resident[key].ptr}
    if case.coords == 'maps':
        key = ('maps', case.shape)
        if key not in resident:
            resident[key] = (ctx.to_device(inp['mx']), ctx.to_device(inp['my']))
        dev['mx'], dev['my'] = resident[key][0].ptr, resident[key][1].ptr
    return dev


def call(ia, ctx, case, inp, src_ptr, dev, dst_ptr, src_stride):
    """the case's export; -> chain_path after it"""
    from imgprocessor_amd import _lib as L
    from imgprocessor_amd.device import dtype_id
    from imgprocessor_amd.ops import border_id, interp_id
    (sh, sw), (dh, dw) = cc.SRC_HW, cc.SHAPES[case.shape]
    dp = C.POINTER(C.c_double)
    head = (ctx.handle, src_ptr, dtype_id(np.dtype(case.sdt)), sh, sw, sw)
    if case.coords == 'maps':
        kind, where = 'remap', (dev['mx'], dev['my'], dw)
    elif case.coords == 'hom':
        kind, where = 'warp_perspective', (L.dbl(np.ravel(inp['M']), 9),)
    else:
        kind, where = 'undistort', (L.dbl(np.ravel(inp['K']), 9), L.dbl(inp['dist'], 5), L.dbl(np.ravel(inp['newK']), 9))
    tail = (dst_ptr, dtype_id(np.float32), dh, dw, dw, case.n, src_stride, dh * dw, interp_id(case.interp),
            border_id('constant'), float(cc.BORDER_VALUE[case.sdt]), border_id('reflect'), border_id('reflect'))
    filt = inp['filt']
    if isinstance(filt, tuple):
        ky = np.ascontiguousarray(filt[0], dtype=np.float64)
        kx = np.ascontiguousarray(filt[1], dtype=np.float64)
        fn = getattr(ctx._lib, 'ipa_%s_sepconv2d_dev' % kind)
        args = head + where + (ky.ctypes.data_as(dp), ky.size, kx.ctypes.data_as(dp), kx.size) + tail
    else:
        k = np.ascontiguousarray(filt, dtype=np.float64)
        fn = getattr(ctx._lib, 'ipa_%s_conv2d_dev' % kind)
        args = head + where + (k.ctypes.data_as(dp), k.shape[0], k.shape[1]) + tail
    ctx._check(fn(*args), case.id)
    return ctx.get_tuning('chain_path')


def run(ia, ctx, resident, case, inp, knobs, overlap=False):
    """-> (result (n, dh, dw) float32, chain_path) under strip_h = 16 and `knobs`"""
    (sh, sw), (dh, dw) = cc.SRC_HW, cc.SHAPES[case.shape]
    dev = device_inputs(ctx, resident, case, inp)
    old = ctx.set_tuning(strip_h=cc.STRIP_H, **knobs)
    try:
        if not overlap:
            dst = ia.DeviceArray(ctx, (case.n, dh, dw), np.float32)
            path = call(ia, ctx, case, inp, dev['src'], dev, dst.ptr, sh * sw)
            return dst.get(), path
        # one allocation: the source frames a stride of sh * sw + SLACK apart, the result from the end of the last
        # frame's pixels on - inside the last stride, so that the ranges overlap as fused_plan measures them
        assert case.sdt == cc.F32 and (sh * sw) % 4 == 0
        stride, off = sh * sw + SLACK, (case.n - 1) * (sh * sw + SLACK) + sh * sw
        host = np.full(off + case.n * dh * dw, 7.0, np.float32)
        for f in range(case.n):
            host[f * stride:f * stride + sh * sw] = inp['src'][f].ravel()
        both = ctx.to_device(host)
        assert both.ptr.value % 16 == 0 and off < case.n * stride
        path = call(ia, ctx, case, inp, both.ptr, dev, C.c_void_p(both.ptr.value + 4 * off), stride)
        got = both.get()
        for f in range(case.n):
            assert np.array_equal(got[f * stride:f * stride + sh * sw], inp['src'][f].ravel()), 'the source was written'
        return got[off:].reshape(case.n, dh, dw).copy(), path
    finally:
        ctx.set_tuning(**old)


def against_reference(case, inp, oracle, got, what):
    rtol, atol = cc.tolerance(case)
    worst = 0.0
    for f in range(case.n):
        want = cc.expected(case, inp, oracle, f)
        err = np.abs(got[f].astype(np.float64) - want)
        worst = max(worst, float((err / cc.rounding_bound(case, inp, oracle, f)).max()))
        assert_close(got[f], want, rtol, atol, '%s, %s, frame %d of %d' % (case.id, what, f, case.n))
    print('%s, %s: worst error / conv_ref.bound() %.3g (the tolerance is %.3g bounds there at the least)'
          % (case.id, what, worst, float(((atol + rtol * np.abs(want)) / cc.rounding_bound(case, inp, oracle, case.n - 1)).min())))


@pytest.mark.parametrize('cid', [c.id for c in cc.CASES])
def test_chain_path(ia, oracle, resident, cid):
    case = cc.BY_ID[cid]
    ctx = ia.default_context(0)
    inp = cc.inputs(case, oracle)
    got, path = run(ia, ctx, resident, case, inp, case.knobs, case.overlap)
    assert got.dtype == np.float32 and got.shape == (case.n,) + cc.SHAPES[case.shape]
    assert path == case.expect, 'the call reports %s, the table says %s' % (cc.path_names(path), cc.path_names(case.expect))
    against_reference(case, inp, oracle, got, 'as the table has it')
    if case.overlap:
        apart, apath = run(ia, ctx, resident, case, inp, case.knobs)
        assert apath & cc.SPLIT, 'separate buffers report ' + cc.path_names(apath)
        against_reference(case, inp, oracle, apart, 'separate buffers')
        same_bits(got, apart, cid + ' against separate buffers')
    if case.expect & cc.STORED:       # the table of the first call is there for the second
        again, apath = run(ia, ctx, resident, case, inp, case.knobs)
        assert apath == case.expect, 'the second call reports ' + cc.path_names(apath)
        same_bits(got, again, cid + ' against a second call')
    if case.expect & (cc.FRAMES_WG | cc.SPLIT | cc.STORED | cc.LENS_MAP):
        plain, ppath = run(ia, ctx, resident, case, inp, dict(case.knobs, **cc.PLAIN))
        assert not ppath & (cc.FRAMES_WG | cc.SPLIT | cc.STORED | cc.LENS_MAP) and \
            (ppath & cc.PER_FRAME or ppath & cc.TWO_LAUNCHES), 'the plain run reports ' + cc.path_names(ppath)
        against_reference(case, inp, oracle, plain, 'the plain run (%s)' % cc.path_names(ppath))
        kernels = cc.RESIDENT | cc.STREAMED | cc.SEP | cc.TWO_LAUNCHES
        if ppath & kernels == path & kernels:      # (another kernel: held to the values only)
            same_bits(got, plain, cid + ' against the plain run')
