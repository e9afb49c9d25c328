"""GPU: the structured IDW fills (csrc/idw.hip) on the case table of tests/idw_cases.py, each
case on a branch that test_cpu_idw_refs.py has proven it stands on, against the float64
references with exact sums of tests/idw_ref.py.

fast_idw_kernel   a stop by hit at neighbour 63 | 64 | 65 and 127 | 128 and in later batches of 64
                  (the hit count carried from batch to batch), a far-outside stop in the first and
                  in a later batch, a far-outside neighbour before any hit, both kinds of stop in
                  one batch in both orders, walks to the end of 80, 288 and 1088 = 17 x 64
                  neighbours, minnvals 1 and beyond the window, nothing unmasked in reach
idw_kernel        k = 1, 7 | 8, 15 | 16, 31 | 32: lanes over the taps | over the columns of a
                  window row, two rows per pass | one | taps again; grids smaller than the window,
                  widths 64 | 65 and 128 | 129, masked corners, a fully masked window, a NaN
                  among the neighbours, a weight table whose centre entry is not zero
Both in float32 and float64, through ops.* on host arrays and through the *_dev entry points on a
grid of pitch w + 7 whose padding would ruin any mean and must be unchanged afterwards.

Tolerance (idw_ref.bound_abs), derived: positive weights, so the quotient of two float64 sums of
n terms in any order is within (n + 2) 2^-53 sum(w |g|) / sum(w) of the exact one; float32 grids
add half a unit in the last place of the float32 result.  Worst err / bound, printed per case
and summed up by test_worst_figures, measured on the MI355X:
  fast IDW  float32 1.00 (the store's rounding, which the bound grants once)   float64 0.47
  IDW fill  float32 1.00 (the same)                                            float64 0.33
"""
import numpy as np
import pytest

from . import idw_cases as ic
from . import idw_ref as ref

pytestmark = pytest.mark.gpu

_worst = {}


@pytest.fixture(scope='module')
def ctx():
    import imgprocessor_amd
    return imgprocessor_amd.default_context(0)


def _dt(dtype):
    from imgprocessor_amd.device import dtype_id
    return dtype_id(dtype)


def _note(kind, dtype, r):
    key = (kind, np.dtype(dtype).name)
    _worst[key] = max(_worst.get(key, 0.0), r)


def _held(got, g, res, dtype, kind, what):
    """got against the reference under the bound; pixels that were not filled keep their bits"""
    r = ref.worst(got, res, dtype)
    u = np.uint32 if dtype == np.float32 else np.uint64
    keep = ~res['filled']
    assert np.array_equal(got.view(u)[keep], g.view(u)[keep]), what + ': bits of an unfilled pixel changed'
    print('%s %s %s: worst err / bound %.3g' % (kind, what, np.dtype(dtype).name, r))
    assert r <= 1.0, '%s %s: err / bound %.3g' % (kind, what, r)
    _note(kind, dtype, r)


def _pitched_run(ctx, g, mask, call):
    big = ic.pitched(g)
    d, dm = ctx.to_device(big), ctx.to_device(np.ascontiguousarray(mask, dtype=np.uint8))
    ctx._check(call(d, dm, big.shape[1]))
    out = d.get()
    u = np.uint32 if g.dtype == np.float32 else np.uint64
    assert np.array_equal(out[:, g.shape[1]:].view(u), big[:, g.shape[1]:].view(u)), 'the padding changed'
    return np.ascontiguousarray(out[:, :g.shape[1]])


@pytest.mark.parametrize('dtype', [np.float32, np.float64])
@pytest.mark.parametrize('case', ic.FAST, ids=[c['name'] for c in ic.FAST])
def test_fast_idw_classes(ctx, case, dtype):
    from imgprocessor_amd import ops
    g, res = ic.fast_ref(case, dtype)
    offs, wts = ic.fast_args(case)
    h, w = case['shape']
    got = ops.fast_idw_fill(g.copy(), case['mask'], offs, wts, case['minnvals'], ctx=ctx)
    _held(got, g, res, dtype, 'fast', case['name'])
    o32 = np.ascontiguousarray(offs, dtype=np.int32)
    wc = np.ascontiguousarray(wts, dtype=np.float64)
    got = _pitched_run(ctx, g, case['mask'], lambda d, dm, pitch: ctx._lib.ipa_fast_idw_fill_dev(
        ctx.handle, d.ptr, _dt(dtype), dm.ptr, h, w, pitch, o32.ctypes.data, wc.ctypes.data_as(ops.C.POINTER(
            ops.C.c_double)), len(wc), case['minnvals']))
    _held(got, g, res, dtype, 'fast', case['name'] + ' pitched')


@pytest.mark.parametrize('dtype', [np.float32, np.float64])
@pytest.mark.parametrize('case', ic.IDW, ids=[c['name'] for c in ic.IDW])
def test_idw_fill_kernels(ctx, case, dtype):
    from imgprocessor_amd import ops
    g, wts, res = ic.idw_ref_of(case, dtype)
    h, w = case['shape']
    k = case['k']
    what = '%s (%s, %d rows per pass)' % ((case['name'],) + case['kernel'])
    got = ops.idw_fill(g.copy(), case['mask'], k, wts, ctx=ctx)
    _held(got, g, res, dtype, 'idw', what)
    wc = np.ascontiguousarray(wts, dtype=np.float64)
    got = _pitched_run(ctx, g, case['mask'], lambda d, dm, pitch: ctx._lib.ipa_idw_fill_dev(
        ctx.handle, d.ptr, _dt(dtype), dm.ptr, h, w, pitch, k, wc.ctypes.data_as(ops.C.POINTER(ops.C.c_double))))
    _held(got, g, res, dtype, 'idw', what + ' pitched')


def test_worst_figures():
    """the figures of the module docstring, printed after the cases above have run"""
    for key in sorted(_worst):
        print('%s %s: worst err / bound %.3g' % (key + (_worst[key],)))
    assert all(v <= 1.0 for v in _worst.values())


def test_refusals_write_nothing(ctx):
    """ksize 0 and 513, an integer grid, minnvals -1: refused on the host before any launch"""
    from imgprocessor_amd import _lib as L, ops
    h, w = 6, 9
    g = np.full((h, w), -5.0)
    d, dm = ctx.to_device(g), ctx.to_device(np.ones((h, w), np.uint8))
    di = ctx.to_device(np.full((h, w), 7, np.uint16))
    one = np.ones(1027 * 1027)
    wp = one.ctypes.data_as(ops.C.POINTER(ops.C.c_double))
    offs = np.ascontiguousarray(ref.neighbours_of(2)[0], dtype=np.int32)
    lib = ctx._lib
    for ksize in (0, 513):
        assert lib.ipa_idw_fill_dev(ctx.handle, d.ptr, _dt(np.float64), dm.ptr, h, w, w, ksize, wp) == L.ERR_BAD_ARG
    assert lib.ipa_idw_fill_dev(ctx.handle, di.ptr, _dt(np.uint16), dm.ptr, h, w, w, 2, wp) != L.OK
    assert lib.ipa_fast_idw_fill_dev(ctx.handle, di.ptr, _dt(np.uint16), dm.ptr, h, w, w, offs.ctypes.data, wp,
                                     24, 4) != L.OK
    assert lib.ipa_fast_idw_fill_dev(ctx.handle, d.ptr, _dt(np.float64), dm.ptr, h, w, w, offs.ctypes.data, wp,
                                     24, -1) == L.ERR_BAD_ARG
    assert lib.ipa_idw_fill_dev(ctx.handle, d.ptr, _dt(np.float64), dm.ptr, h, w, w - 1, 2, wp) == L.ERR_BAD_ARG
    with pytest.raises(ValueError):
        ops.idw_fill(g.copy(), np.ones((h, w), bool), 0, np.ones((1, 1)), ctx=ctx)
    with pytest.raises(ValueError):
        ops.fast_idw_fill(g.copy(), np.ones((h, w), bool), offs, np.ones(24), -1, ctx=ctx)
    ctx.synchronize()
    assert np.array_equal(d.get(), g) and (di.get() == 7).all(), 'something was launched'
