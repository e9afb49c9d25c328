"""CPU-only: what imgprocessor_amd.ops hands to the C ABI, recorded on a stub context instead of a
device.  ops needs four things of a context - handle, _check, _alloc and _lib - so a stub whose
_lib records (name, args) stands in for one: every public function of ops is called once with
host arrays and once with DeviceArrays built on the stub, and every recorded call must fit the
prototype it would have been marshalled through.

Shapes: sources 3 x 37 x 53 or 37 x 53, maps, grids and results 41 x 59, kernels 5 x 5 / 5 + 5."""
import ctypes as C
import inspect

import numpy as np
import pytest

from imgprocessor_amd import _lib, ops
from imgprocessor_amd.device import Context, DeviceArray

SRC, DST = (3, 37, 53), (41, 59)
COPIES = {'ipa_memcpy_h2d', 'ipa_memcpy_d2h', 'ipa_memcpy_d2d'}
# the exports that exist in a host-pointer and a device-pointer form
HOST_EXPORTS = {n[len('ipa_'):] for n in _lib.PROTOTYPES if n + '_dev' in _lib.PROTOTYPES}


class Tape(object):
    """stands in for the ctypes library: every ipa_* attribute records its call and returns IPA_OK"""

    def __init__(self):
        self.calls = []

    def __getattr__(self, name):
        if not name.startswith('ipa_'):
            raise AttributeError(name)
        return lambda *args: self.calls.append((name, args)) or 0


class StubContext(object):
    """a context without a device: allocations are distinct fake addresses, nothing is checked"""
    to_device, empty = Context.to_device, Context.empty

    def __init__(self):
        self._lib = Tape()
        self.handle = C.c_void_p(0x1000)
        self.allocs = []            # (address, bytes) in allocation order
        self._next = 1 << 32

    def _check(self, status, what=''):
        pass

    def _alloc(self, nbytes):
        self.allocs.append((self._next, nbytes))
        self._next += (nbytes + 8191) // 4096 * 4096
        return C.c_void_p(self.allocs[-1][0])

    def _release(self, ptr, nbytes):
        pass


def inputs():
    """the host arrays of every call below, C-contiguous and of the dtype the op takes as it is"""
    rng = np.random.default_rng(7)
    f = {}
    f['src'] = rng.random(SRC).astype(np.float32)
    f['img'] = np.ascontiguousarray(f['src'][0])
    f['img'][4, 6] = np.nan
    f['mapx'], f['mapy'] = (rng.random(DST) * 50).astype(np.float32), (rng.random(DST) * 35).astype(np.float32)
    f['k5'] = rng.random((5, 5))
    f['taps'] = rng.random(5)
    f['K'] = np.array([[53., 0, 26.0], [0, 53., 18.0], [0, 0, 1.0]])
    f['dist'] = np.array([-0.12, 0.03, 1e-3, -5e-4, 0.0])
    f['M'] = np.array([[0.9, 0.05, 1.5], [-0.04, 0.88, 2.0], [1e-4, -2e-4, 1.0]])
    f['rects'] = np.array([[0, 0, 30, 20], [30, 0, 29, 20], [0, 20, 59, 21]], np.int32)
    f['cellM'] = np.stack([f['M'], f['M'] + 0.01, np.eye(3)])
    f['mask'] = (rng.random(SRC[1:]) < 0.2).astype(np.uint8)
    f['grid'] = rng.random(DST).astype(np.float32)
    f['gmask'] = (rng.random(DST) < 0.2).astype(np.uint8)
    f['sig'] = 0.5 + rng.random(SRC[1:])
    f['rowk'] = rng.random((SRC[1], 3, 5))
    f['hwc'] = rng.random((37, 53, 3)).astype(np.float32)
    f['w7'] = rng.random((7, 7))
    f['offs'] = rng.integers(-3, 4, (12, 2)).astype(np.int32)
    f['w12'] = rng.random(12)
    f['pts'] = rng.random((3, 9)) * 40
    return f


# ops that exist for DeviceArrays only: host arrays are a TypeError
DEVICE_ONLY = {'from_planes', 'nan_to_zero', 'remap_conv2d', 'undistort_conv2d', 'warp_perspective_conv2d',
               'remap_sepconv2d', 'undistort_sepconv2d', 'warp_perspective_sepconv2d'}
# public functions that make no library call
NO_CALL = {'interp_id', 'border_id', 'gaussian_kernel1d'}


def cases(ctx, dev, f):
    """[(label, ops function, export it must reach without its _dev, thunk)] with every array argument in the
    host (dev False) or the device form"""
    up = ctx.to_device if dev else (lambda a: a.copy())
    src, img, mapx, mapy = up(f['src']), up(f['img']), up(f['mapx']), up(f['mapy'])
    mask, u8 = up(f['mask']), up(f['mask'])
    geo = dict(interpolation='cubic_cv', border_mode='reflect101', border_value=0.25, ctx=ctx)
    K, dist, M, k5, t = f['K'], f['dist'], f['M'], f['k5'], f['taps']
    x, y, v = f['pts']

    def state():
        return (ctx.to_device(np.zeros(SRC[1:])), DeviceArray.counts(ctx, SRC[1:]), ctx.to_device(np.zeros(SRC[1:])),
                ctx.to_device(f['mask']), ctx.to_device(f['mask']))

    def ste(mask=None):
        avg, count, thr, ms, mc = state()
        return ops.ste_update(src, avg, count, thr, first_pair=True, nlf=(0.01, 0.0, 0.1), mask=mask, mask_ste=ms,
                              mask_clean=mc, ctx=ctx)

    def fill(fn, *a, **kw):
        return lambda: fn(up(f['grid']), up(f['gmask']), *a, ctx=ctx, **kw)

    out = [
        ('to_planes', 'to_planes', 'deinterleave', lambda: ops.to_planes(up(f['hwc']), ctx=ctx)),
        ('from_planes', 'from_planes', 'interleave', lambda: ops.from_planes(src, ctx=ctx)),
        ('build_undistort_map', 'build_undistort_map', 'build_undistort_map',
         lambda: ops.build_undistort_map(K, dist, K, DST[0], DST[1], ctx=ctx, device=dev)),
        ('remap', 'remap', 'remap', lambda: ops.remap(src, mapx, mapy, out_dtype=np.float32, **geo)),
        ('undistort', 'undistort', 'undistort', lambda: ops.undistort(src, K, dist, out_shape=DST, **geo)),
        ('undistort same shape', 'undistort', 'undistort', lambda: ops.undistort(img, K, dist, K * 0.9, **geo)),
        ('warp_perspective', 'warp_perspective', 'warp_perspective', lambda: ops.warp_perspective(src, M, DST, **geo)),
        ('warp_grid_plan', 'warp_grid_plan', 'warp_grid_plan', lambda: ops.warp_grid_plan(f['rects'], DST)),
        ('warp_grid', 'warp_grid', 'warp_grid', lambda: ops.warp_grid(src, f['rects'], f['cellM'], DST, **geo)),
        ('conv2d', 'conv2d', 'conv2d', lambda: ops.conv2d(src, k5, mode='wrap', mode_y='mirror', cval=0.5, ctx=ctx)),
        ('conv2d mask', 'conv2d', 'conv2d', lambda: ops.conv2d(src, k5, mask=mask, ctx=ctx)),
        ('sepconv2d', 'sepconv2d', 'sepconv2d', lambda: ops.sepconv2d(src, t, t[::-1], ctx=ctx)),
        ('gaussian_filter', 'gaussian_filter', 'sepconv2d', lambda: ops.gaussian_filter(src, 1.0, ctx=ctx)),
        ('extend_array', 'extend_array', 'extend_array', lambda: ops.extend_array(img, (5, 3), 'wrap', ctx=ctx)),
        ('conv_ydep', 'conv_ydep', 'conv_ydep', lambda: ops.conv_ydep(img, f['rowk'], ctx=ctx)),
        ('var_y_gauss', 'var_y_gauss', 'var_y_gauss', lambda: ops.var_y_gauss(img, 0.5, 2.0, 5, t, ctx=ctx)),
        ('local_std', 'local_std', 'local_std', lambda: ops.local_std(img, up(f['img'] * 0.5), (5, 3), ctx=ctx)),
        ('nan_max', 'nan_max', 'nan_max', lambda: ops.nan_max(img, 5, ctx=ctx)),
        ('pos_intensity_unc', 'pos_intensity_unc', 'pos_intensity_unc',
         lambda: ops.pos_intensity_unc(img, 0.7, 1.1, 3, ctx=ctx)),
        ('pos_intensity_unc maps', 'pos_intensity_unc', 'pos_intensity_unc',
         lambda: ops.pos_intensity_unc(img, up(f['sig']), up(f['sig'] * 2), 3, ctx=ctx)),
        ('median_threshold', 'median_threshold', 'median_threshold_size',
         lambda: ops.median_threshold(img, 0.2, '<', ctx=ctx, size=5)),
        ('median_threshold no indices', 'median_threshold', 'median_threshold_size',
         lambda: ops.median_threshold(img, want_indices=False, ctx=ctx)),
        ('calib_prefilter', 'calib_prefilter', 'calib_prefilter',
         lambda: ops.calib_prefilter(img, up(f['img'] * 0.1), up(f['img'] + 1), 0.3, ctx=ctx)),
        ('calib_prefilter bare', 'calib_prefilter', 'calib_prefilter', lambda: ops.calib_prefilter(img, ctx=ctx)),
        ('closest_distance', 'closest_distance', 'closest_distance', lambda: ops.closest_distance(u8, 7, ctx=ctx)),
        ('closest_distance f64', 'closest_distance', 'closest_distance',
         lambda: ops.closest_distance(u8, 7, np.float64, ctx=ctx)),
        ('remove_single_pixels', 'remove_single_pixels', 'remove_single_pixels',
         lambda: ops.remove_single_pixels(u8, ctx=ctx)),
        ('ste_update', 'ste_update', 'ste', ste),
        ('ste_update mask', 'ste_update', 'ste', lambda: ste(mask)),
        ('nl_means', 'nl_means', 'nl_means', lambda: ops.nl_means(src, 5, 3, 0.2, 0.01, ctx=ctx)),
        ('nan_to_zero', 'nan_to_zero', 'nan_to_zero', lambda: ops.nan_to_zero(src)),
        ('remap_conv2d', 'remap_conv2d', 'remap_conv2d',
         lambda: ops.remap_conv2d(src, mapx, mapy, k5, conv_mode='wrap', **geo)),
        ('undistort_conv2d', 'undistort_conv2d', 'undistort_conv2d',
         lambda: ops.undistort_conv2d(src, K, dist, None, k5, out_shape=DST, **geo)),
        ('warp_perspective_conv2d', 'warp_perspective_conv2d', 'warp_perspective_conv2d',
         lambda: ops.warp_perspective_conv2d(src, M, DST, k5, **geo)),
        ('remap_sepconv2d', 'remap_sepconv2d', 'remap_sepconv2d',
         lambda: ops.remap_sepconv2d(src, mapx, mapy, t, t[::-1], conv_mode='mirror', **geo)),
        ('undistort_sepconv2d', 'undistort_sepconv2d', 'undistort_sepconv2d',
         lambda: ops.undistort_sepconv2d(img, K, dist, K * 0.9, t, t[::-1], **geo)),
        ('warp_perspective_sepconv2d', 'warp_perspective_sepconv2d', 'warp_perspective_sepconv2d',
         lambda: ops.warp_perspective_sepconv2d(src, M, DST, t, t[::-1], **geo)),
        ('idw_fill', 'idw_fill', 'idw_fill', fill(ops.idw_fill, 3, f['w7'])),
        ('fast_idw_fill', 'fast_idw_fill', 'fast_idw_fill', fill(ops.fast_idw_fill, f['offs'], f['w12'], 4)),
        ('unstructured_idw', 'unstructured_idw', 'unstructured_idw',
         lambda: ops.unstructured_idw(x, y, v, up(f['grid']), 3, ctx=ctx)),
        ('circular_idw_fill', 'circular_idw_fill', 'circular_idw_fill',
         fill(ops.circular_idw_fill, 4, 2, 1, 0.3, 21, 30)),
        ('cross_avg_fill', 'cross_avg_fill', 'cross_avg_fill', fill(ops.cross_avg_fill, 3, 1)),
        ('point_spread_idw', 'point_spread_idw', 'point_spread_idw', fill(ops.point_spread_idw, 3, max_iter=50)),
        ('resize', 'resize', 'resize', lambda: ops.resize(img, DST, 'lanczos4', ctx=ctx)),
        ('fast_filter_stat', 'fast_filter_stat', 'fast_filter_stat',
         lambda: ops.fast_filter_stat(img, 7, 3, 'nanmean', ctx=ctx)),
    ]
    for fn in ('mean', 'median'):
        for fm in (True, False):
            out.append(('masked_mean %s fill_mask=%s' % (fn, fm), 'masked_mean', 'masked_' + fn,
                        lambda fn=fn, fm=fm: ops.masked_mean(up(f['img']), mask, 5, fm, ctx=ctx, fn=fn)))
    if dev:
        out += [
            ('remap map_roi', 'remap', 'remap', lambda: ops.remap(src, mapx, mapy, map_roi=(3, 4, 20, 30), **geo)),
            ('remap out', 'remap', 'remap',
             lambda: ops.remap(src, mapx, mapy, out=ctx.empty((3,) + DST, np.float32), ctx=ctx)),
            ('resize src_shape', 'resize', 'resize', lambda: ops.resize(img, DST, 2, src_shape=(30, 40))),
            ('nl_means out', 'nl_means', 'nl_means', lambda: ops.nl_means(img, out=ctx.empty(img.shape, np.float32))),
        ]
    return out


@pytest.fixture
def stub(monkeypatch):
    ctx = StubContext()
    monkeypatch.setattr(_lib, 'lib', lambda: ctx._lib)   # warp_grid_plan takes no context
    return ctx


def run_case(ctx, thunk):
    del ctx._lib.calls[:], ctx.allocs[:]
    thunk()
    return list(ctx._lib.calls)


def check_call(name, args):
    """the call as ctypes would marshal it: right count, every argument accepted by its argtype"""
    assert name in _lib.PROTOTYPES, '%s has no prototype' % name
    proto = _lib.PROTOTYPES[name]
    assert len(args) == len(proto), '%s: %d arguments for %d parameters' % (name, len(args), len(proto))
    for i, (t, a) in enumerate(zip(proto, args)):
        try:
            t.from_param(a)
        except (TypeError, C.ArgumentError) as e:
            raise AssertionError('%s: argument %d (%r) is no %s: %s' % (name, i, a, t.__name__, e))


def test_the_check_refuses_what_ctypes_would():
    good = [C.c_void_p(1), C.c_void_p(2), 2, 37, 53, 53, 5, C.c_void_p(3), 41]
    check_call('ipa_nan_max_dev', good)
    for i, bad in ((4, 53.0), (7, np.zeros(3)), (5, 'x')):
        args = list(good)
        args[i] = bad
        with pytest.raises(AssertionError):
            check_call('ipa_nan_max_dev', args)
    with pytest.raises(AssertionError):
        check_call('ipa_nan_max_dev', good[:-1])
    with pytest.raises(AssertionError):
        check_call('ipa_nan_max', good)


def test_every_public_function_is_called():
    public = {n for n, fn in vars(ops).items()
              if inspect.isfunction(fn) and fn.__module__ == ops.__name__ and not n.startswith('_')}
    ctx = StubContext()
    called = {fn for _, fn, _, _ in cases(ctx, True, inputs())}
    assert called == public - NO_CALL
    exports = {e for _, _, e, _ in cases(ctx, True, inputs())}
    assert HOST_EXPORTS <= exports, 'host export without a case: %s' % (HOST_EXPORTS - exports)


@pytest.mark.parametrize('dev', [False, True], ids=['host', 'device'])
def test_calls_fit_their_prototypes_and_reach_the_right_export(stub, dev):
    for label, fn, export, thunk in cases(stub, dev, inputs()):
        if not dev and fn in DEVICE_ONLY:
            with pytest.raises(TypeError):
                thunk()
            continue
        calls = run_case(stub, thunk)
        for name, args in calls:
            check_call(name, args)
        want = export if (not dev and export in HOST_EXPORTS) or export == 'warp_grid_plan' else export + '_dev'
        got = {name for name, _ in calls} - COPIES
        assert got == {'ipa_' + want}, '%s (%s): reached %s' % (label, 'device' if dev else 'host', sorted(got))
        if not dev and export in HOST_EXPORTS:
            assert not stub.allocs, '%s: a host-pointer export needs no device array' % label


@pytest.mark.parametrize('dev', [False, True], ids=['host', 'device'])
def test_masked_fills_refuse_a_mask_of_another_shape(stub, dev):
    """the library reads h * w mask bytes: a 40 x 59 mask on a 41 x 59 grid is a ValueError, not a read past its end"""
    f = inputs()
    up = stub.to_device if dev else (lambda a: a.copy())
    fills = {
        'idw_fill': lambda g, m: ops.idw_fill(g, m, 3, f['w7'], ctx=stub),
        'fast_idw_fill': lambda g, m: ops.fast_idw_fill(g, m, f['offs'], f['w12'], 4, ctx=stub),
        'circular_idw_fill': lambda g, m: ops.circular_idw_fill(g, m, 4, ctx=stub),
        'cross_avg_fill': lambda g, m: ops.cross_avg_fill(g, m, 3, ctx=stub),
        'point_spread_idw': lambda g, m: ops.point_spread_idw(g, m, 3, ctx=stub),
    }
    for name, run in fills.items():
        del stub._lib.calls[:]
        with pytest.raises(ValueError):
            run(up(f['grid']), up(f['gmask'][:40]))
        assert not set(n for n, _ in stub._lib.calls) - COPIES, '%s reached the library' % name
        run(up(f['grid']), up(f['gmask']))          # the right shape passes
    if dev:
        for name, run in fills.items():
            with pytest.raises(ValueError):          # a device mask is read as bytes: uint8 only
                run(up(f['grid']), up(f['grid']))


# --------------------------------------------------------------- the calibration families
class PoolContext(StubContext):
    """a stub whose released blocks come back: pooled by size, last in first out, as Context._alloc
    and _release pool them.  An upload that is dropped before the call hands its address to the
    next allocation of that size."""

    def __init__(self):
        StubContext.__init__(self)
        self._pool = {}

    def _alloc(self, nbytes):
        blocks = self._pool.get(nbytes)
        return blocks.pop() if blocks else StubContext._alloc(self, nbytes)

    def _release(self, ptr, nbytes):
        self._pool.setdefault(nbytes, []).append(ptr)


CAL_N, CAL_HW, CAL_SMALL = 3, (37, 53), (4, 5)


def calibration_cases(ctx):
    """[(label, thunk)]: every calibration op once, every array argument a HOST array - the frames
    and all side arrays (bg, signal, noise, ascent, avg, small, obj, masks, the three TSS planes)"""
    rng = np.random.default_rng(11)
    h, w = CAL_HW
    img, img2, bg, sig, plane = (rng.random(CAL_HW) for _ in range(5))
    stack = (rng.random((CAL_N,) + CAL_HW) * 1000).astype(np.uint16)
    masks = (rng.random((CAL_N,) + CAL_HW) < 0.2).astype(np.uint8)
    times = np.arange(CAL_N, dtype=np.float64)
    mats = np.tile(np.eye(3), (CAL_N, 1, 1))
    edges = np.linspace(0.0, 1.0, 9)
    nlf = (0.01, 0.0, 0.1)
    return [
        ('nlf_signal bg', lambda: ops.nlf_signal(img, bg=bg, ctx=ctx)),
        ('nlf_signal pair bg', lambda: ops.nlf_signal(img, img2, bg=bg, ctx=ctx)),
        ('nlf_moments', lambda: ops.nlf_moments(img, ctx=ctx)),
        ('nlf_bins signal bg', lambda: ops.nlf_bins(img, sig, edges, 0.125, bg=bg, ctx=ctx)),
        ('nlf_bins pair signal bg', lambda: ops.nlf_bins(img, sig, edges, 0.125, img2=img2, bg=bg, ctx=ctx)),
        ('snr_map noise', lambda: ops.snr_map(sig, noise=plane, ctx=ctx)),
        ('snr_bg_median', lambda: ops.snr_bg_median(img, ctx=ctx)),
        ('pair_min', lambda: ops.pair_min(img, img2, ctx=ctx)),
        ('nlf_threshold', lambda: ops.nlf_threshold(img, nlf, ctx=ctx)),
        ('stack_linregress', lambda: ops.stack_linregress(times, stack, ctx=ctx)),
        ('dark_current_eval ascent', lambda: ops.dark_current_eval(img, plane, 2.0, 255, ctx=ctx)),
        ('cast_trunc', lambda: ops.cast_trunc(img, np.uint16, ctx=ctx)),
        ('stack_mean', lambda: ops.stack_mean(stack, ctx=ctx)),
        ('stack_mean list', lambda: ops.stack_mean(list(stack), ctx=ctx)),
        ('luma', lambda: ops.luma(rng.random(CAL_HW + (3,)), ctx=ctx)),
        ('strided_median_max', lambda: ops.strided_median_max(img, ctx=ctx)),
        ('strided_min', lambda: ops.strided_min(img, 3, 2, ctx=ctx)),
        ('flat_scale bg', lambda: ops.flat_scale(img, bg=bg, div=2.0, ctx=ctx)),
        ('nlf_lower_mask avg', lambda: ops.nlf_lower_mask(stack[0], plane, nlf, ctx=ctx)),
        ('sens_shrink bg', lambda: ops.sens_shrink(img, bg=bg, f=10, ctx=ctx)),
        ('sens_accumulate small bg', lambda: ops.sens_accumulate(
            img, rng.random(CAL_SMALL), ctx.to_device(np.zeros(CAL_HW)), bg=bg, first=True, ctx=ctx)),
        ('tss_event_length planes', lambda: ops.tss_event_length(
            stack, times, img, plane, sig, events=True, ctx=ctx, zero_mask=True)),
        ('tss_finish mask', lambda: ops.tss_finish(img, masks[0], ctx=ctx)),
        ('ovs_object ff', lambda: ops.ovs_object(rng.random((41, 59)), stack, mats, ctx=ctx)),
        ('ovs_flatfield obj masks', lambda: ops.ovs_flatfield(img, stack, masks, mats, (41, 59), ctx=ctx,
                                                              sub_step=10)),
        ('masked_running_mean_update', lambda: ops.masked_running_mean_update(
            img, np.ones(CAL_HW, np.int32), stack[0], masks[0], ctx=ctx)),
    ]


CAL_LABELS = [label for label, _ in calibration_cases(None)]


def test_every_calibration_op_has_a_host_case():
    names = set()
    for mod in ('ops_nlf', 'ops_dark', 'ops_flat', 'ops_tss', 'ops_ovs'):
        full = 'imgprocessor_amd.' + mod
        names |= {n for n, fn in vars(ops).items() if inspect.isfunction(fn) and fn.__module__ == full}
    assert names - {'nlf_params'} == {label.split()[0] for label in CAL_LABELS}


@pytest.mark.parametrize('label', CAL_LABELS)
def test_host_side_arrays_outlive_their_call(label):
    """Within one ipa_*_dev call no two arguments are the same allocation.  A host side array is
    uploaded into a temporary; if the wrapper lets go of it before the call, the pool hands its
    block to the result and the library sees the input and the output at one address."""
    ctx = PoolContext()
    dict(calibration_cases(ctx))[label]()
    blocks = {a for a, _ in ctx.allocs}
    dev_calls = [(n, a) for n, a in ctx._lib.calls if n.endswith('_dev')]
    assert dev_calls, '%s reached no device entry point' % label
    for name, args in dev_calls:
        check_call(name, args)
        got = [a.value for a in args if isinstance(a, C.c_void_p) and a.value in blocks]
        assert len(set(got)) == len(got), '%s: %s was handed one block twice: %s' % (
            label, name, ['%#x' % v for v in got])


def test_frame_stack_normalises_stacks_and_lists():
    from imgprocessor_amd._staging import frame_stack
    ctx = StubContext()
    rng = np.random.default_rng(5)
    host = (rng.random((CAL_N,) + CAL_HW) * 255).astype(np.uint8)
    # host: a stack as it is, a list through np.stack; nothing is allocated
    assert frame_stack('t', host) is host
    got = frame_stack('t', [f for f in host])
    assert isinstance(got, np.ndarray) and got.dtype == np.uint8 and np.array_equal(got, host)
    assert not ctx.allocs and not ctx._lib.calls
    # device: a stack as it is, a list gathered into ONE allocation by n device copies
    d_stack = ctx.to_device(host)
    assert frame_stack('t', d_stack) is d_stack
    frames = [ctx.to_device(f) for f in host]
    del ctx.allocs[:], ctx._lib.calls[:]
    st = frame_stack('t', frames)
    assert isinstance(st, DeviceArray) and st.shape == host.shape and st.dtype == np.uint8 and st.ctx is ctx
    assert ctx.allocs == [(st.ptr.value, host.nbytes)]
    copies = [(args[1].value, args[2].value, args[3]) for name, args in ctx._lib.calls if name == 'ipa_memcpy_d2d']
    assert [n for n, _ in ctx._lib.calls] == ['ipa_memcpy_d2d'] * CAL_N
    assert copies == [(st.ptr.value + k * host[0].nbytes, f.ptr.value, host[0].nbytes) for k, f in enumerate(frames)]
    # colour frames where the caller allows them
    rgb = [ctx.to_device(np.zeros(CAL_HW + (3,), np.float32)) for _ in range(2)]
    assert frame_stack('t', rgb, ndims=(2, 3)).shape == (2,) + CAL_HW + (3,)
    with pytest.raises(ValueError):
        frame_stack('t', rgb)
    with pytest.raises(ValueError):
        frame_stack('t', host[0])                                  # one frame is no stack
    # a mix is a TypeError, device frames of different shape or dtype a ValueError
    for mixed in ([frames[0], host[1]], [host[0], frames[1]]):
        with pytest.raises(TypeError):
            frame_stack('t', mixed)
    with pytest.raises(ValueError):
        frame_stack('t', [frames[0], ctx.to_device(host[1][:, :50])])
    with pytest.raises(ValueError):
        frame_stack('t', [frames[0], ctx.to_device(host[1].astype(np.uint16))])
    with pytest.raises(ValueError):
        frame_stack('t', [frames[0], StubContext().to_device(host[1])])
    with pytest.raises(ValueError):
        frame_stack('t', [host[0], host[1][:, :50]])


@pytest.mark.parametrize('family', ['ops_nlf', 'ops_dark', 'ops_flat', 'ops_tss', 'ops_ovs'])
def test_an_ops_family_imports_no_layer_built_on_it(family):
    import subprocess
    import sys
    code = ('import sys, imgprocessor_amd.%s\n'
            'up = [m for m in ("features", "camera", "uncertainty") if "imgprocessor_amd." + m in sys.modules]\n'
            'assert not up, up' % family)
    subprocess.check_call([sys.executable, '-c', code])
