"""GPU: object / vignetting separation (csrc/ovs.hip, camera/flatField/vignettingFromRandomSteps.py)
against the numpy restatement (tests/ovs_ref.py) driven by the project's own
ops.warp_perspective(float64, 'linear_cv_q5'): bit for bit - the taps are the same device function
and everything after them is correctly rounded IEEE arithmetic in a fixed order.  Counts with
array_equal.  (Oracle warps against device warps: test_vignetting_random_steps_warps, 1e-12.)

The kernels run through the C ABI with pitched rows and guard-valued padding at (object / flat
field) (1, 1) / (1, 1), (3, 67) / (5, 70) and (33, 130) / (41, 257) - more than one workgroup in
both directions -, with 1, 2, 5 and 64 frames of all four element types and the five matrices of
tests/ovs_cases.py; the planted values are checked to occur in the expected output.
"""
import hashlib

import numpy as np
import pytest

from . import ovs_cases as oc
from . import ovs_ref as ref
from .test_cpu_dark import same
from .test_gpu_dark import DT_ID, ERR_BAD_ARG, ERR_UNSUPPORTED, GUARD, dptr, padded, planes, unpad

pytestmark = pytest.mark.gpu

IGUARD = -77
SHAPE_IDS = ['%dx%d' % o for o, _ in oc.SHAPES]


@pytest.fixture(scope='module')
def ctx():
    import imgprocessor_amd
    return imgprocessor_amd.default_context(0)


def _ops():
    from imgprocessor_amd import ops
    return ops


@pytest.fixture(scope='module')
def warp(ctx):
    """the yardstick's warp: the parent commit's own launch, one call per distinct (image, matrix)"""
    ops, memo = _ops(), {}

    def w(src, M, shape):
        src = np.ascontiguousarray(src, dtype=np.float64)
        M = np.ascontiguousarray(M, dtype=np.float64)
        key = (hashlib.sha1(src.tobytes()).digest(), M.tobytes(), src.shape, tuple(shape))
        if key not in memo:
            out = ops.warp_perspective(src, M, (int(shape[0]), int(shape[1])), 'linear_cv_q5', 'constant', 0.0,
                                       ctx=ctx)
            out.setflags(write=False)
            memo[key] = out
        return memo[key]
    return w


def count_plane(ctx, h, pitch):
    from imgprocessor_amd import DeviceArray
    d = DeviceArray.counts(ctx, (h, pitch))
    d.set(np.full((h, pitch), IGUARD, np.int32))
    return d


def unpad_i(d, w):
    a = d.get()
    assert np.all(a[:, w:] == IGUARD), 'the padding was written'
    return a[:, :w]


def abi_object(ctx, ff, fits, M, n=None, dtype=None, fit_pitch=None, out=None):
    N, oh, ow = fits.shape
    fh, fw = ff.shape
    fp = ow + 3 if fit_pitch is None else fit_pitch
    d_ff = ctx.to_device(padded(ff, fw + 1, GUARD))
    d_fits = ctx.to_device(padded(fits, max(fp, ow)))
    d_obj, = planes(ctx, 1, oh, ow + 5)
    d_cnt = count_plane(ctx, oh, ow + 2)
    m = np.ascontiguousarray(M, dtype=np.float64)
    rc = ctx._lib.ipa_ovs_object_dev(
        ctx.handle, d_ff.ptr, fh, fw, fw + 1, d_fits.ptr, DT_ID[fits.dtype] if dtype is None else dtype,
        N if n is None else n, oh, ow, fp, oh * max(fp, ow), dptr(m),
        (d_obj if out is None else out(d_ff, d_fits)).ptr, ow + 5, d_cnt.ptr, ow + 2)
    return rc, d_obj, d_cnt


def abi_flatfield(ctx, obj, fits, masks, M, ff_shape, n=None, dtype=None, mask_pitch=None, out=None, clip=0,
                  sub_step=0):
    N, oh, ow = fits.shape
    fh, fw = ff_shape
    mp = ow + 4 if mask_pitch is None else mask_pitch
    d_obj = ctx.to_device(padded(obj, ow + 1, GUARD))
    d_fits = ctx.to_device(padded(fits, ow + 3))
    d_masks = ctx.to_device(padded(masks.astype(np.uint8), max(mp, ow), 1))
    d_ff, = planes(ctx, 1, fh, fw + 5)
    d_cnt = count_plane(ctx, fh, fw + 2)
    sh, sw = (-(-fh // sub_step), -(-fw // sub_step)) if sub_step else (1, 1)
    d_sub, = planes(ctx, 1, sh, sw + 1)
    m = np.ascontiguousarray(M, dtype=np.float64)
    rc = ctx._lib.ipa_ovs_flatfield_dev(
        ctx.handle, d_obj.ptr, ow + 1, d_fits.ptr, DT_ID[fits.dtype] if dtype is None else dtype,
        N if n is None else n, oh, ow, ow + 3, oh * (ow + 3), d_masks.ptr, mp, oh * max(mp, ow), dptr(m),
        (d_ff if out is None else out(d_obj, d_fits, d_masks)).ptr, fh, fw, fw + 5, d_cnt.ptr, fw + 2, clip,
        d_sub.ptr if sub_step else None, max(sub_step, 1), sw + 1)
    return rc, d_ff, d_cnt, d_sub


# ------------------------------------------------------------------ kernel (a)
@pytest.mark.parametrize('n', oc.N_VALUES)
@pytest.mark.parametrize('shapes', oc.SHAPES, ids=SHAPE_IDS)
def test_object_kernel(ctx, warp, shapes, n):
    obj_shape, ff_shape = shapes
    ff = oc.flat_field(ff_shape, 5)
    M = oc.pick(oc.matrices(ff_shape, obj_shape), n)
    for i, dt in enumerate(oc.ALL_DTYPES):
        fits = oc.fit_stack(n, obj_shape, dt, 100 + i)
        want, want_n = ref.ovs_object(warp, ff, list(fits), M)
        rc, d_obj, d_cnt = abi_object(ctx, ff, fits, M)
        ctx._check(rc, 'ovs_object')
        assert same(unpad(d_obj, obj_shape[1]), want), (shapes, n, dt)
        assert np.array_equal(unpad_i(d_cnt, obj_shape[1]), want_n), (shapes, n, dt)
        if n == 1:   # the fit that misses entirely
            assert not want_n.any() and not want.any()
    if shapes == oc.BIG and n >= 5:
        assert want_n.min() < want_n.max() < n and len(np.unique(want_n)) > 2   # (one of five fits misses)
        assert np.isnan(want).any()
    # the ops wrapper: host arrays, device arrays
    ops = _ops()
    got = ops.ovs_object(ff, fits, M, ctx=ctx)
    assert isinstance(got[0], np.ndarray) and same(got[0], want) and np.array_equal(got[1], want_n)
    assert got[1].dtype == np.int32
    if n <= 2:
        got = ops.ovs_object(ctx.to_device(ff), [ctx.to_device(f) for f in fits], M)
        assert same(got[0].get(), want) and np.array_equal(got[1].get(), want_n)


def test_object_kernel_planted_values(ctx, warp):
    obj_shape, ff_shape = oc.BIG
    ff = oc.flat_field(ff_shape, 5)
    mats = oc.matrices(ff_shape, obj_shape)
    fits = oc.fit_stack(1, obj_shape, np.float64, 7)
    zr = ff_shape[0] // 2
    # the identity: the zero block is rejected, the negative value, the NaN and the inf come through
    want, want_n = ref.ovs_object(warp, ff, list(fits), mats[[oc.IDENTITY]])
    assert not want_n[zr, 10:16].any() and not want[zr, 10:16].any() and want_n[zr, 9] == 1
    assert want[1, 20] < 0 and np.isnan(want[1, 30]) and want_n[1, 30] == 1
    assert want[1, 40] == 0 and want_n[1, 40] == 1 and fits[0, 1, 40] > 0     # x / inf
    rc, d_obj, d_cnt = abi_object(ctx, ff, fits, mats[[oc.IDENTITY]])
    ctx._check(rc, 'ovs_object')
    assert same(unpad(d_obj, obj_shape[1]), want) and np.array_equal(unpad_i(d_cnt, obj_shape[1]), want_n)
    # the integer translation (+1, +1): weights exactly 1 and 0 - a NaN or an inf under a zero weight
    # still poisons the pixel
    assert np.array_equal(mats[oc.TRANSLATION], [[1, 0, 1], [0, 1, 1], [0, 0, 1]])
    want, want_n = ref.ovs_object(warp, ff, list(fits), mats[[oc.TRANSLATION]])
    assert np.isnan(want[0, 28]) and np.isnan(want[0, 29]) and np.isnan(want[0, 38]) and want_n[0, 28] == 1
    assert np.isfinite(want[0, 27]) and want[0, 27] == fits[0, 0, 27] / ff[1, 28]
    rc, d_obj, d_cnt = abi_object(ctx, ff, fits, mats[[oc.TRANSLATION]])
    ctx._check(rc, 'ovs_object')
    assert same(unpad(d_obj, obj_shape[1]), want) and np.array_equal(unpad_i(d_cnt, obj_shape[1]), want_n)
    # the partial placement: pixels whose footprint lies wholly outside, and border footprints
    want, want_n = ref.ovs_object(warp, ff, list(fits), mats[[oc.PARTIAL]])
    assert (want_n == 0).any() and (want_n == 1).any()


# ------------------------------------------------------------------ kernel (b)
@pytest.mark.parametrize('n', oc.N_VALUES)
@pytest.mark.parametrize('shapes', oc.SHAPES, ids=SHAPE_IDS)
def test_flatfield_kernel(ctx, warp, shapes, n):
    obj_shape, ff_shape = shapes
    M = oc.pick(oc.matrices(obj_shape, ff_shape), n)
    masks = oc.mask_stack(n, obj_shape, 9)
    for i, dt in enumerate(oc.ALL_DTYPES):
        fits = oc.fit_stack(n, obj_shape, dt, 200 + i)
        obj = oc.object_image(obj_shape, dt, 300 + i)
        want, want_n = ref.ovs_flatfield(warp, obj, list(fits), list(masks), M, ff_shape)
        rc, d_ff, d_cnt, _ = abi_flatfield(ctx, obj, fits, masks, M, ff_shape)
        ctx._check(rc, 'ovs_flatfield')
        assert same(unpad(d_ff, ff_shape[1]), want), (shapes, n, dt)
        assert np.array_equal(unpad_i(d_cnt, ff_shape[1]), want_n), (shapes, n, dt)
        if n == 1:
            assert not want_n.any() and not want.any()
    if shapes == oc.BIG and n >= 5:
        assert want_n.min() == 0 and len(np.unique(want_n)) > 2
    # clipped, with the every-third-pixel grid of the unclipped result
    rc, d_ff, d_cnt, d_sub = abi_flatfield(ctx, obj, fits, masks, M, ff_shape, clip=1, sub_step=3)
    ctx._check(rc, 'ovs_flatfield')
    assert same(unpad(d_ff, ff_shape[1]), np.clip(want, 0, 1))
    assert same(unpad(d_sub, -(-ff_shape[1] // 3)), np.ascontiguousarray(want[::3, ::3]))
    # the ops wrapper
    ops = _ops()
    got = ops.ovs_flatfield(obj, fits, masks.astype(bool), M, ff_shape, ctx=ctx)
    assert len(got) == 2 and isinstance(got[0], np.ndarray) and same(got[0], want) and np.array_equal(got[1], want_n)
    if n <= 2:
        got = ops.ovs_flatfield(ctx.to_device(obj), ctx.to_device(fits), ctx.to_device(masks), M, ff_shape,
                                clip=True, sub_step=10)
        assert same(got[0].get(), np.clip(want, 0, 1)) and np.array_equal(got[1].get(), want_n)
        assert isinstance(got[2], np.ndarray) and same(got[2], np.ascontiguousarray(want[::10, ::10]))


@pytest.mark.parametrize('dtype', (np.float64, np.float32, np.uint16))
def test_flatfield_kernel_planted_values(ctx, warp, dtype):
    obj_shape, ff_shape = oc.BIG
    mats = oc.matrices(obj_shape, ff_shape)
    fits = oc.fit_stack(1, obj_shape, dtype, 11)
    masks = oc.mask_stack(1, obj_shape, 9)
    obj = oc.object_image(obj_shape, dtype, 12)
    zr = obj_shape[0] // 2
    assert not masks[0, zr - 1:zr + 2, 3:23].any(), 'the planted pixels are not masked'
    want, want_n = ref.ovs_flatfield(warp, obj, list(fits), list(masks), mats[[oc.IDENTITY]], ff_shape)
    # a positive fit over a zero of the object: inf, DBL_MAX after nan_to_num, accepted
    assert fits[0, zr - 1, 20] > 0 and want[zr - 1, 20] == oc.DBL_MAX and want_n[zr - 1, 20] == 1
    # (the integer types have no negative fit: their second zero of the object gives +inf too)
    n_inf = 1 if np.dtype(dtype).kind == 'f' else 2
    assert (want == oc.DBL_MAX).sum() == n_inf, 'with a zero weight on the inf the sample is NaN, not inf'
    # 0 / 0: NaN, 0 after nan_to_num, rejected - and so is every pixel whose footprint touches it
    assert fits[0, zr, 5] == 0 and want_n[zr, 5] == 0 and want[zr, 5] == 0 and want_n[zr, 4] == 0
    # a zero fit over a positive object is an exact 0: rejected
    assert fits[0, zr, 6] == 0 and obj[zr, 6] > 0 and want_n[zr, 6] == 0
    if np.dtype(dtype).kind == 'f':
        assert fits[0, zr, 12] < 0 and want[zr, 12] == -oc.DBL_MAX and want_n[zr, 12] == 1
    # masked pixels next to unmasked ones; the flat field beyond the object
    assert want_n[3, 3] == 1 and want_n[2, 3] == 0 and want_n[3, 2] == 0
    assert not want_n[obj_shape[0]:].any() and not want_n[:, obj_shape[1]:].any()
    rc, d_ff, d_cnt, _ = abi_flatfield(ctx, obj, fits, masks, mats[[oc.IDENTITY]], ff_shape)
    ctx._check(rc, 'ovs_flatfield')
    assert same(unpad(d_ff, ff_shape[1]), want) and np.array_equal(unpad_i(d_cnt, ff_shape[1]), want_n)
    # the integer translation (-1, -1): a masked pixel under a zero weight poisons its neighbour
    want, want_n = ref.ovs_flatfield(warp, obj, list(fits), list(masks), mats[[oc.TRANSLATION]], ff_shape)
    assert want_n[4, 4] == 1 and want_n[3, 4] == 0 and (want == oc.DBL_MAX).sum() == n_inf
    rc, d_ff, d_cnt, _ = abi_flatfield(ctx, obj, fits, masks, mats[[oc.TRANSLATION]], ff_shape)
    ctx._check(rc, 'ovs_flatfield')
    assert same(unpad(d_ff, ff_shape[1]), want) and np.array_equal(unpad_i(d_cnt, ff_shape[1]), want_n)
    # rotation and the partial placement: border footprints and footprints wholly outside
    for k in (oc.ROTATION, oc.PARTIAL):
        want, want_n = ref.ovs_flatfield(warp, obj, list(fits), list(masks), mats[[k]], ff_shape)
        assert (want_n == 0).any() and (want_n == 1).any()


# ------------------------------------------------------------------ kernel (c)
@pytest.mark.parametrize('shapes', oc.SHAPES, ids=SHAPE_IDS)
def test_masked_running_mean(ctx, shapes):
    from imgprocessor_amd import DeviceArray
    ops = _ops()
    h, w = shapes[1]
    rng = np.random.default_rng(21)
    for i, dt in enumerate(oc.ALL_DTYPES):
        avg, n = np.zeros((h, w)), np.zeros((h, w), np.int32)
        d_avg = ctx.to_device(padded(avg, w + 3, GUARD))
        d_n = count_plane(ctx, h, w + 1)
        d_n.set(padded(n, w + 1, IGUARD))
        h_avg, h_n = avg, n
        v_avg, v_n = ctx.to_device(avg), DeviceArray.counts(ctx, (h, w))
        v_n.set(n)
        for step in range(3):
            data = oc.fit_stack(1, (h, w), dt, 400 + 10 * i + step)[0]
            mask = rng.random((h, w)) < 0.6
            if h * w > 4:
                mask[0, 1] = False          # never accepted
                mask[0, 2] = step == 1      # accepted once
            avg, n = ref.masked_running_mean(avg, n, data, mask)
            d_data = ctx.to_device(padded(data, w + 2))
            d_mask = ctx.to_device(padded(mask.astype(np.uint8), w + 4, 1))
            ctx._check(ctx._lib.ipa_masked_running_mean_dev(
                ctx.handle, d_avg.ptr, w + 3, d_n.ptr, w + 1, d_data.ptr, DT_ID[np.dtype(dt)], w + 2, d_mask.ptr,
                w + 4, h, w), 'masked_running_mean')
            assert same(unpad(d_avg, w), avg) and np.array_equal(unpad_i(d_n, w), n), (shapes, dt, step)
            h_avg, h_n = ops.masked_running_mean_update(h_avg, h_n, data, mask, ctx=ctx)
            assert same(h_avg, avg) and np.array_equal(h_n, n) and h_n.dtype == np.int32
            out = ops.masked_running_mean_update(v_avg, v_n, ctx.to_device(data), ctx.to_device(mask.astype(np.uint8)))
            assert out[0] is v_avg and out[1] is v_n and same(v_avg.get(), avg) and np.array_equal(v_n.get(), n)
        if h * w > 4:
            assert n[0, 1] == 0 and avg[0, 1] == 0 and n[0, 2] == 1 and n.max() == 3
    # no mask: everywhere
    data = oc.fit_stack(1, (h, w), np.float32, 450)[0]
    avg, n = ref.masked_running_mean(avg, n, data, None)
    got = ops.masked_running_mean_update(h_avg, h_n, data, ctx=ctx)
    assert same(got[0], avg) and np.array_equal(got[1], n)
    # in place on the data is refused
    d = ctx.to_device(avg)
    cnt = DeviceArray.counts(ctx, (h, w))
    assert ctx._lib.ipa_masked_running_mean_dev(ctx.handle, d.ptr, w, cnt.ptr, w, d.ptr, 3, w, None, w, h, w) \
        == ERR_BAD_ARG
    assert ctx._lib.ipa_masked_running_mean_dev(ctx.handle, d.ptr, w, cnt.ptr, w, d_data.ptr, 9, w + 2, None, w, h,
                                                w) == ERR_UNSUPPORTED
    assert ctx._lib.ipa_masked_running_mean_dev(ctx.handle, d.ptr, w - 1, cnt.ptr, w, d_data.ptr, 2, w + 2, None, w,
                                                h, w) == ERR_BAD_ARG
    assert same(d.get(), avg)


# ------------------------------------------------------------------ refusals
def test_refusals_write_nothing(ctx):
    obj_shape, ff_shape = oc.SHAPES[1]
    oh, ow = obj_shape
    ff = oc.flat_field(ff_shape, 5)
    fits = oc.fit_stack(2, obj_shape, np.float64, 1)
    masks = oc.mask_stack(2, obj_shape, 2)
    obj = oc.object_image(obj_shape, np.float64, 3)
    M = oc.pick(oc.matrices(ff_shape, obj_shape), 2)
    M65 = np.tile(np.eye(3), (65, 1, 1))
    f65 = np.zeros((65,) + obj_shape, np.float32)

    def guard_a(rc, d_obj, d_cnt):
        ctx.synchronize()
        assert np.all(d_obj.get() == GUARD) and np.all(d_cnt.get() == IGUARD), 'a refused call wrote its outputs'
        return rc

    def guard_b(rc, d_ff, d_cnt, d_sub):
        ctx.synchronize()
        assert np.all(d_ff.get() == GUARD) and np.all(d_cnt.get() == IGUARD) and np.all(d_sub.get() == GUARD)
        return rc

    assert guard_a(*abi_object(ctx, ff, fits, M, n=0)) == ERR_BAD_ARG
    assert guard_a(*abi_object(ctx, ff, f65, M65)) == ERR_UNSUPPORTED
    assert guard_a(*abi_object(ctx, ff, fits, M, fit_pitch=ow - 1)) == ERR_BAD_ARG
    assert guard_a(*abi_object(ctx, ff, fits, M, dtype=7)) == ERR_UNSUPPORTED
    assert guard_a(*abi_object(ctx, ff, fits, M, out=lambda d_ff, d_fits: d_fits)) == ERR_BAD_ARG
    assert guard_a(*abi_object(ctx, ff, fits, M, out=lambda d_ff, d_fits: d_ff)) == ERR_BAD_ARG
    rc, d_obj, d_cnt = abi_object(ctx, ff, fits, M)
    assert rc == 0 and not np.all(d_obj.get() == GUARD)

    Mb = oc.pick(oc.matrices(obj_shape, ff_shape), 2)
    m65 = np.zeros((65,) + obj_shape, np.uint8)
    assert guard_b(*abi_flatfield(ctx, obj, fits, masks, Mb, ff_shape, n=0, sub_step=2)) == ERR_BAD_ARG
    assert guard_b(*abi_flatfield(ctx, obj, f65, m65, M65, ff_shape, sub_step=2)) == ERR_UNSUPPORTED
    assert guard_b(*abi_flatfield(ctx, obj, fits, masks, Mb, ff_shape, mask_pitch=ow - 1, sub_step=2)) == ERR_BAD_ARG
    assert guard_b(*abi_flatfield(ctx, obj, fits, masks, Mb, ff_shape, dtype=-1, sub_step=2)) == ERR_UNSUPPORTED
    for pick_in in range(3):
        assert guard_b(*abi_flatfield(ctx, obj, fits, masks, Mb, ff_shape, sub_step=2,
                                      out=lambda *ins: ins[pick_in])) == ERR_BAD_ARG, pick_in
    rc, d_ff, d_cnt, d_sub = abi_flatfield(ctx, obj, fits, masks, Mb, ff_shape, sub_step=2)
    assert rc == 0 and not np.all(d_sub.get()[:, :-1] == GUARD)
    ops = _ops()
    with pytest.raises(NotImplementedError):
        ops.ovs_object(ff, f65, M65, ctx=ctx)
    with pytest.raises(ValueError):
        ops.ovs_flatfield(obj, fits, masks[:1], Mb, ff_shape, ctx=ctx)


# ------------------------------------------------------------------ the class
def V():
    from imgprocessor_amd.camera.flatField import vignettingFromRandomSteps
    return vignettingFromRandomSteps


def _filled(sc, ctx, dev, with_imgs=False, **kw):
    s = V().ObjectVignettingSeparation(sc['ff0'].shape, sc['fits'].shape[1:], ctx=ctx, **kw)
    up = ctx.to_device if dev else (lambda a: a)
    for k in range(len(sc['fits'])):
        extra = dict(img=up(sc['imgs'][k]), img_mask=up(sc['img_masks'][k].astype(np.uint8))) if with_imgs else {}
        s.addFit(up(sc['fits'][k]), up(sc['masks'][k].astype(np.uint8)), sc['Hs'][k], **extra)
    return s


def _host(a):
    return a if isinstance(a, np.ndarray) else a.get()


@pytest.mark.parametrize('dtype', (np.float64, np.uint16))
def test_one_step_host_and_device_frames(ctx, warp, dtype, capsys):
    from imgprocessor_amd import DeviceArray
    sc = oc.loop_scene(dtype=dtype)
    want = ref.Separation(warp, sc['ff0'], list(sc['fits']), list(sc['masks']), list(sc['Hs']))
    next(iter(want))
    got = []
    for dev in (False, True):
        s = _filled(sc, ctx, dev)
        assert len(s.Hs) == len(s.Hinvs) == 6 and same(s.Hinvs[2], np.linalg.inv(sc['Hs'][2]))
        s.flatField = ctx.to_device(sc['ff0']) if dev else sc['ff0']
        assert next(iter(s)) == 1
        assert isinstance(s.flatField, DeviceArray if dev else np.ndarray)
        assert isinstance(s.object, DeviceArray if dev else np.ndarray)
        got.append((_host(s.flatField), _host(s.object)))
        assert same(got[-1][0], want.flatField) and same(got[-1][1], want.object), dev
    assert same(got[0][0], got[1][0]) and same(got[0][1], got[1][1])
    out = capsys.readouterr().out.splitlines()
    assert out == ['residuum: %s' % want.residua[0]] * 2


@pytest.fixture(scope='module')
def loop_reference(warp):
    sc = oc.loop_scene()
    s = ref.Separation(warp, sc['ff0'], list(sc['fits']), list(sc['masks']), list(sc['Hs']))
    s.run()
    return s.residua


@pytest.mark.parametrize('case', ('maxIter0', 'maxIter1', 'maxIter10', 'early'))
def test_separate(ctx, warp, loop_reference, case, capsys):
    sc = oc.loop_scene()
    r = loop_reference
    kw = {'maxIter0': dict(max_iter=0), 'maxIter1': dict(max_iter=1), 'maxIter10': dict(max_iter=10),
          'early': dict(max_dev=0.5 * (r[2] + r[3]))}[case]
    want = ref.Separation(warp, sc['ff0'], list(sc['fits']), list(sc['masks']), list(sc['Hs']), **kw)
    want.run()
    s = _filled(sc, ctx, False, maxIter=kw.get('max_iter', 10), maxDev=kw.get('max_dev', 1e-4))
    s.flatField = sc['ff0']
    capsys.readouterr()
    ff, obj = s.separate()
    lines = capsys.readouterr().out.splitlines()
    assert [ln for ln in lines if ln.startswith('residuum')] == ['residuum: %s' % d for d in want.residua]
    assert s.n == want.n == {'maxIter0': 0, 'maxIter1': 1, 'maxIter10': 10, 'early': 3}[case]
    assert sum(ln.startswith('iteration step') for ln in lines) == want.n
    assert same(ff, want.flatField) and same(obj, want.object)
    assert same(s.flatField, want.flatField) and same(s.object, want.object)
    if case == 'early':
        assert s.n < s.maxIter
    if case == 'maxIter0':
        assert same(ff, sc['ff0'])


def test_initial_flat_field_from_the_images(ctx, warp, capsys):
    from imgprocessor_amd.filters.fastFilter import fastFilter
    sc = oc.loop_scene(dtype=np.uint16)
    mma = ref.MaskedMovingAverage(sc['ff0'].shape)
    for img, m in zip(sc['imgs'], sc['img_masks']):
        mma.update(img, m)
    assert mma.n.min() == 0 and mma.n.max() > 1
    f = int(max(sc['ff0'].shape) / 9)
    ff0 = fastFilter(mma.avg, f, int(f / 3.5), ctx=ctx)
    ff0 /= ff0.max()
    for dev in (False, True):
        s = _filled(sc, ctx, dev, with_imgs=True, maxIter=2)
        assert same(s._ff_avg.get(), mma.avg) and np.array_equal(s._ff_n.get(), mma.n)
        assert same(s._createInitialflatField(), ff0)
        want = ref.Separation(warp, ff0, list(sc['fits']), list(sc['masks']), list(sc['Hs']), max_iter=2)
        want.run()
        ff, obj = s.separate()
        assert same(_host(ff), want.flatField) and same(_host(obj), want.object) and s.n == 2
    s = _filled(sc, ctx, False)
    with pytest.raises(ValueError):
        s.separate()
