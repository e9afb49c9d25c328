"""GPU: the entry points of csrc/conv.hip that take all four element types - ipa_extend_array_dev and
ipa_deinterleave_dev / ipa_interleave_dev - at every one of them, on the C ABI.  They move elements and compute
nothing: the results are asked bit for bit.

The frame is 5 x 67: one column past the 64-lane block of both kernels, and 5 rows where a block holds 4.
"""
import numpy as np
import pytest

pytestmark = pytest.mark.gpu

DTYPES = (np.uint8, np.uint16, np.float32, np.float64)
H, W = 5, 67
# the library's border mode -> numpy.pad's name for it
PAD = {'constant': 'constant', 'nearest': 'edge', 'reflect': 'symmetric', 'wrap': 'wrap', 'mirror': 'reflect'}
MODES = tuple(PAD)


@pytest.fixture(scope='module')
def ctx():
    import imgprocessor_amd
    return imgprocessor_amd.default_context(0)


def image(shape, dt):
    """every element different from its neighbours, no zero (the constant border writes zeros); the integer types
    over their whole range"""
    n = int(np.prod(shape))
    if np.dtype(dt).kind == 'u':
        top = np.iinfo(dt).max
        return (1 + (np.arange(n, dtype=np.int64) * 7919) % top).astype(dt).reshape(shape)
    return (np.random.default_rng(n).standard_normal(n) + 3.0 * np.arange(1, n + 1)).astype(dt).reshape(shape)


def bits(a):
    return np.ascontiguousarray(a).view(np.uint8)


@pytest.mark.parametrize('dt', DTYPES, ids=lambda d: np.dtype(d).name)
def test_extend_array(ctx, dt):
    """kernel (5, 3) - two columns and one row of padding per side -, every border mode along x against a different
    one along y: numpy.pad axis by axis (an index map per axis; a constant border on either axis is 0)"""
    from imgprocessor_amd import _lib, ops
    from imgprocessor_amd.device import dtype_id
    kx, ky = 5, 3
    px, py = kx // 2, ky // 2
    img = image((H, W), dt)
    src = ctx.to_device(img)
    guard = np.dtype(dt).type(201)
    for i, mx in enumerate(MODES):
        my = MODES[(i + 1) % len(MODES)]
        dp = W + 2 * px + 3
        dst = ctx.to_device(np.full((H + 2 * py, dp), guard, dt))
        rc = ctx._lib.ipa_extend_array_dev(ctx.handle, src.ptr, dtype_id(dt), H, W, W, kx, ky, ops.border_id(mx),
                                           ops.border_id(my), dst.ptr, dp)
        assert rc == _lib.OK, (mx, my, rc)
        want = np.pad(np.pad(img, ((0, 0), (px, px)), PAD[mx]), ((py, py), (0, 0)), PAD[my])
        got = dst.get()
        assert np.array_equal(bits(got[:, :W + 2 * px]), bits(want)), (mx, my)
        assert (got[:, W + 2 * px:] == guard).all(), 'wrote past the padded row'
    assert np.array_equal(bits(src.get()), bits(img))
    dst = ctx.to_device(np.full((H + 2 * py, W + 2 * px), guard, dt))
    rc = ctx._lib.ipa_extend_array_dev(ctx.handle, src.ptr, 99, H, W, W, kx, ky, 0, 0, dst.ptr, W + 2 * px)
    assert rc == _lib.ERR_BAD_ARG and (dst.get() == guard).all()     # unknown dtype


@pytest.mark.parametrize('dt', DTYPES, ids=lambda d: np.dtype(d).name)
def test_channel_layout(ctx, dt):
    """a 5 x 67 x 3 image with a padded interleaved pitch into planes with a padded row pitch and plane stride, and
    back: numpy.moveaxis, the round trip the identity, the guard elements of both paddings untouched"""
    from imgprocessor_amd import _lib
    from imgprocessor_amd.device import dtype_id
    ch = 3
    ipitch, ppitch = W * ch + 5, W + 3
    pstride = H * ppitch + 11
    guard = np.dtype(dt).type(201)
    img = image((H, W, ch), dt)
    inter = np.full((H, ipitch), guard, dt)
    inter[:, :W * ch] = img.reshape(H, W * ch)
    d_inter = ctx.to_device(inter)
    d_planes = ctx.to_device(np.full(ch * pstride, guard, dt))
    L, hnd, did = ctx._lib, ctx.handle, dtype_id(dt)
    assert L.ipa_deinterleave_dev(hnd, d_inter.ptr, did, H, W, ch, ipitch, d_planes.ptr, ppitch, pstride) == _lib.OK
    planes = d_planes.get()
    want = np.full(ch * pstride, guard, dt)
    for c in range(ch):
        want[c * pstride:c * pstride + H * ppitch].reshape(H, ppitch)[:, :W] = np.moveaxis(img, 2, 0)[c]
    assert np.array_equal(bits(planes), bits(want))     # the planes AND every guard element around them
    d_back = ctx.to_device(np.full((H, ipitch), guard, dt))
    assert L.ipa_interleave_dev(hnd, d_planes.ptr, did, H, W, ch, ppitch, pstride, d_back.ptr, ipitch) == _lib.OK
    assert np.array_equal(bits(d_back.get()), bits(inter))
    assert np.array_equal(bits(d_planes.get()), bits(want)) and np.array_equal(bits(d_inter.get()), bits(inter))
    for f, args in ((L.ipa_deinterleave_dev, (ipitch, d_planes.ptr, ppitch, pstride)),
                    (L.ipa_interleave_dev, (ppitch, pstride, d_back.ptr, ipitch))):
        src = d_inter if f is L.ipa_deinterleave_dev else d_planes
        assert f(hnd, src.ptr, 99, H, W, ch, *args) == _lib.ERR_BAD_ARG     # unknown dtype
    assert np.array_equal(bits(d_planes.get()), bits(want)) and np.array_equal(bits(d_back.get()), bits(inter))
