"""GPU: every host-pointer export of the C ABI (numpy arrays staged through the context's workspace by
ipa_stage_in / ipa_stage_out, csrc/runtime.hip) gives byte for byte what its `_dev` twin gives on
DeviceArrays - the eighteen exports, reached through ops.*.

Shapes: sources 3 x 37 x 53, results and maps 41 x 59 (odd, more than one block, no multiple of a tile).
The fills, resize and fast_filter_stat take one 2-D array: grids 41 x 59, sources 37 x 53; INTER_AREA only
shrinks, so its result is 23 x 31 (scales 37 / 23 and 53 / 31: not integers)."""
import numpy as np
import pytest

from .gpu_helpers import frames, rot_maps, kern

pytestmark = pytest.mark.gpu

SRC, DST = (3, 37, 53), (41, 59)


@pytest.fixture(scope='module')
def ia():
    import imgprocessor_amd
    imgprocessor_amd.default_context(0)  # raises without a gfx950 device: no fallback
    return imgprocessor_amd


def same_bytes(host, dev, what):
    dev = dev.get() if hasattr(dev, 'get') else dev
    assert host.dtype == dev.dtype and host.shape == dev.shape, what
    assert host.tobytes() == dev.tobytes(), '%s: host-pointer and device results differ' % what


def _src(dtype, shape=SRC):
    f = frames(shape[0], shape[1], shape[2])
    if dtype == np.uint8:
        return np.round(f * 255).astype(np.uint8)
    if dtype == np.uint16:
        return np.round(f * 4095).astype(np.uint16)
    return f


_K = np.array([[53., 0, 26.0], [0, 53., 18.0], [0, 0, 1.0]])
_DIST = np.array([-0.12, 0.03, 1e-3, -5e-4, 0.0])
_M = np.array([[0.9, 0.05, 1.5], [-0.04, 0.88, 2.0], [1e-4, -2e-4, 1.0]])


def _cells():
    rects = np.array([[0, 0, 30, 20], [30, 0, 29, 20], [0, 20, 59, 21]], np.int32)
    M = np.stack([_M, _M + 0.01, np.eye(3)])
    return rects, M


@pytest.mark.parametrize('dtype', [np.float32, np.uint8, np.uint16])
def test_remaps(ia, dtype):
    ops, ctx = ia.ops, ia.default_context(0)
    src = _src(dtype)
    d_src = ctx.to_device(src)
    mx, my = rot_maps(DST[0], DST[1], 7.0)
    mx, my = mx * np.float32(53 / 59.), my * np.float32(37 / 41.)
    mx[3, 5] = np.nan                       # NaN coordinates (and, float32: NaN results) count as bytes
    if dtype == np.float32:
        src[1, 4, 4] = np.nan
        d_src = ctx.to_device(src)
    rects, cm = _cells()
    for interp in ('linear', 'cubic_cv', 'lanczos4'):
        kw = dict(interpolation=interp, border_mode='reflect101')
        same_bytes(ops.remap(src, mx, my, **kw), ops.remap(d_src, ctx.to_device(mx), ctx.to_device(my), **kw),
                   'remap %s' % interp)
        same_bytes(ops.undistort(src, _K, _DIST, out_shape=DST, **kw),
                   ops.undistort(d_src, _K, _DIST, out_shape=DST, **kw), 'undistort %s' % interp)
        same_bytes(ops.warp_perspective(src, _M, DST, **kw), ops.warp_perspective(d_src, _M, DST, **kw),
                   'warp_perspective %s' % interp)
        same_bytes(ops.warp_grid(src, rects, cm, DST, **kw), ops.warp_grid(d_src, rects, cm, DST, **kw),
                   'warp_grid %s' % interp)


def test_build_undistort_map(ia):
    ops = ia.ops
    hx, hy = ops.build_undistort_map(_K, _DIST, _K, *DST)
    dx, dy = ops.build_undistort_map(_K, _DIST, _K, *DST, device=True)
    same_bytes(hx, dx, 'map x')
    same_bytes(hy, dy, 'map y')


def test_filters(ia):
    ops, ctx = ia.ops, ia.default_context(0)
    src = _src(np.float32)
    src[2, 30, 7] = np.nan
    d_src = ctx.to_device(src)
    mask = (np.random.default_rng(3).random(SRC[1:]) < 0.2).astype(np.uint8)
    k = kern(5)
    same_bytes(ops.conv2d(src, k), ops.conv2d(d_src, k), 'conv2d')
    same_bytes(ops.conv2d(src, k, mask=mask), ops.conv2d(d_src, k, mask=ctx.to_device(mask)), 'conv2d, mask')
    g = ops.gaussian_kernel1d(1.0)
    same_bytes(ops.sepconv2d(src, g, g), ops.sepconv2d(d_src, g, g), 'sepconv2d')
    one = np.ascontiguousarray(src[0])
    same_bytes(ops.fast_filter_stat(one, 7, 3), ops.fast_filter_stat(ctx.to_device(one), 7, 3), 'fast_filter_stat')


def test_resize(ia):
    ops, ctx = ia.ops, ia.default_context(0)
    one = np.ascontiguousarray(_src(np.float32)[0])
    d_one = ctx.to_device(one)
    for interp, dsize in (('linear', DST), ('area', (23, 31)), ('lanczos4', DST)):
        same_bytes(ops.resize(one, dsize, interp), ops.resize(d_one, dsize, interp), 'resize %s' % interp)
    # the same shape again: ipa_resize_dev finds its tables of the call before on the device
    first = ops.resize(one, DST, 'lanczos4')
    second = ops.resize(one, DST, 'lanczos4')
    want = ops.resize(d_one, DST, 'lanczos4')
    same_bytes(first, want, 'resize, first of two')
    same_bytes(second, want, 'resize, cached tables')


def _holes(shape, seed, frac=0.25):
    rng = np.random.default_rng(seed)
    grid = rng.random(shape).astype(np.float32)
    mask = rng.random(shape) < frac
    grid[5, 6] = np.nan
    mask[5, 6] = False
    return grid, mask


def test_fills(ia):
    from imgprocessor_amd.interpolate.interpolate2dStructuredIDW import idw_weights
    from imgprocessor_amd.interpolate.interpolate2dStructuredFastIDW import growPositions
    ops, ctx = ia.ops, ia.default_context(0)
    grid, mask = _holes(DST, 11)
    m8 = mask.astype(np.uint8)
    pos, dist = growPositions(4)
    runs = {
        'idw_fill': lambda g, m: ops.idw_fill(g, m, 3, idw_weights(3, 2, 1, 1)),
        'fast_idw_fill': lambda g, m: ops.fast_idw_fill(g, m, pos, 1 / dist, 4),
        'circular_idw_fill': lambda g, m: ops.circular_idw_fill(g, m, 4, 2, 1, 0.3, 21, 30),
        'cross_avg_fill': lambda g, m: ops.cross_avg_fill(g, m, 3),
    }
    for name, run in runs.items():
        host = run(grid.copy(), m8.copy())
        same_bytes(host, run(ctx.to_device(grid), ctx.to_device(m8)), name)
    # point spread: the grid and the mask both come back
    hg, hm = grid.copy(), m8.copy()
    dg, dm = ctx.to_device(grid), ctx.to_device(m8)
    ops.point_spread_idw(hg, hm, 3)
    ops.point_spread_idw(dg, dm, 3)
    same_bytes(hg, dg, 'point_spread_idw grid')
    same_bytes(hm, dm, 'point_spread_idw mask')
    assert not np.array_equal(hm, m8)
    # unstructured: nothing is uploaded, every pixel written
    rng = np.random.default_rng(12)
    x, y, v = rng.random(9) * DST[0], rng.random(9) * DST[1], rng.standard_normal(9)
    host = ops.unstructured_idw(x, y, v, np.full(DST, 7, np.float32))
    same_bytes(host, ops.unstructured_idw(x, y, v, ctx.to_device(np.full(DST, 9, np.float32))), 'unstructured_idw')


# One sequence per family on a context of its own, whose workspace is empty at first: a 16 x 16 call reserves it
# (16 x 16 arrays + 25 % + 1 MiB), the large call does not fit and makes it grow, the third call reuses the grown one.
# Batches are 3 x 200 x 300 (2.2 MB of float32 source and result); the fills and resize take one 2-D array, and
# 200 x 300 of those would still fit the first reservation: 600 x 900 (2.1 MB of float32) there.
def _grow_sequence(ia, big, run):
    ctx = ia.Context(0)
    try:
        for shape in ((1, 16, 16), big, (1, 16, 16)):
            run(ctx, shape)
    finally:
        ctx.close()


def test_workspace_grows_and_is_reused_remap(ia):
    def run(ctx, shape):
        src = frames(*shape)
        mx, my = rot_maps(shape[1], shape[2], 3.0)
        same_bytes(ia.ops.remap(src, mx, my, ctx=ctx),
                   ia.ops.remap(ctx.to_device(src), ctx.to_device(mx), ctx.to_device(my)), 'remap %s' % (shape,))
    _grow_sequence(ia, (3, 200, 300), run)


def test_workspace_grows_and_is_reused_conv(ia):
    def run(ctx, shape):
        src = frames(*shape)
        mask = (np.random.default_rng(4).random(shape[1:]) < 0.1).astype(np.uint8)
        same_bytes(ia.ops.conv2d(src, kern(3), mask=mask, ctx=ctx),
                   ia.ops.conv2d(ctx.to_device(src), kern(3), mask=ctx.to_device(mask)), 'conv2d %s' % (shape,))
        g = ia.ops.gaussian_kernel1d(0.5)
        same_bytes(ia.ops.sepconv2d(src, g, g, ctx=ctx), ia.ops.sepconv2d(ctx.to_device(src), g, g),
                   'sepconv2d %s' % (shape,))
    _grow_sequence(ia, (3, 200, 300), run)


def test_workspace_grows_and_is_reused_fill(ia):
    from imgprocessor_amd.interpolate.interpolate2dStructuredIDW import idw_weights

    def run(ctx, shape):
        grid, mask = _holes(shape[1:], 13, 0.1)
        m8 = mask.astype(np.uint8)
        w = idw_weights(2, 2, 1, 1)
        same_bytes(ia.ops.idw_fill(grid.copy(), m8, 2, w, ctx=ctx),
                   ia.ops.idw_fill(ctx.to_device(grid), ctx.to_device(m8), 2, w), 'idw_fill %s' % (shape,))
    _grow_sequence(ia, (1, 600, 900), run)


def test_workspace_grows_and_is_reused_resize(ia):
    def run(ctx, shape):
        one = np.ascontiguousarray(frames(*shape)[0])
        dsize = (shape[1] * 3 // 4, shape[2] * 3 // 4 + 1)
        same_bytes(ia.ops.resize(one, dsize, 'linear', ctx=ctx), ia.ops.resize(ctx.to_device(one), dsize, 'linear'),
                   'resize %s' % (shape,))
    _grow_sequence(ia, (1, 600, 900), run)
