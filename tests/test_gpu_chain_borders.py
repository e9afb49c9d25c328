"""GPU: the remap -> filter chains with a DIFFERENT filter border mode per axis.

The six chain exports take the filter's two border modes in two orders - the dense ones as
(conv_border_x, conv_border_y), the separable ones as (conv_border_y, conv_border_x) - and ops.py passes
the same mode for both, so an x / y swap anywhere between an export and its kernel is invisible to the rest
of the suite.  Here the exports are called directly (ctx._lib) with wrap along one axis and constant along
the other, both ways round, on every route a chain can take: the resident strip kernel (dense 3 x 3), the
rank-1 route (outer(g5, g5) -> the separable loop), the separable loop (7 + 7), the streamed kernel (dense
9 x 9; with maps - the other coordinate sources run it as two launches) and the two launches (bicubic +
separable 5 + 5).  n = 1 is the per-frame loop, n = 4 the shared-record loop.  Every call's launch record
(ctx.get_tuning('chain_path')) is held against route() below, which states all of this case by case.

Expected: the oracle's remap of each frame (float32), then tests/conv_ref.py's ref_conv2d / ref_sepconv2d
with mode (columns) and mode_y (rows) set per axis, within that file's bound().  Every case first shows, on
the CPU, that the reference with the two modes swapped is at least 100 bounds away somewhere in the frame:
a swap cannot pass.
"""
import ctypes as C

import numpy as np
import pytest

from .conv_ref import bound, ref_conv2d, ref_sepconv2d

pytestmark = pytest.mark.gpu

H, W = 24, 260       # two strips per row at the 240- and the 248-px steps; W a multiple of 4
SH, SW = 36, 272     # the source: every tap of the mild coordinates below stays inside it
NMAX = 4


@pytest.fixture(scope='module')
def ia():
    import imgprocessor_amd
    imgprocessor_amd.default_context(0)
    return imgprocessor_amd


def gauss(k, sigma=1.0):
    g = np.exp(-0.5 * ((np.arange(k) - k // 2) / sigma) ** 2)
    return g / g.sum()


def dense(K, seed):
    k = np.random.default_rng(seed).random((K, K)) + 0.1   # (full rank: not an outer product)
    return k / k.sum()


# name -> (dense kernel or (ky, kx), interpolation of the remap)
FILTERS = {
    'dense3': (dense(3, 3), 'linear'),
    'rank1_5': (np.outer(gauss(5), gauss(5)), 'linear'),
    'sep7': ((gauss(7, 1.4), gauss(7, 1.1)), 'linear'),
    'dense9': (dense(9, 9), 'linear'),
    'cubic_sep5': ((gauss(5), gauss(5, 0.8)), 'cubic'),
}
COORDS = ('maps', 'lens', 'lens_nocache', 'homography')
K_LENS = np.array([[300.0, 0, 135.5], [0, 300.0, 17.5], [0, 0, 1.0]])
NEWK_LENS = np.array([[300.0, 0, 129.5], [0, 300.0, 11.5], [0, 0, 1.0]])
DIST = np.array([-0.02, 0.004, 1e-4, -1e-4, 0.0])
M_HOM = np.array([[1.002, 0.01, 5.3], [0.004, 0.998, 3.6], [1e-6, -2e-6, 1.0]])


@pytest.fixture(scope='module')
def scene(ia, oracle):
    """frames in [1, 2), their device copy, the coordinate sources and - computed once, left unchanged - the
    oracle's remap of every frame for (coordinate source, interpolation)"""
    from imgprocessor_amd import ops
    ctx = ia.default_context(0)
    src = (1.0 + np.random.default_rng(11).random((NMAX, SH, SW))).astype(np.float32)
    y, x = np.mgrid[0:H, 0:W].astype(np.float64)
    mx = (x + 5.3 + 0.01 * y).astype(np.float32)
    my = (y + 3.6 + 0.005 * x).astype(np.float32)
    # the lens model's float32 coordinates as the library evaluates them (cached map and per-pixel form: same bits)
    lx, ly = ops.build_undistort_map(K_LENS, DIST, NEWK_LENS, H, W)
    mid = {}
    for interp, oi in (('linear', oracle.LINEAR), ('cubic', oracle.CUBIC_KEYS)):   # (ops.py's names)
        mid['maps', interp] = [oracle.remap(f, mx, my, oi) for f in src]
        mid['lens', interp] = [oracle.remap(f, lx, ly, oi) for f in src]
        mid['homography', interp] = [oracle.warp_perspective(f, M_HOM, (H, W), oi) for f in src]
    for v in mid.values():
        for m in v:
            # (bicubic taps undershoot 1 by up to 0.16 on this noise)
            assert m.dtype == np.float32 and m.min() > 0.5, 'the remapped rim must be non-zero'
            m.setflags(write=False)
    return {'ctx': ctx, 'src': src, 'd_src': ctx.to_device(src), 'mx': ctx.to_device(mx), 'my': ctx.to_device(my),
            'mid': mid}


def route(coords, fname, n):
    """the launch record of a case, from fused.hip's rules: the kernel by filter and coordinate source; LENS_MAP
    where the lens model goes through its cached map; FRAMES_WG for the four frames of a one-kernel chain,
    PER_FRAME for one; STORED for four frames under a homography on the shared-record loop"""
    from imgprocessor_amd import _lib as L
    kernel = {'dense3': L.CHAIN_PATH_RESIDENT, 'rank1_5': L.CHAIN_PATH_RANK1 | L.CHAIN_PATH_SEP,
              'sep7': L.CHAIN_PATH_SEP, 'cubic_sep5': L.CHAIN_PATH_TWO_LAUNCHES,
              'dense9': L.CHAIN_PATH_STREAMED if coords in ('maps', 'lens') else L.CHAIN_PATH_TWO_LAUNCHES}[fname]
    path = kernel | (L.CHAIN_PATH_LENS_MAP if coords == 'lens' else 0)
    if kernel & L.CHAIN_PATH_TWO_LAUNCHES:
        return path
    if coords == 'homography' and n == 4:
        path |= L.CHAIN_PATH_STORED
    return path | (L.CHAIN_PATH_FRAMES_WG if n == 4 else L.CHAIN_PATH_PER_FRAME)


def expected(mids, filt, bx, by, n):
    """the reference and its bound for the first n frames; asserts that swapped modes could not pass"""
    ref = ref_sepconv2d if isinstance(filt, tuple) else ref_conv2d
    args = filt if isinstance(filt, tuple) else (filt,)
    want, tol = [], []
    for f in range(n):
        w = ref(mids[f], *args, mode=bx, mode_y=by)
        t = bound(mids[f], filt, mode=bx, mode_y=by)
        swapped = ref(mids[f], *args, mode=by, mode_y=bx)
        assert (np.abs(swapped - w) >= 100 * t).any(), 'the swapped modes must be told apart by the reference alone'
        want.append(w)
        tol.append(t)
    return want, tol


def call_chain(ia, s, coords, filt, interp, n, bx, by):
    """one of the six exports, straight through ctypes; -> (n, H, W) float32"""
    from imgprocessor_amd import _lib as L
    from imgprocessor_amd.device import dtype_id
    from imgprocessor_amd.ops import border_id, interp_id
    ctx = s['ctx']
    lib = ctx._lib
    dst = ia.DeviceArray(ctx, (n, H, W), np.float32)
    dp = C.POINTER(C.c_double)
    f32 = dtype_id(np.float32)
    head = (ctx.handle, s['d_src'].ptr, f32, SH, SW, SW)
    if coords == 'maps':
        kind, where = 'remap', (s['mx'].ptr, s['my'].ptr, W)
    elif coords == 'homography':
        kind, where = 'warp_perspective', (L.dbl(np.ravel(M_HOM), 9),)
    else:
        kind, where = 'undistort', (L.dbl(np.ravel(K_LENS), 9), L.dbl(DIST, 5), L.dbl(np.ravel(NEWK_LENS), 9))
    tail = (dst.ptr, f32, H, W, W, n, SH * SW, H * W, interp_id(interp), border_id('constant'), 0.0)
    bx, by = border_id(bx), border_id(by)
    if isinstance(filt, tuple):
        ky = np.ascontiguousarray(filt[0], dtype=np.float64)
        kx = np.ascontiguousarray(filt[1], dtype=np.float64)
        fn = getattr(lib, 'ipa_%s_sepconv2d_dev' % kind)
        args = head + where + (ky.ctypes.data_as(dp), ky.size, kx.ctypes.data_as(dp), kx.size) + tail + (by, bx)
    else:
        k = np.ascontiguousarray(filt, dtype=np.float64)
        fn = getattr(lib, 'ipa_%s_conv2d_dev' % kind)
        args = head + where + (k.ctypes.data_as(dp), k.shape[0], k.shape[1]) + tail + (bx, by)
    ctx._check(fn(*args), '%s + %s' % (kind, 'separable' if isinstance(filt, tuple) else 'dense'))
    return dst.get()


@pytest.mark.parametrize('n', [1, 4])
@pytest.mark.parametrize('bx,by', [('wrap', 'constant'), ('constant', 'wrap')])
@pytest.mark.parametrize('fname', sorted(FILTERS))
@pytest.mark.parametrize('coords', COORDS)
def test_filter_border_per_axis(ia, scene, coords, fname, bx, by, n):
    filt, interp = FILTERS[fname]
    ctx = scene['ctx']
    mids = scene['mid']['lens' if coords == 'lens_nocache' else coords, interp]
    want, tol = expected(mids, filt, bx, by, n)
    old = ctx.set_tuning(lens_cache=0) if coords == 'lens_nocache' else {}
    try:
        before = ctx.get_tuning('rank1_routed')
        got = call_chain(ia, scene, coords, filt, interp, n, bx, by)
        routed = ctx.get_tuning('rank1_routed') - before
        path = ctx.get_tuning('chain_path')
    finally:
        if old:
            ctx.set_tuning(**old)
    assert routed == (1 if fname == 'rank1_5' else 0), 'rank-1 route'
    assert path == route(coords, fname, n), 'chain_path %#x, expected %#x' % (path, route(coords, fname, n))
    for f in range(n):
        err = np.abs(got[f].astype(np.float64) - want[f])
        worst = np.unravel_index(np.argmax(err - tol[f]), err.shape)
        print('%s %s x=%s y=%s n=%d frame %d: max err %.3g, bound there %.3g, worst err/bound %.3g'
              % (coords, fname, bx, by, n, f, err.max(), tol[f][worst], (err / tol[f]).max()))
        assert (err <= tol[f]).all(), ('%s, %s, x %s / y %s, frame %d of %d: worst at %s, got %r want %r bound %g'
                                      % (coords, fname, bx, by, f, n, worst, got[f][worst], want[f][worst],
                                         tol[f][worst]))
