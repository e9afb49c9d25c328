"""ops.warp_grid / PerspectiveCorrection.correctGrid on the device: one launch must give bit for bit
what the reference's sequence of per-cell warps gives (tests/grid_ref.py::compose around the
existing ops.warp_perspective), holes the defined hole value, and correctGrid the oracle's result
within the tolerances tests/test_gpu_parity.py applies to warp_perspective in the same mode."""
import numpy as np
import pytest

from . import grid_ref
from .conftest import synth, assert_close

pytestmark = pytest.mark.gpu

SRC = (96, 128)
# (n0, n1, snew, b).  Main: sx = 73 - no multiple of the kernel's 4-px groups, so groups straddle cells -,
# 300 px cross the 256-px tile boundary, 2 hole columns, the bottom corners overlap the bottom cells
MAIN = (4, 3, (300, 45), 3)
SMALL = [(2, 2, (20, 20), 0), (1, 1, (9, 7), 0)]
FAR = np.array([[1.0, 0, 1e5], [0, 1.0, 1e5], [0, 0, 1.0]])   # every sample wholly outside the source


@pytest.fixture(scope='module')
def ia():
    import imgprocessor_amd
    imgprocessor_amd.default_context(0)  # raises without a gfx950 device: no fallback
    return imgprocessor_amd


@pytest.fixture(scope='module')
def src():
    img = synth(SRC, 7)
    img.setflags(write=False)
    return img


def _case(case, seed=3):
    from imgprocessor_amd.camera.PerspectiveCorrection import PerspectiveCorrection
    n0, n1, snew, b = case
    grid = grid_ref.lattice(n0, n1, SRC, seed)
    rects, M = PerspectiveCorrection(SRC, new_size=snew, border=b)._gridCells(grid)
    return grid, rects, M


def _as(img, dtype):
    """the float32 test image in another element type, over that type's range"""
    if dtype == np.uint8:
        return np.round(img * 255).astype(np.uint8)
    if dtype == np.uint16:
        return np.round(img * 65535).astype(np.uint16)
    return img.astype(dtype)


def _same(got, want, what):
    assert got.shape == want.shape and got.dtype == want.dtype, (what, got.shape, want.shape, got.dtype)
    if got.dtype.kind == 'f':
        u = np.uint32 if got.dtype.itemsize == 4 else np.uint64
        bad = (got.view(u) != want.view(u)) & ~(np.isnan(got) & np.isnan(want))
    else:
        bad = got != want
    assert not bad.any(), '%s: %d of %d values differ, first at %s (%r vs %r)' % (
        what, bad.sum(), got.size, np.argwhere(bad)[0], got[bad][0], want[bad][0])


def _check(ia, img, case, interp, border='constant', cval=0.0, out_dtype=None):
    """ops.warp_grid against the per-cell ops.warp_perspective calls pasted in the reference's order;
    the hole value: what ops.warp_perspective stores wholly outside the source under 'constant'"""
    from imgprocessor_amd.utils.geometry import getPerspectiveTransform
    n0, n1, snew, b = case
    grid, rects, M = _case(case)
    odt = np.dtype(out_dtype or img.dtype)
    hole = ia.ops.warp_perspective(img, FAR, (1, 1), interp, 'constant', cval, out_dtype=odt)[0, 0]

    def warp(im, Minv, shape):
        return ia.ops.warp_perspective(im, Minv, shape, interp, border, cval, out_dtype=odt)
    want = grid_ref.compose(warp, img, grid, snew, b, getPerspectiveTransform, hole, dtype=odt)
    got = ia.ops.warp_grid(img, rects, M, snew[::-1], interp, border, cval, out_dtype=odt)
    what = '%s %s %s->%s %s %r' % (case, interp, img.dtype, odt, border, cval)
    _same(got, want, what)
    holes = grid_ref.paint(n0, n1, snew, b) == -1
    if holes.any():
        _same(got[holes], np.full(int(holes.sum()), hole, odt), what + ' holes')
    return got, holes


def test_every_interpolation_float32(ia, src):
    for interp in sorted(ia.ops.INTERPOLATIONS):
        _, holes = _check(ia, src, MAIN, interp)
        assert holes[:, 298:].all() and holes.sum() >= 2 * 45
    for case in SMALL:
        for interp in ('lanczos4', 'linear', 'cubic'):
            _check(ia, src, case, interp)


@pytest.mark.parametrize('sdt,ddt', [(np.float32, np.float32), (np.float64, np.float64),
                                     (np.uint16, np.uint16), (np.uint16, np.float32),
                                     (np.uint8, np.uint8), (np.uint8, np.float32),
                                     (np.float32, np.uint8), (np.float32, np.uint16)])
def test_every_dtype_pair_lanczos4(ia, src, sdt, ddt):
    img = _as(src, sdt)
    if sdt == np.float32 and ddt != np.float32:
        img = src * np.float32(255 if ddt == np.uint8 else 65535)   # values over the destination's range
    _check(ia, img, MAIN, 'lanczos4', cval=17.0, out_dtype=ddt)
    _check(ia, img, SMALL[1], 'lanczos4', cval=0.0, out_dtype=ddt)


@pytest.mark.parametrize('border,cval', [('constant', 0.0), ('constant', float('nan')),
                                         ('replicate', 7.5), ('reflect101', 7.5), ('wrap', 7.5)])
def test_borders_and_holes_float32_bilinear(ia, src, border, cval):
    got, holes = _check(ia, src, MAIN, 'linear', border, cval)
    # the hole value is the border value under every border mode
    hv = got[holes]
    assert np.isnan(hv).all() if cval != cval else (hv == np.float32(cval)).all()
    if cval == cval:   # integer frames in cv2's own arithmetic: the border value as that branch rounds it
        got8, holes = _check(ia, _as(src, np.uint8), MAIN, 'linear_cv_q5', border, cval)
        assert (got8[holes] == int(np.rint(cval))).all()


def test_correct_grid_against_the_oracle(ia, src, oracle):
    from imgprocessor_amd.camera.PerspectiveCorrection import PerspectiveCorrection
    n0, n1, snew, b = MAIN
    grid = grid_ref.lattice(n0, n1, SRC, 3)
    for dtype, interp, iid in ((np.float32, None, oracle.LANCZOS4), (np.uint16, None, oracle.LANCZOS4),
                               (np.uint8, None, oracle.LANCZOS4), (np.float32, 'linear', oracle.LINEAR)):
        img = _as(src, dtype)
        pc = PerspectiveCorrection(SRC, new_size=snew, border=b, interpolation=interp)
        got = pc.correctGrid(img, grid)
        assert got.shape == (45, 300) and got.dtype == img.dtype

        def warp(im, Minv, shape):
            return oracle.warp_perspective(im, Minv, shape, iid, oracle.CONSTANT, 0.0)
        want = grid_ref.compose(warp, img, grid, snew, b, oracle.get_perspective_transform, 0)
        if dtype == np.float32:   # test_gpu_parity.close32 with scale = 1: 1e-5 of the data range
            assert_close(got, want, 1e-5, 1e-5, 'correctGrid %s' % (interp or 'lanczos4'))
        else:
            assert np.array_equal(got, want), (dtype, np.abs(got.astype(int) - want.astype(int)).max())


def test_batches_equal_single_frames(ia, src):
    _, rects, M = _case(MAIN)
    shape = MAIN[2][::-1]
    f32 = np.stack([np.roll(src, 11 * i, axis=1) for i in range(4)])
    for frames, interp in ((f32, 'lanczos4'), (f32, 'cubic'), (_as(f32, np.uint16), 'lanczos4')):
        got = ia.ops.warp_grid(frames, rects, M, shape, interp, 'constant', 3.0)
        assert got.shape == (4,) + shape
        for i in range(4):
            _same(got[i], ia.ops.warp_grid(frames[i], rects, M, shape, interp, 'constant', 3.0),
                  '%s %s frame %d' % (frames.dtype, interp, i))


def test_known_answer_pins_the_bottom_corner_offset(ia):
    """the exact lattice: every cell is the identity, so the output is the source - except that the
    reference starts its two bottom corner cells one row early (out[-sy - b - 1:]): they hold the
    source one row further down, their last row reads row 40 of a 40-row source = the border value.
    The right one loses its first row to the top right cell, painted after it; the left one is
    painted last."""
    from imgprocessor_amd.camera.PerspectiveCorrection import PerspectiveCorrection
    img = np.random.default_rng(4).random((40, 60)).astype(np.float32)
    grid = np.stack(np.meshgrid(np.arange(4) * 20.0, np.arange(3) * 20.0, indexing='ij'), axis=-1)
    got = PerspectiveCorrection(img.shape, new_size=(60, 40), border=0).correctGrid(img, grid)
    want = img.copy()
    want[19:39, 0:20] = img[20:40, 0:20]
    want[20:39, 40:60] = img[21:40, 40:60]
    want[39, 0:20] = 0
    want[39, 40:60] = 0
    assert np.array_equal(got, want), np.argwhere(got != want)[:5]


def test_colour_and_device_arrays(ia, src):
    from imgprocessor_amd.camera.PerspectiveCorrection import PerspectiveCorrection
    n0, n1, snew, b = MAIN
    grid = grid_ref.lattice(n0, n1, SRC, 3)
    pc = PerspectiveCorrection(SRC, new_size=snew, border=b)
    rgb = np.stack([src, src[::-1], src[:, ::-1]], axis=-1)
    got = pc.correctGrid(rgb, grid)
    assert got.shape == (45, 300, 3)
    planes = [pc.correctGrid(np.ascontiguousarray(rgb[..., c]), grid) for c in range(3)]
    for c in range(3):
        _same(np.ascontiguousarray(got[..., c]), planes[c], 'plane %d' % c)
    d = pc.correctGrid(pc.ctx.to_device(np.ascontiguousarray(rgb[..., 1])), grid)
    assert isinstance(d, ia.DeviceArray) and d.shape == (45, 300)
    _same(d.get(), planes[1], 'DeviceArray')


def test_plan_cache_alternating_and_evicting(ia, src):
    """two grids alternated on one context (both plans stay cached), then more grids than the cache
    holds, twice round (every plan is evicted and made again): always the first result"""
    ctx = ia.default_context(0)
    d = ctx.to_device(src)
    shape = MAIN[2][::-1]
    cells = [_case(MAIN, seed)[1:] for seed in range(20, 26)]
    first = [ia.ops.warp_grid(d, r, M, shape, 'lanczos4').get() for r, M in cells]
    assert not np.array_equal(first[0], first[1])
    for _ in range(3):
        for k in (0, 1):
            _same(ia.ops.warp_grid(d, cells[k][0], cells[k][1], shape, 'lanczos4').get(), first[k], 'grid %d' % k)
    for _ in range(2):
        for k, (r, M) in enumerate(cells):
            _same(ia.ops.warp_grid(d, r, M, shape, 'lanczos4').get(), first[k], 'grid %d' % k)


def test_bad_arguments(ia, src):
    _, rects, M = _case(MAIN)
    shape = MAIN[2][::-1]
    with pytest.raises(ValueError, match='not inside'):
        ia.ops.warp_grid(src, rects, M, (shape[0], shape[1] - 10))
    bad = rects.copy()
    bad[3, 2] = 0
    with pytest.raises(ValueError, match='empty rectangle'):
        ia.ops.warp_grid(src, bad, M, shape)
    with pytest.raises(ValueError, match='n_cells'):
        ia.ops.warp_grid(src, rects[:0], M[:0], shape)
    with pytest.raises(ValueError):
        ia.ops.warp_grid(src, rects, M[:-1], shape)
    with pytest.raises(ValueError):
        ia.ops.warp_grid(src, rects, M, shape, 'bogus')
