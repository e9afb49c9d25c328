"""PerspectiveCorrection.correctGrid, the parts that need no device: the cell list of
_gridCells against the reference's table of writes (tests/grid_ref.py) and the ownership plan of
ipa_warp_grid_plan against a per-pixel paint."""
import ctypes as C

import numpy as np
import pytest

from . import grid_ref

CASES = [(4, 3, (300, 45), 3), (3, 3, (32, 26), 2), (2, 2, (20, 20), 0), (1, 1, (9, 7), 0),
         (1, 4, (16, 40), 1)]


def _pc(snew, b):
    from imgprocessor_amd.camera.PerspectiveCorrection import PerspectiveCorrection
    return PerspectiveCorrection((96, 128), new_size=snew, border=b)


def _cells(n0, n1, snew, b, seed=3):
    grid = grid_ref.lattice(n0, n1, (96, 128), seed)
    rects, M = _pc(snew, b)._gridCells(grid)
    assert rects.dtype == np.int32 and rects.shape[1] == 4
    assert M.dtype == np.float64 and M.shape == (len(rects), 9)
    return grid, rects, M


@pytest.mark.parametrize('n0,n1,snew,b', CASES)
def test_grid_cells_paint_like_the_reference(n0, n1, snew, b):
    _, rects, _ = _cells(n0, n1, snew, b)
    want = grid_ref.paint(n0, n1, snew, b)
    assert want.shape == snew[::-1]
    assert np.array_equal(grid_ref.paint_rects(rects, snew[::-1]), want)


def test_grid_cells_by_hand():
    """(3, 3, (32, 26), 2): sx = 9, sy = 7, x_r = 20; the nine groups written out"""
    grid, rects, M = _cells(3, 3, (32, 26), 2)
    #        x0  y0   w   h    objP offset   cell
    want = [(11,  9,  9,  7), (11,  0,  9,  9), (11, 16,  9,  9), ( 0,  9, 11,  7), (20,  9, 11,  7),
            (20, 16, 11, 10), ( 0,  0, 11,  9), (20,  0, 11,  9), ( 0, 16, 11, 10)]
    offs = [(0, 0), (0, 2), (0, 0), (2, 0), (0, 0), (0, 0), (2, 2), (0, 2), (2, 0)]
    cell = [(1, 1), (1, 0), (1, 2), (0, 1), (2, 1), (2, 2), (0, 0), (2, 0), (0, 2)]
    assert rects.tolist() == [list(r) for r in want]
    for i in range(9):
        # hcell = inv(M) takes the cell's first lattice point to objP[0] = the offset, the
        # opposite one to offset + (sx, sy)
        h = np.linalg.inv(M[i].reshape(3, 3))
        ix, iy = cell[i]
        for p, q in ((grid[ix, iy], offs[i]), (grid[ix + 1, iy + 1], (offs[i][0] + 9, offs[i][1] + 7))):
            v = h @ np.array([np.float32(p[0]), np.float32(p[1]), 1.0])
            assert np.allclose(v[:2] / v[2], q, atol=1e-6), (i, v, q)
    own = grid_ref.paint_rects(rects, (26, 32))
    assert (own[:, 31] == -1).all()
    assert (own[25, 11:20] == -1).all() and (own[:25, :31] >= 0).all()
    assert (own[16:26, :11] == 8).all() and (own[16:26, 20:31] == 5).all()   # the bottom corners, 10 rows
    assert (own[16:25, 11:20] == 2).all()


def test_grid_cells_errors():
    with pytest.raises(ValueError):
        _pc((5, 40), 0)._gridCells(np.zeros((7, 3, 2)))     # sx = 5 // 6 = 0
    with pytest.raises(ValueError):
        _pc((40, 9), 4)._gridCells(np.zeros((3, 3, 2)))     # sy = (9 - 8) // 2 = 0
    with pytest.raises(ValueError):
        _pc((40, 40), 0)._gridCells(np.zeros((3, 3)))


def _check_plan(rects, shape):
    from imgprocessor_amd import ops
    col, row, owner = ops.warp_grid_plan(rects, shape)
    assert col.shape == (shape[1],) and row.shape == (shape[0],)
    assert col[0] == 0 and row[0] == 0 and col[-1] == owner.shape[1] - 1 and row[-1] == owner.shape[0] - 1
    got = owner[row.astype(np.intp)[:, None], col.astype(np.intp)[None, :]]
    assert np.array_equal(got, grid_ref.paint_rects(rects, shape))
    return owner


@pytest.mark.parametrize('n0,n1,snew,b', CASES)
def test_plan_owner_matches_paint(n0, n1, snew, b):
    _, rects, _ = _cells(n0, n1, snew, b)
    _check_plan(rects, snew[::-1])
    assert np.array_equal(grid_ref.paint_rects(rects, snew[::-1]), grid_ref.paint(n0, n1, snew, b))


def test_plan_random_overlapping_rectangles():
    rng = np.random.default_rng(11)
    for it in range(50):
        dh, dw = int(rng.integers(1, 48)), int(rng.integers(1, 48))
        rects = []
        for _ in range(int(rng.integers(1, 14))):
            kind = rng.integers(0, 3)
            if kind == 0:     # 1-px rectangle
                x0, y0, w, h = int(rng.integers(0, dw)), int(rng.integers(0, dh)), 1, 1
            elif kind == 1:   # corners on a coarse lattice: rectangles that share edges
                xs = np.unique(np.minimum(rng.integers(0, 6, 2) * 8, dw))
                ys = np.unique(np.minimum(rng.integers(0, 6, 2) * 8, dh))
                if len(xs) < 2 or len(ys) < 2:
                    continue
                x0, y0, w, h = int(xs[0]), int(ys[0]), int(xs[1] - xs[0]), int(ys[1] - ys[0])
            else:
                x0, y0 = int(rng.integers(0, dw)), int(rng.integers(0, dh))
                w, h = int(rng.integers(1, dw - x0 + 1)), int(rng.integers(1, dh - y0 + 1))
            rects.append((x0, y0, w, h))
        if not rects:
            rects.append((0, 0, dw, dh))
        _check_plan(np.array(rects, np.int32), (dh, dw))


def test_plan_bad_arguments():
    """n_cells outside [1, 32767], empty rectangles, rectangles not inside the destination.  (More than
    65535 bands on an axis needs more than 32767 cells: that refusal cannot be reached on its own.)"""
    from imgprocessor_amd import _lib
    lib = _lib.lib()
    nr, nc = C.c_int(0), C.c_int(0)

    def plan(rects, dh, dw, n=None):
        r = np.ascontiguousarray(rects, np.int32).reshape(-1, 4)
        return lib.ipa_warp_grid_plan(r.ctypes.data_as(_lib._ip), len(r) if n is None else n, dh, dw,
                                      None, None, None, C.byref(nr), C.byref(nc))
    ok = [(0, 0, 4, 4)]
    assert plan(ok, 8, 8) == _lib.OK and (nr.value, nc.value) == (2, 2)
    for bad in ([(0, 0, 0, 4)], [(0, 0, 4, 0)], [(0, 0, 4, -1)], [(-1, 0, 4, 4)], [(0, -1, 4, 4)],
                [(5, 0, 4, 4)], [(0, 5, 4, 4)], ok + [(0, 0, 9, 1)], [(2 ** 31 - 1, 0, 2, 2)]):
        assert plan(bad, 8, 8) == _lib.ERR_BAD_ARG, bad
        assert lib.ipa_last_error(None), bad
    assert plan(ok, 8, 8, n=0) == _lib.ERR_BAD_ARG
    assert plan(ok, 0, 8) == _lib.ERR_BAD_ARG and plan(ok, 8, 0) == _lib.ERR_BAD_ARG
    many = np.tile(np.array([0, 0, 1, 1], np.int32), (32768, 1))
    assert plan(many, 8, 8) == _lib.ERR_BAD_ARG
    assert plan(many[:32767], 8, 8) == _lib.OK
    assert lib.ipa_warp_grid_plan(None, 1, 8, 8, None, None, None, C.byref(nr), C.byref(nc)) == _lib.ERR_BAD_ARG
