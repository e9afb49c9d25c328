"""PerspectiveCorrection.correctGrid restated for the tests, from its table of writes (nine groups
of cells, in paint order) with real numpy slices: `paint` records which write owns which pixel,
`compose` performs the writes with a per-cell warp function.  Independent of
PerspectiveCorrection._gridCells and of the library's ownership plan, which are checked against it."""
import numpy as np


def writes(n0, n1, snew, b):
    """-> list of (ix, iy, rows slice, cols slice, (offx, offy) of objP), sx, sy; the output has shape
    snew[::-1]: snew = (width, height), grid axis 0 runs along x"""
    W, H = snew
    sx, sy = (W - 2 * b) // n0, (H - 2 * b) // n1
    xr = (n0 - 1) * sx + b
    w = []
    for ix in range(1, n0 - 1):                                   # 1 inner
        for iy in range(1, n1 - 1):
            w.append((ix, iy, slice(iy * sy + b, (iy + 1) * sy + b),
                      slice(ix * sx + b, (ix + 1) * sx + b), (0, 0)))
    for ix in range(1, n0 - 1):                                   # 2 top
        w.append((ix, 0, slice(None, sy + b), slice(ix * sx + b, (ix + 1) * sx + b), (0, b)))
    for ix in range(1, n0 - 1):                                   # 3 bottom
        iy = n1 - 1
        w.append((ix, iy, slice(iy * sy + b, iy * sy + sy + 2 * b),
                  slice(ix * sx + b, ix * sx + b + sx), (0, 0)))
    for iy in range(1, n1 - 1):                                   # 4 left
        w.append((0, iy, slice(iy * sy + b, iy * sy + b + sy), slice(None, sx + b), (b, 0)))
    for iy in range(1, n1 - 1):                                   # 5 right
        w.append((n0 - 1, iy, slice(iy * sy + b, iy * sy + b + sy), slice(xr, xr + sx + b), (0, 0)))
    w.append((n0 - 1, n1 - 1, slice(-sy - b - 1, None), slice(xr, xr + sx + b), (0, 0)))   # 6
    w.append((0, 0, slice(0, sy + b), slice(0, sx + b), (b, b)))                           # 7
    w.append((n0 - 1, 0, slice(None, sy + b), slice(xr, xr + sx + b), (0, b)))             # 8
    w.append((0, n1 - 1, slice(-sy - b - 1, None), slice(None, sx + b), (b, 0)))           # 9
    return w, sx, sy


def paint(n0, n1, snew, b):
    """the ordinal of the write that owns each pixel, -1 where none does"""
    out = np.full(tuple(snew[::-1]), -1, dtype=np.int64)
    for k, (_, _, rows, cols, _) in enumerate(writes(n0, n1, snew, b)[0]):
        out[rows, cols] = k
    return out


def paint_rects(rects, shape):
    """the same map from a list of (x0, y0, w, h) painted in order"""
    out = np.full(tuple(shape), -1, dtype=np.int64)
    for k, (x0, y0, w, h) in enumerate(np.asarray(rects).reshape(-1, 4)):
        out[y0:y0 + h, x0:x0 + w] = k
    return out


def compose(warp_fn, img, grid, snew, b, transform_fn, hole, dtype=None):
    """the reference's sequence of writes: warp_fn(img, inv(hcell), (rows, cols)) into out[rows, cols],
    out pre-filled with `hole`; img (H, W) or (N, H, W); transform_fn = getPerspectiveTransform"""
    grid = np.asarray(grid)
    n0, n1 = grid.shape[0] - 1, grid.shape[1] - 1
    w, sx, sy = writes(n0, n1, snew, b)
    img = np.asarray(img)
    out = np.full(img.shape[:-2] + tuple(snew[::-1]), hole, dtype=dtype or img.dtype)
    objP0 = np.array([[0, 0], [sx, 0], [sx, sy], [0, sy]], dtype=np.float32)
    for ix, iy, rows, cols, off in w:
        view = out[..., rows, cols]
        quad = grid[ix:ix + 2, iy:iy + 2].reshape(4, 2)[np.array([0, 2, 3, 1])].astype(np.float32)
        hcell = transform_fn(quad, objP0 + np.float32(off))
        view[...] = warp_fn(img, np.linalg.inv(hcell), view.shape[-2:])
    return out


def lattice(n0, n1, src_shape, seed, jitter=3.0):
    """(n0 + 1, n1 + 1, 2) points (x, y): the regular lattice over the central 80 % of the source plus
    a seeded jitter of up to `jitter` px"""
    sh, sw = src_shape
    xs = np.linspace(0.1 * sw, 0.9 * sw, n0 + 1)
    ys = np.linspace(0.1 * sh, 0.9 * sh, n1 + 1)
    g = np.stack(np.meshgrid(xs, ys, indexing='ij'), axis=-1)
    return g + np.random.default_rng(seed).uniform(-jitter, jitter, g.shape)
