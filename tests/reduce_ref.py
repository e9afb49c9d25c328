"""numpy restatement of the ORDER in which the calibration units add a frame up (csrc/reduce.hpp and
the kernels of nlf.hip, spot.hip and poly.hip that use it).  Two stages:
  1  workgroup b of `grid` takes units b, b + grid, ...; lane t adds its sample of each unit, in
     that order, onto the identity 0.0; then the tree over the 256 lanes;
  2  one workgroup: lane t adds partials t, t + 256, ... onto 0.0; then the tree again.
The tree runs top down: in the step of width s = 128, 64, .., 1 lane t < s becomes
lane[t] + lane[t + s].  Those units are compiled without FP contraction, so float64 numpy
arithmetic in this order gives the device's bits.  numpy only."""
import numpy as np

LANES = 256


def tree(lanes):
    """the 256 lanes' values -> lane 0 after the tree"""
    a = np.array(lanes, dtype=np.float64)
    assert a.shape == (LANES,)
    s = LANES // 2
    while s:
        a[:s] = a[:s] + a[s:2 * s]
        s //= 2
    return a[0]


def fold_partials(parts):
    """stage 2: lane t takes parts[t], parts[t + 256], ... in that order, then the tree"""
    parts = np.asarray(parts, dtype=np.float64)
    acc = np.zeros(LANES)
    for p0 in range(0, len(parts), LANES):
        chunk = parts[p0:p0 + LANES]
        acc[:len(chunk)] = acc[:len(chunk)] + chunk
    return tree(acc)


def row_unit_partials(values, live, grid):
    """stage 1 of the kernels whose unit is 256 consecutive pixels of one row: `values` (rows, w)
    float64, `live` (rows, w) bool - the lanes whose sample is added; the others, and the lanes
    beyond the row's end, keep what they have -> the `grid` partial sums"""
    values = np.asarray(values, dtype=np.float64)
    live = np.asarray(live, dtype=bool)
    rows, w = values.shape
    upr = (w + LANES - 1) // LANES
    parts = np.empty(grid)
    for b in range(grid):
        acc = np.zeros(LANES)
        for u in range(b, rows * upr, grid):
            y, x0 = u // upr, (u % upr) * LANES
            v, on = values[y, x0:x0 + LANES], live[y, x0:x0 + LANES]
            acc[:len(v)] = np.where(on, acc[:len(v)] + v, acc[:len(v)])
        parts[b] = tree(acc)
    return parts


def row_unit_sum(values, live, grid):
    return fold_partials(row_unit_partials(values, live, grid))


def capped_grid(units, cap):
    """min(units, cap), at least 1: the arithmetic every unit shares; the cap is the unit's own"""
    return max(1, min(units, cap))


def row_units(rows, w):
    return rows * ((w + LANES - 1) // LANES)


def tile_partials(values, grid=None):
    """stage 1 of poly_eval_kernel: lane t of a 64 x 4 tile is its pixel (t & 63, t >> 6), a lane
    outside the frame holds 0.0; tiles in row-major order.  The kernel runs one workgroup per tile
    (grid None); with fewer, workgroup b would take tiles b, b + grid, ... as the row units are taken"""
    values = np.asarray(values, dtype=np.float64)
    h, w = values.shape
    ty, tx = (h + 3) // 4, (w + 63) // 64
    pad = np.zeros((ty * 4, tx * 64))
    pad[:h, :w] = values
    tiles = [pad[4 * j:4 * j + 4, 64 * i:64 * i + 64].ravel() for j in range(ty) for i in range(tx)]
    grid = len(tiles) if grid is None else grid
    parts = np.empty(grid)
    for b in range(grid):
        acc = np.zeros(LANES)
        for t in tiles[b::grid]:
            acc = acc + t
        parts[b] = tree(acc)
    return parts


def tile_sum(values, grid=None):
    return fold_partials(tile_partials(values, grid))


def bits(x):
    return np.float64(x).tobytes()
