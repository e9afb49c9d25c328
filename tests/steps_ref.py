"""numpy restatement of camera/flatField/vignettingFromDiscreteSteps.py up to its post-processing, the
yardstick of tests/test_cpu_steps.py and tests/test_gpu_steps.py.  It imports nothing of the package.

  cell_edges / cell_means   array/subCell2D.py:51-71 with the cell function of :228-234; the cell sums
                            through math.fsum (exactly rounded), where the reference has numpy's pairwise sum
  slices                    :26-60, _DeviceAndGridSlice.iter() as it is written
  separate                  :257-281, :316 with every np.nanmean(axis=0) spelt out as numpy computes it
                            (NaN -> 0, a sequential sum in frame order, divided by the count of non-NaN) and
                            the iteration cap of csrc/steps.hip: iteration k = 1, 2, ... is the last when
                            dev < max_dev or k > max_iter + 1
  offset_meshgrid           interpolate/offsetMeshgrid.py:18-27
"""
import math

import numpy as np


def cell_edges(size, g, d, p):
    acc, out = p, []
    for _ in range(g + 1):
        out.append(min(size, max(0, int(round(acc)))))
        acc = acc + d
    return np.array(out, dtype=np.int32)


def _cells(frames, row_edges, col_edges, thresh, bg, value):
    frames = np.asarray(frames)
    g0, g1 = len(row_edges) - 1, len(col_edges) - 1
    out = np.full((len(frames), g0, g1), np.nan)
    for n, f in enumerate(frames):
        x = f.astype(np.float64)
        if bg is not None:
            x = x - np.asarray(bg).astype(np.float64)
        for i in range(g0):
            for j in range(g1):
                c = x[row_edges[i]:row_edges[i + 1], col_edges[j]:col_edges[j + 1]]
                ind = c > thresh
                count = int(ind.sum())
                if c.size == 0 or 2 * count < c.size:
                    continue
                out[n, i, j] = math.fsum(value(c[ind]).tolist()) / count
    return out


def cell_means(frames, row_edges, col_edges, thresh, bg=None):
    return _cells(frames, row_edges, col_edges, thresh, bg, lambda v: v)


def cell_scale(frames, row_edges, col_edges, thresh, bg=None):
    """mean |x| over the samples of every cell: what the tolerance of a cell's mean is relative to"""
    return _cells(frames, row_edges, col_edges, thresh, bg, np.abs)


def slices(n0, n1, g0, g1, cell_positions):
    for i, (p0, p1) in enumerate(cell_positions):
        bottom = -1 < p0
        top = p0 + n0 <= g0
        left = -1 < p1
        right = p1 + n1 <= g1
        if left and right:
            q1, qq1 = slice(None, n1), slice(p1, p1 + n1)
        elif not left and right:
            q1, qq1 = slice(-p1, n1), slice(None, p1 + n1)
        elif not right and left:
            q1, qq1 = slice(None, -(p1 + n1 - g1)), slice(p1, None)
        else:
            q1, qq1 = slice(-p1, -(p1 + n1 - g1)), slice(p1, p1 + n1)
        if bottom and top:
            q0, qq0 = slice(None, n0), slice(p0, p0 + n0)
        elif not bottom and top:
            q0, qq0 = slice(-p0, n0), slice(None, p0 + n0)
        elif not top and bottom:
            q0, qq0 = slice(None, -(p0 + n0 - g0)), slice(p0, None)
        else:
            q0, qq0 = slice(-p0, -(p0 + n0 - g0)), slice(None, p0 + n0)
        yield i, q0, q1, qq0, qq1


def nanmean0(a):
    """np.nanmean(a, axis=0) as numpy computes it: bit for bit for 1 ... 64 frames (asserted by
    tests/test_cpu_steps.py against numpy itself)"""
    nan = np.isnan(a)
    z = np.where(nan, 0.0, a)
    acc = z[0].copy()
    for k in range(1, len(z)):
        acc = acc + z[k]
    with np.errstate(all='ignore'):
        return acc / (len(a) - nan.sum(axis=0))


def separate(grid, n_cells, cell_positions, bg_value=None, max_iter=100, max_dev=1e-6):
    """-> ff, avgobj, pointdensity, iterations, the deviations of all iterations"""
    grid = np.asarray(grid, dtype=np.float64)
    N, g0, g1 = grid.shape
    n0, n1 = n_cells
    sl = list(slices(n0, n1, g0, g1, cell_positions))
    devices = np.full((N, n0, n1), np.nan)
    for n, q0, q1, qq0, qq1 in sl:
        devices[n, q0, q1] = grid[n][qq0, qq1]
    with np.errstate(all='ignore'):
        ff = nanmean0(grid)
        if bg_value is not None:
            ff = ff - bg_value
        valid = ff[~np.isnan(ff)]
        ff = ff / (valid.max() if valid.size else np.nan)   # np.nanmax
        ffs = np.full_like(grid, np.nan)
        obj = np.full_like(devices, np.nan)
        devs = []
        k = 0
        while True:
            k += 1
            for n, q0, q1, qq0, qq1 in sl:
                obj[n, q0, q1] = devices[n, q0, q1] / ff[qq0, qq1]
            avgobj = nanmean0(obj)
            for n, q0, q1, qq0, qq1 in sl:
                ffs[n, qq0, qq1] = devices[n, q0, q1] / avgobj[q0, q1]
            ff2 = nanmean0(ffs)
            sq = (ff - ff2) ** 2
            ok = ~np.isnan(sq)
            dev = float(np.sqrt(sq[ok].sum() / ok.sum())) if ok.any() else np.nan   # RMS
            devs.append(dev)
            ff = ff2
            if dev < max_dev or k > max_iter + 1:
                break
    pointdensity = N - np.isnan(grid).sum(axis=0)
    return ff, avgobj, pointdensity, k, devs


def offset_meshgrid(offset, grid, shape):
    g0, g1 = grid
    s0, s1 = shape
    o0, o1 = offset
    o0 = -o0 / s0 * (g0 - 1)
    o1 = -o1 / s1 * (g1 - 1)
    xx, yy = np.meshgrid(np.linspace(o1, o1 + g1 - 1, s1), np.linspace(o0, o0 + g0 - 1, s0))
    return yy, xx


def grid_geometry(shape, positions):
    (f0, f1), cell_positions, (d0, d1) = positions
    s0, s1 = shape
    g0, g1 = int(s0 / d0) + 1, int(s1 / d1) + 1
    p0init, p1init = cell_positions[0]
    return (g0, g1), (f0 - d0 * p0init, f1 - d1 * p1init), (d0, d1)


def run(frames, n_cells_device, positions, bg_img=None, bg_value=0, thresh=None, max_iter=100, max_dev=1e-6):
    """the routine up to its post-processing -> grid, ff, avgobj, pointdensity, iterations, deviations"""
    frames = np.asarray(frames)
    n1, n0 = n_cells_device
    s0, s1 = frames.shape[1:]
    (g0, g1), p01, (d0, d1) = grid_geometry((s0, s1), positions)
    if thresh is None:
        thresh = bg_value
    grid = cell_means(frames, cell_edges(s0, g0, d0, p01[0]), cell_edges(s1, g1, d1, p01[1]), thresh, bg_img)
    return (grid,) + separate(grid, (n0, n1), positions[1], None if bg_img is not None else bg_value, max_iter,
                              max_dev)
