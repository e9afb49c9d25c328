"""The discrete-steps family of ``ops`` (csrc/steps.hip), re-exported there as ``ops.cell_edges``,
``ops.cell_means``, ``ops.steps_separate``, ``ops.offset_meshgrid`` and ``ops.isnan_mask``: what
camera/flatField/vignettingFromDiscreteSteps.py does before its post-processing.  Like every family
it goes through ``_stage_in`` / ``_stage_out``: host arrays in give host arrays out, DeviceArrays stay
on the device.
"""
import ctypes as C

import numpy as np

from . import _lib as L
from .device import DeviceArray, dtype_id
from ._staging import PIXEL_DTYPES, _ctx_of, _is_dev, _px_host, _f64_host, _stage_in, _stage_out, frame_stack

MAX_FRAMES = 64      # kStepsMaxN of csrc/steps.hip
MAX_ITER = 10000     # kSepMaxIter
SEG_ROWS = 32        # kCellSegRows: the rows of one row segment of cell_means
MAX_PARTS = 1 << 24  # kCellMaxParts: frames * cell rows * row segments * cell columns
FLOAT_DTYPES = (np.float32, np.float64)


def cell_edges(size, g, d, p):
    """The g + 1 edges of the g cells of width `d` that start at position `p` along an axis of
    `size` pixels, as array/subCell2D.py:51-71 (subCell2DSlices) forms them - the position is
    accumulated by repeated addition, rounded with Python's ``round`` (half to even) and held at 0 -
    and clipped to `size`, which is what slicing the array does to them: cell k is
    [edges[k], edges[k + 1]), empty where the grid lies outside the frame.  Host arithmetic; -> int32."""
    size, g, d, acc = int(size), int(g), float(d), float(p)
    if size < 0 or g < 1:
        raise ValueError('cell_edges: needs a size >= 0 and at least one cell (got %d, %d)' % (size, g))
    if not d > 0 or not np.isfinite(d) or not np.isfinite(acc):
        raise ValueError('cell_edges: the cell size must be positive and finite, the position finite (got %r, %r)'
                         % (d, p))
    edges = np.empty(g + 1, np.int32)
    for k in range(g + 1):
        edges[k] = min(size, max(0, int(round(acc))))
        acc = acc + d
    return edges


def _edges(name, what, e, size):
    e = np.ascontiguousarray(e, dtype=np.int32)
    if e.ndim != 1 or e.size < 2:
        raise ValueError('%s: the %s edges must be a 1-D table of at least two entries' % (name, what))
    if e[0] < 0 or e[-1] > size or np.any(np.diff(e.astype(np.int64)) < 0):
        raise ValueError('%s: the %s edges must not decrease and must lie within [0, %d]' % (name, what, size))
    return e


def _float_host(a):
    a = np.asarray(a)
    return np.ascontiguousarray(a, dtype=a.dtype if a.dtype in FLOAT_DTYPES else np.float64)


def _ip(a):
    return a.ctypes.data_as(L._ip)


def cell_means(frames, row_edges, col_edges, thresh, bg=None, ctx=None):
    """camera/flatField/vignettingFromDiscreteSteps.py:228-246 for all frames in one pass -> float64
    (N, g0, g1): per cell [row_edges[i], row_edges[i + 1]) x [col_edges[j], col_edges[j + 1]) of
    x = float(frame) - float(bg) the mean of the samples x > thresh, NaN where fewer than half of
    the cell's pixels are such samples (2 * count < size, a NaN being none) or the cell is empty
    (ipa_cell_means_dev).  frames: a (N, h, w) array or a list of N frames, uint8 / uint16 /
    float32 / float64, 1 <= N <= 64 (ValueError below, NotImplementedError above); bg: None or one
    (h, w) frame of any of the four types; the edge tables as ``cell_edges`` gives them.  Two calls
    give identical bits.  NotImplementedError where N * g0 * ceil(tallest cell row / 32) * g1
    exceeds 2^24: the partial sums of the 32-row segments live in the context's workspace."""
    st = frame_stack('cell_means', frames)
    n = st.shape[0]
    if n < 1:
        raise ValueError('cell_means: needs at least one frame')
    if n > MAX_FRAMES:
        raise NotImplementedError('cell_means: at most %d frames (got %d)' % (MAX_FRAMES, n))
    dev, ctx, d, h, w = _stage_in('cell_means', st, ctx, PIXEL_DTYPES, _px_host, (bg,), ndims=(3,))
    re, ce = _edges('cell_means', 'row', row_edges, h), _edges('cell_means', 'column', col_edges, w)
    g0, g1 = re.size - 1, ce.size - 1
    d_bg = None
    if bg is not None:
        d_bg = bg if _is_dev(bg) else ctx.to_device(_px_host(bg))
        if d_bg.dtype not in PIXEL_DTYPES or tuple(d_bg.shape) != (h, w):
            raise ValueError('cell_means: bg must be a uint8 / uint16 / float32 / float64 frame of shape %s (got %s %s)'
                             % ((h, w), d_bg.dtype, tuple(d_bg.shape)))
    d_grid = DeviceArray(ctx, (n, g0, g1), np.float64)
    ctx._check(ctx._lib.ipa_cell_means_dev(
        ctx.handle, d.ptr, dtype_id(d.dtype), n, h, w, w, h * w, d_bg.ptr if d_bg is not None else None,
        dtype_id(d_bg.dtype) if d_bg is not None else 0, w, float(thresh), _ip(re), g0, _ip(ce), g1, d_grid.ptr),
        'cell_means')
    return _stage_out(dev, d_grid)


def device_grid_slices(n_cells, grid_shape, cell_positions):
    """camera/flatField/vignettingFromDiscreteSteps.py:26-60 (_DeviceAndGridSlice.iter) resolved:
    per frame (q0, q1, qq0, qq1, l0, l1) - device cells [q0, q0 + l0) x [q1, q1 + l1) are the grid
    cells [qq0, qq0 + l0) x [qq1, qq1 + l1) - as an int32 (N, 6) array.  n_cells = (n0, n1), rows
    first.  The reference's slices are taken as numpy takes them (a negative bound counts from the
    end); where a pair does not select equally many cells - a device that hangs over both the left
    and the right of the grid, or one that lies wholly outside - numpy's assignment fails and this
    raises its ValueError.  numpy would instead broadcast where the grid side of such a pair has
    length 1 (one grid row or column copied to several device rows); that is refused here too."""
    n0, n1 = int(n_cells[0]), int(n_cells[1])
    g0, g1 = int(grid_shape[0]), int(grid_shape[1])
    if n0 < 1 or n1 < 1 or g0 < 1 or g1 < 1:
        raise ValueError('device_grid_slices: empty device or grid')

    def axis(p, n, g):
        low, high = -1 < p, p + n <= g
        if low and high:
            q, qq = slice(None, n), slice(p, p + n)
        elif not low and high:
            q, qq = slice(-p, n), slice(None, p + n)
        elif not high and low:
            q, qq = slice(None, -(p + n - g)), slice(p, None)
        else:
            q, qq = slice(-p, -(p + n - g)), None
        return q, qq

    out = np.empty((len(cell_positions), 6), np.int32)
    for k, (p0, p1) in enumerate(cell_positions):
        p0, p1 = int(p0), int(p1)
        q0, qq0 = axis(p0, n0, g0)
        q1, qq1 = axis(p1, n1, g1)
        if qq0 is None:   # :59
            qq0 = slice(None, p0 + n0)
        if qq1 is None:   # :46
            qq1 = slice(p1, p1 + n1)
        r = [range(*s.indices(m)) for s, m in ((q0, n0), (q1, n1), (qq0, g0), (qq1, g1))]
        if len(r[0]) != len(r[2]) or len(r[1]) != len(r[3]):
            raise ValueError('could not broadcast input array from shape (%d,%d) into shape (%d,%d): frame %d at '
                             'cell position %s' % (len(r[2]), len(r[3]), len(r[0]), len(r[1]), k, (p0, p1)))
        out[k] = (r[0].start, r[1].start, r[2].start, r[3].start, len(r[0]), len(r[1]))
    return out


def steps_separate(grid, n_cells, cell_positions, bg_value=None, max_iter=100, max_dev=1e-6, ctx=None):
    """camera/flatField/vignettingFromDiscreteSteps.py:257-281 and :316 in one launch ->
    (ff, avgobj, pointdensity, iterations, dev): the flat field (float64 (g0, g1)), the averaged
    object (float64 (n0, n1)), the number of frames with a value per grid cell (int32 (g0, g1)), the
    iterations run and the last RMS deviation (ipa_steps_separate_dev).  grid: float64 (N, g0, g1),
    what ``cell_means`` returns, 1 <= N <= 64; n_cells = (n0, n1), the device's cells, rows first;
    cell_positions: N pairs (p0, p1), the grid cell of the device's first cell in every frame (they
    may be negative or leave the grid, see ``device_grid_slices``).  bg_value: subtracted from the
    initial flat field (:259-260: where there is no background image), None: nothing is.
    DEVIATION: the reference's `max_iter` never ends its loop, because the inner loops reuse the
    counter's name.  Here iteration k = 1, 2, ... is the last when dev < max_dev or k > max_iter + 1,
    what that counter would give: at most max_iter + 2 iterations, which a NaN deviation takes.
    0 <= max_iter <= 10000 (ValueError)."""
    dev, ctx, d, g0, g1 = _stage_in('steps_separate', grid, ctx, (np.float64,), _f64_host, ndims=(3,))
    n = d.shape[0]
    if n < 1:
        raise ValueError('steps_separate: needs at least one frame')
    if n > MAX_FRAMES:
        raise NotImplementedError('steps_separate: at most %d frames (got %d)' % (MAX_FRAMES, n))
    max_iter = int(max_iter)
    if not 0 <= max_iter <= MAX_ITER:
        raise ValueError('steps_separate: max_iter must lie in 0 ... %d (got %d)' % (MAX_ITER, max_iter))
    if len(cell_positions) != n:
        raise ValueError('steps_separate: %d cell positions for %d frames' % (len(cell_positions), n))
    if g0 < 1 or g1 < 1:
        raise ValueError('steps_separate: empty grid')
    n0, n1 = int(n_cells[0]), int(n_cells[1])
    rects = np.ascontiguousarray(device_grid_slices((n0, n1), (g0, g1), cell_positions))
    d_ff = DeviceArray(ctx, (g0, g1), np.float64)
    d_obj = DeviceArray(ctx, (n0, n1), np.float64)
    d_cnt = DeviceArray.counts(ctx, (g0, g1))
    it, last = C.c_int(0), C.c_double(0.0)
    ctx._check(ctx._lib.ipa_steps_separate_dev(
        ctx.handle, d.ptr, n, g0, g1, n0, n1, _ip(rects), 0.0 if bg_value is None else float(bg_value),
        0 if bg_value is None else 1, max_iter, float(max_dev), d_ff.ptr, d_obj.ptr, d_cnt.ptr, C.byref(it),
        C.byref(last)), 'steps_separate')
    return _stage_out(dev, d_ff), _stage_out(dev, d_obj), _stage_out(dev, d_cnt), it.value, last.value


def offset_axes(offset, grid, shape):
    """interpolate/offsetMeshgrid.py:18-26 up to the two np.linspace calls -> per axis
    (start, step, stop, length), np.linspace's own host arithmetic"""
    out = []
    for o, g, s in zip(offset, grid, shape):
        g, s = int(g), int(s)
        if g < 1 or s < 1:
            raise ValueError('offset_meshgrid: empty grid or shape')
        start = -o / s * (g - 1)
        stop = start + g - 1
        start, stop = float(start), float(stop)
        step = (stop - start) / (s - 1) if s > 1 else 0.0
        out.append((start, step, stop, s))
    return out


def offset_meshgrid(offset, grid, shape, dtype=np.float64, ctx=None):
    """interpolate/offsetMeshgrid.py on the device -> (yy, xx) DeviceArrays of `shape`: the positions
    on a (g0, g1) cell grid, shifted by `offset` pixels, of the pixels of a frame of `shape`
    (ipa_offset_meshgrid_dev).  Each axis is np.linspace bit for bit: i * step + start, the last
    element the stop.  dtype float64, or float32: the float64 value rounded once, the
    ``astype(np.float32)`` of vignettingFromDiscreteSteps.py:312.  Nothing of frame size is uploaded."""
    if np.dtype(dtype) not in FLOAT_DTYPES:
        raise TypeError('offset_meshgrid writes float32 / float64 (got %s)' % np.dtype(dtype))
    (a0, st0, b0, h), (a1, st1, b1, w) = offset_axes(offset, grid, shape)
    ctx = _ctx_of(ctx=ctx)
    d_yy, d_xx = DeviceArray(ctx, (h, w), dtype), DeviceArray(ctx, (h, w), dtype)
    ctx._check(ctx._lib.ipa_offset_meshgrid_dev(ctx.handle, a0, st0, b0, a1, st1, b1, h, w, dtype_id(d_yy.dtype),
                                                d_yy.ptr, d_xx.ptr, w), 'offset_meshgrid')
    return d_yy, d_xx


def isnan_mask(arr, ctx=None):
    """np.isnan(arr) of a float32 / float64 frame as a uint8 mask (ipa_isnan_mask_dev)"""
    dev, ctx, d, h, w = _stage_in('isnan_mask', arr, ctx, FLOAT_DTYPES, _float_host)
    if h < 1 or w < 1:
        raise ValueError('isnan_mask: empty frame')
    d_mask = DeviceArray(ctx, (h, w), np.uint8)
    ctx._check(ctx._lib.ipa_isnan_mask_dev(ctx.handle, d.ptr, dtype_id(d.dtype), h, w, w, d_mask.ptr, w),
               'isnan_mask')
    return _stage_out(dev, d_mask)
