"""Scenes and case lists of the discrete-steps tests (tests/test_cpu_steps.py, tests/test_gpu_steps.py,
tests/golden/gen_steps_golden.py).  Everything is seeded; the fixture holds arrays only and stores the
sums of every scene's inputs, so a scene that drifts from the fixture is noticed.

A scene is a device of n_cells_device cells with one brightness per cell, imaged through a smooth flat
field at the cell positions that positionsFromRaster / positionsFromTopLeftCorner give; the cells are
(11.5, 13.25) pixels with a non-zero pixel offset throughout, the frames 66 x 90: a grid of 6 x 7 cells whose
last row and column are cut by the frame.  Every grid cell is covered by the device in some frame, so that
the order-5 polynomial of 'POLY replace' is determined; in three scenes one cell is dead (dark in every frame)
and stays NaN in the flat field.
"""
import numpy as np

from . import steps_ref as ref

SEG_ROWS = 32      # rows of one row segment of ipa_cell_means_dev (kCellSegRows): a taller cell has several
CHUNK_COLS = 256   # columns of one chunk of that kernel: a wider cell is carried from chunk to chunk

SHAPE = (66, 90)
CELL = (11.5, 13.25)   # d0, d1
MAX_ITER, MAX_DEV = 100, 1e-6

# The largest relative difference between the reference's ff / avgobj (cell means through numpy's pairwise
# sums) and the restatement's (cell means through math.fsum) over all scenes, as tests/golden/
# gen_steps_golden.py measures and prints it.  The whole routine on the device is held to 100 x this
# and not below 1e-12.
MEASURED_REL = 5.63e-16
ROUTINE_TOL = max(100 * MEASURED_REL, 1e-12)


def positions_raster(initial_cell, nimgs, nimgrow, px=(5.0, 3.0), direction=1, first_axis=1):
    """positionsFromRaster restated: (x, y) arguments, (axis 0, axis 1) results"""
    p1, p0 = p1init, p0init = initial_cell
    cp, c = [], 1
    for _ in range(nimgs):
        cp.append((p0, p1))
        if first_axis == 0:
            p0 += direction
            if c == nimgrow:
                p0, p1, c = p0init, p1 + 1, 0
        else:
            p1 += direction
            if c == nimgrow:
                p1, p0, c = p1init, p0 + 1, 0
        c += 1
    return (px[1], px[0]), cp, CELL


def flat_field(shape):
    y, x = np.mgrid[0:shape[0], 0:shape[1]].astype(np.float64)
    cy, cx = 0.45 * shape[0], 0.55 * shape[1]
    r2 = ((y - cy) / shape[0]) ** 2 + ((x - cx) / shape[1]) ** 2
    return 1.0 / (1.0 + 1.8 * r2)


def render(positions, n_cells_device, seed, dtype, gain, bg_level, noise, dead=None, shape=SHAPE):
    """-> (frames (N, h, w) of `dtype`, the device's cell brightnesses): frame k shows the device at
    cell_positions[k] on the grid of steps_ref.grid_geometry, times the flat field, plus bg_level; the pixels
    of grid cell `dead` carry no signal in any frame"""
    rng = np.random.default_rng(seed)
    n1, n0 = n_cells_device
    (g0, g1), p01, (d0, d1) = ref.grid_geometry(shape, positions)
    re, ce = ref.cell_edges(shape[0], g0, d0, p01[0]), ref.cell_edges(shape[1], g1, d1, p01[1])
    obj = 0.6 + 0.4 * rng.random((n0, n1))
    V = flat_field(shape)
    frames = []
    for p0, p1 in positions[1]:
        f = np.zeros(shape)
        for a in range(n0):
            for b in range(n1):
                i, j = p0 + a, p1 + b
                if 0 <= i < g0 and 0 <= j < g1:
                    f[re[i]:re[i + 1], ce[j]:ce[j + 1]] = obj[a, b]
        if dead is not None:
            f[re[dead[0]]:re[dead[0] + 1], ce[dead[1]]:ce[dead[1] + 1]] = 0.0
        f = gain * f * V * (1.0 + noise * rng.standard_normal(shape)) + bg_level
        frames.append(f)
    frames = np.stack(frames)
    if np.dtype(dtype).kind == 'u':
        frames = np.clip(np.rint(frames), 0, np.iinfo(dtype).max)
    return frames.astype(dtype), obj


def scenes():
    """name -> dict(frames, n_cells_device, positions, kw): the keyword arguments are the routine's"""
    out = {}
    d0, d1 = CELL
    # float64 frames with bg_value; the device stays inside the grid
    pos = positions_raster((0, 0), 20, 5)
    fr, _ = render(pos, (3, 3), 1, np.float64, 1.0, 0.05, 0.01, dead=(2, 3))
    out['f64_bgvalue'] = dict(frames=fr, n_cells_device=(3, 3), positions=pos, kw=dict(bg_value=0.1))
    # uint16 frames with a background image and a threshold
    pos = positions_raster((0, 0), 20, 5)
    fr, _ = render(pos, (3, 3), 2, np.uint16, 4000.0, 0.0, 0.01, dead=(0, 0))
    rng = np.random.default_rng(22)
    bg = (100 + 10 * rng.random(SHAPE)).astype(np.uint16)
    fr = (fr + bg[None]).astype(np.uint16)
    out['u16_bgimg'] = dict(frames=fr, n_cells_device=(3, 3), positions=pos, kw=dict(bg_img=bg, bg_value=0, thresh=300))
    # the device leaves the grid at top / left (negative cell positions) and at bottom / right; its first
    # position lies one cell outside the frame, so that the grid still starts at pixel (3, 5)
    pos = positions_raster((-1, -1), 42, 7, px=(5.0 - d1, 3.0 - d0))
    fr, _ = render(pos, (3, 3), 3, np.float64, 1.0, 0.02, 0.01)
    out['leaves_grid'] = dict(frames=fr, n_cells_device=(3, 3), positions=pos, kw=dict(bg_value=0.05))
    # a device taller than the grid, hanging over its top and bottom: the fourth branch of axis 0
    pos = positions_raster((0, -1), 5, 5, px=(5.0, 3.0 - d0))
    fr, _ = render(pos, (3, 8), 4, np.float32, 1.0, 0.02, 0.01)
    out['tall_device'] = dict(frames=fr, n_cells_device=(3, 8), positions=pos, kw=dict(bg_value=0.05))
    # pixel positions of the device's top left corner: the grid starts above / left of the frame
    ref0, ref1 = 14.5 - d0 * 2, 18.25 - d1 * 2
    order = [(2, 2)] + [(r, c) for r in range(4) for c in range(5) if (r, c) != (2, 2)]
    corners = [(ref1 + d1 * c + 0.1 * ((3 * k) % 7 - 3), ref0 + d0 * r + 0.1 * ((5 * k) % 7 - 3)) if k else
               (ref1 + d1 * c, ref0 + d0 * r) for k, (r, c) in enumerate(order)]
    out['top_left_corner'] = dict(corners=corners, cell_size=(d1, d0), n_cells_device=(3, 3), dead=(3, 2),
                                  kw=dict(bg_value=0.05))
    return out


def corner_positions(corners, cell_size):
    """positionsFromTopLeftCorner restated"""
    d1, d0 = cell_size
    f1, f0 = corners[0]
    p1init = int(f1 / d1) + 1 if f1 > 0 else 0
    p0init = int(f0 / d0) + 1 if f0 > 0 else 0
    ref1, ref0 = f1 - p1init * d1, f0 - p0init * d0
    cp = [(p0init, p1init)]
    for x, y in corners[1:]:
        cp.append((int(round((y - ref0) / d0)), int(round((x - ref1) / d1))))
    return (f0, f1), cp, (d0, d1)


def finish(sc):
    """fill in what the corner scene derives: its positions and frames"""
    if 'corners' in sc:
        sc['positions'] = corner_positions(sc['corners'], sc['cell_size'])
        sc['frames'], _ = render(sc['positions'], sc['n_cells_device'], 5, np.float64, 1.0, 0.02, 0.01, dead=sc['dead'])
    return sc


def all_scenes():
    return {k: finish(v) for k, v in scenes().items()}


# ---------------------------------------------------------------------------------- cell_means cases
def _img(shape, dtype, seed, n=1):
    rng = np.random.default_rng(seed)
    a = rng.random((n,) + tuple(shape))
    if np.dtype(dtype).kind == 'u':
        return (a * min(np.iinfo(dtype).max, 4000)).astype(dtype)
    return (a * 2 - 0.5).astype(dtype)


def cell_cases():
    """name -> (frames (N, h, w), row_edges, col_edges, thresh, bg)"""
    E = ref.cell_edges
    c = {}
    c['frame_1x1'] = (np.array([[[7]]], np.uint8), [0, 1], [0, 1], 3, None)
    c['cells_1px'] = (_img((5, 7), np.float32, 1, 2), np.arange(6), np.arange(8), 0.1, None)
    c['one_cell'] = (_img((37, 300), np.uint16, 2), [0, 37], [0, 300], 100, None)   # wider than a chunk
    c['c67x131'] = (_img((270, 480), np.uint16, 3, 2), E(270, 5, 67, 0), E(480, 4, 131, 0), 500,
                    _img((270, 480), np.float32, 4)[0] * 100)
    # cells of 70 rows: three row segments of SEG_ROWS = 32, the last of 6 rows
    c['tall_70'] = (_img((150, 40), np.float64, 5), E(150, 3, 70, 3), E(40, 2, 19.5, 1), 0.0, None)
    # the grid starts above / left of the frame and ends beyond it: empty cells at both ends
    c['outside'] = (_img((60, 84), np.float64, 6, 3), E(60, 9, 11.5, -20.0), E(84, 10, 13.25, -30.5), 0.2, None)
    # cells wider than a chunk that start at column 7 and straddle the chunk boundaries at 256 and 512
    c['wide_offset'] = (_img((40, 700), np.float64, 7), E(40, 2, 33, 2), E(700, 3, 300.5, 7.0), 0.0, None)
    # 24-pixel cells: exactly half the pixels are samples (kept), one fewer (NaN)
    f = np.zeros((1, 4, 12), np.uint8)
    f[0, :, :3] = 9     # cell 0: 12 of 24
    f[0, :, 6:9] = 9    # cell 1: 12, then one taken away
    f[0, 3, 8] = 0
    c['majority'] = (f, [0, 4], [0, 6, 12], 5, None)
    # samples exactly on the threshold do not count: cell 0 keeps 4 of 8, cell 1 has 3 of 8
    f = np.full((1, 2, 8), 0.5)
    f[0, :, :2] = 1.5
    f[0, 0, 4:7] = 2.5
    c['on_thresh'] = (f, [0, 2], [0, 4, 8], 0.5, None)
    f = _img((30, 45), np.float32, 8, 2)
    f[0, 3:9, 5:20] = np.nan
    f[1, ::3, ::2] = np.nan
    c['nan_f32'] = (f, E(30, 3, 11.5, 2), E(45, 4, 13.25, 1), 0.0, None)
    g = f.astype(np.float64)
    c['nan_f64_bg'] = (g, E(30, 3, 11.5, 2), E(45, 4, 13.25, 1), -0.8, _img((30, 45), np.uint8, 9)[0] // 128)
    c['n64'] = (_img((20, 30), np.uint8, 10, 64), E(20, 2, 9.5, 1), E(30, 3, 9.25, 2), 100, None)
    return c


ALL_DTYPES = (np.uint8, np.uint16, np.float32, np.float64)


def dtype_case(dtype, bg_dtype):
    """a (2, 45, 70) scene of `dtype` with cells of (11.5, 13.25) from (3, 5), bg of `bg_dtype` or None"""
    f = _img((45, 70), dtype, 30, 2)
    fl = np.dtype(dtype).kind == 'f'
    bg = None
    if bg_dtype is not None:
        bg = _img((45, 70), bg_dtype, 31)[0]
        if np.dtype(bg_dtype).kind == 'u':   # 0 / 1 under float frames, up to 6 or 100 under integer frames
            bg = bg // (np.array(bg.max() // 2 + 1 if fl else 40, bg_dtype))
    thresh = (0.1 if bg is None else -0.7) if fl else 60
    return f, ref.cell_edges(45, 4, 11.5, 3), ref.cell_edges(70, 6, 13.25, 5), thresh, bg


def separate_cases():
    """name -> (grid, n_cells, cell_positions, kw, expectation)"""
    rng = np.random.default_rng(40)
    out = {}
    pos = positions_raster((0, 0), 6, 3)[1]
    g = 0.5 + rng.random((6, 4, 5))
    out['plain'] = (g, (3, 3), pos, dict(bg_value=0.1), None)
    out['n1'] = (0.5 + rng.random((1, 4, 5)), (3, 3), [(0, 1)], dict(), None)
    g2 = g.copy()
    g2[:, 1, 2] = np.nan          # a grid cell that is NaN in every frame
    g2[2, 0, 0] = np.nan
    out['all_nan_cell'] = (g2, (3, 3), pos, dict(bg_value=None), None)
    g3 = g.copy()
    # a zero flat-field cell under a device cell that only one frame sees: 1 / 0 -> inf, which stays
    g3[:, 3, 4] = np.nan
    g3[5, 3, 4], g3[0, 3, 4] = 1.0, -1.0
    out['zero_cell'] = (g3, (3, 3), pos, dict(bg_value=None, max_iter=4, max_dev=0.0), 'inf')
    out['cap'] = (g, (3, 3), pos, dict(max_dev=0.0, max_iter=3), 5)   # runs to the cap: max_iter + 2
    return out
