"""Flat field from discrete steps: the reference's camera/flatField/vignettingFromDiscreteSteps.py
("Method D" of K. Bedrich, M. Bokalic et al., Electroluminescence imaging of PV devices: advanced
flat field calibration, 2017, for a device that is moved by whole cells between the frames).

A device of n_cells_device cells is imaged at known positions of a grid of cells on the image plane.
Every frame is reduced to the thresholded mean of every grid cell (``ops.cell_means``: one pass over
all frames, csrc/steps.hip), device and flat field are separated iteratively on that grid
(``ops.steps_separate``: the whole loop of :257-281 in one launch), and the flat field on the grid is
brought to image resolution by the post-processing the reference has in this function: 'POLY replace'
(``polyfit2dGrid(ff, isnan(ff), order=5, outgrid=offsetMeshgrid(...))``) or 'POLY repair'
(``polyfit2dGrid(ff, isnan(ff), order=3)`` and ``rescaleToGrid``, Lanczos4 with a reflecting border).
The positions come from ``positionsFromRaster`` or ``positionsFromTopLeftCorner``, plain host
arithmetic.  Frames are uint8 / uint16 / float32 / float64 grey arrays, host arrays or DeviceArrays (a
list of frames or one stack, at most 64); host frames give host arrays, device frames DeviceArrays -
nothing of frame size crosses the bus then, the two coordinate arrays included.

Differences from the reference:
  - the default `postprocessing_method` is 'POLY replace'; the reference's default, 'polynomial',
    fails its own assertion.
  - the 'KW ...' and 'AoV ...' methods raise NotImplementedError, as in ``postProcessing``.
  - ``visualize=True`` raises NotImplementedError (matplotlib windows per frame).
  - `max_iter`: the reference's inner loops reuse the name `n` of its iteration counter, so its
    `max_iter` never ends the loop (unless there are more than max_iter + 1 frames, which ends it
    after the first pass).  A loop that may never end does not run on a GPU: iteration k = 1, 2, ...
    is the last when dev < max_dev or k > max_iter + 1 - what the counter would give - and a NaN
    deviation runs to that cap.  max_iter above 10000 is a ValueError.
  - a device position whose slices (:26-60) do not select equally many device and grid cells - a
    device hanging over both the left and the right side of the grid, or lying wholly outside it - is
    the ValueError numpy's assignment raises at :249; where the grid side of such a pair has length 1
    numpy would broadcast it instead, which is refused too.
  - frames and background are arrays, not file paths (TypeError); more than 64 frames raise
    NotImplementedError.
  - the polynomial fits are this package's ``polyfit2dGrid``: where the grid's valid cells do not
    determine the polynomial (order 5 needs six valid rows and columns of cells) it raises ValueError,
    where the reference returns lstsq's minimum-norm answer.
  - the cell means are sums in the device's fixed order, not numpy's pairwise sums: they may differ
    in the last digits and are identical from call to call.  `pointdensity` is int32.
"""
import numpy as np

from ... import ops
from ..._staging import _ctx_of, _is_dev, _px_host, frame_stack
from ...ops_steps import MAX_FRAMES, cell_edges, device_grid_slices
from ...interpolate.polyfit2d import polyfit2dGrid

METHODS = ('POLY replace', 'KW replace', 'AoV replace', 'POLY repair', 'KW repair', 'AoV repair')


def positionsFromRaster(initial_cell_position, nimgs, nimgrow, cell_size, initial_px_position, direction,
                        first_axis):
    """input function for argument [positions] in vignettingFromDiscreteSteps()
    to be used, if device positions changes like a raster first monotonously in one direction, then
    in another, like (0,0),(1,0),(2,0),(0,1),(1,1)...

    initial_cell_position(x,y) --> position of the device in first image
    nimgrow -> how many images are taken until the device jumps to the next column
    cell_size(x,y) --> number of pixels of one cell/step in x and y
    initial_px_position(x,y) --> pixel position of bottom left in the image
    direction (-1,1) --> first direction of the positional change of the device
    first_axis(0,1) -> whether major direction is in y(0) or x(1)
    """
    assert first_axis in (0, 1)
    assert direction in (-1, 1)
    p1, p0 = p1init, p0init = initial_cell_position
    cell_positions = []
    c = 1
    for _ in range(nimgs):
        cell_positions.append((p0, p1))
        if first_axis == 0:
            p0 += direction
            if c == nimgrow:
                p0 = p0init
                p1 += 1
                c = 0
        else:
            p1 += direction
            if c == nimgrow:
                p1 = p1init
                p0 += 1
                c = 0
        c += 1
    f1, f0 = initial_px_position
    d1, d0 = cell_size
    return (f0, f1), cell_positions, (d0, d1)


def positionsFromTopLeftCorner(pos, cell_size):
    """input function for argument [positions] in vignettingFromDiscreteSteps()
    to be used, if corner positions [pixels] of the device are known

    pos ((x,y),...) -> all pixel positions of the TOP LEFT corner of the device
    cell_size(x,y) --> number of pixels of one cell/step in x and y
    """
    d1, d0 = cell_size
    f1, f0 = pos[0]
    p1init = int(f1 / d1) + 1 if f1 > 0 else 0
    p0init = int(f0 / d0) + 1 if f0 > 0 else 0
    ref1 = f1 - p1init * d1
    ref0 = f0 - p0init * d0
    cell_positions = [(p0init, p1init)]
    for x, y in pos[1:]:
        cell_positions.append((int(round((y - ref0) / d0)), int(round((x - ref1) / d1))))
    return (f0, f1), cell_positions, (d0, d1)


def rescaleToGrid(ff, xx, yy):
    """ff sampled at the (sub-pixel) grid positions xx, yy - Lanczos4, reflecting border
    (fedcba|abcdef, cv2.BORDER_REFLECT)"""
    return ops.remap(np.asarray(ff), np.asarray(xx).astype(np.float32),
                     np.asarray(yy).astype(np.float32), 'lanczos4', 'reflect', 0.0)


def grid_geometry(shape, positions):
    """:210-217, :244-245 -> ((g0, g1), p01, (d0, d1)): the resolution of the cell grid on a frame of
    `shape`, the pixel position of its top left corner and the cell size"""
    (f0, f1), cell_positions, (d0, d1) = positions
    s0, s1 = shape
    g0, g1 = int(s0 / d0) + 1, int(s1 / d1) + 1
    p0init, p1init = cell_positions[0]
    return (g0, g1), (f0 - d0 * p0init, f1 - d1 * p1init), (d0, d1)


def vignettingFromDiscreteSteps(imgs, n_cells_device, positions, bg_img=None, bg_value=0, thresh=None,
                                postprocessing_method='POLY replace', visualize=False, max_iter=100,
                                max_dev=1e-6, ctx=None):
    """imgs --> all images in the right order
    n_cells_device(x,y) --> how many cells does the device have
    positions --> output of either [positionsFromTopLeftCorner] or [positionsFromRaster]
    bg_value -> in order to exclude background when averaging set this value to > 0;
                if bg_img is given, bg_value should be a threshold between background and signal
    thresh --> image intensity separating background from signal (None: bg_value)
    postprocessing_method --> 'POLY replace': replace the grid with a 2d polynomial fit;
                              'POLY repair': fit only the empty cells, then rescale
    max_iter --> maximum number of iterations (see the module's text)
    max_dev --> break iteration, if deviation between consecutive vignetting arrays < [max_dev]

    Returns (ff, ff2, avgobj, pointdensity): the flat field on the cell grid, the flat field at image
    resolution, the averaged device and the number of frames behind every grid cell."""
    name = 'vignettingFromDiscreteSteps'
    assert postprocessing_method in METHODS, \
        'post processing method (%s) must be one of %s' % (postprocessing_method, METHODS)
    if not postprocessing_method.startswith('POLY'):
        raise NotImplementedError('%s: %r needs fancytools.fit.fit2dArrayToFn, which this package does not have; '
                                  'the POLY methods run on the device' % (name, postprocessing_method))
    if visualize:
        raise NotImplementedError('%s: visualize=True opens matplotlib windows per frame and is not built' % name)
    if isinstance(imgs, str) or isinstance(bg_img, str) or (
            not _is_dev(imgs) and not isinstance(imgs, np.ndarray) and any(isinstance(i, str) for i in imgs)):
        raise TypeError('%s takes arrays, not file paths' % name)
    frames = frame_stack(name, imgs)
    n = frames.shape[0]
    if n < 1:
        raise ValueError('%s: no images' % name)
    if n > MAX_FRAMES:
        raise NotImplementedError('%s: at most %d images (got %d)' % (name, MAX_FRAMES, n))
    cell_positions = positions[1]
    if len(cell_positions) != n:
        raise ValueError('%s: %d positions for %d images' % (name, len(cell_positions), n))
    n1, n0 = n_cells_device
    s0, s1 = frames.shape[1:]
    (g0, g1), p01, (d0, d1) = grid_geometry((s0, s1), positions)
    if thresh is None:
        thresh = bg_value
    # the host checks of the loop before anything runs on the device
    device_grid_slices((n0, n1), (g0, g1), cell_positions)
    row_edges, col_edges = cell_edges(s0, g0, d0, p01[0]), cell_edges(s1, g1, d1, p01[1])
    dev = _is_dev(frames)
    ctx = _ctx_of(frames, bg_img, ctx=ctx)
    if not dev:   # host frames go up once; everything after them stays on the device until the end
        frames = ctx.to_device(_px_host(frames))
        if bg_img is not None and not _is_dev(bg_img):
            bg_img = ctx.to_device(_px_host(bg_img))
    grid = ops.cell_means(frames, row_edges, col_edges, thresh, bg=bg_img)
    ff, avgobj, pointdensity, _, _ = ops.steps_separate(grid, (n0, n1), cell_positions,
                                                        bg_value=bg_value if bg_img is None else None,
                                                        max_iter=max_iter, max_dev=max_dev)
    mask = ops.isnan_mask(ff)
    if postprocessing_method == 'POLY replace':
        ff2 = polyfit2dGrid(ff, mask, order=5, outgrid=ops.offset_meshgrid(p01, (g0, g1), (s0, s1), ctx=ctx))
    else:   # 'POLY repair': the repaired grid is also the first result, as in the reference
        ff = polyfit2dGrid(ff, mask, order=3)
        yy, xx = ops.offset_meshgrid(p01, (g0, g1), (s0, s1), dtype=np.float32, ctx=ctx)
        ff2 = ops.remap(ff, xx, yy, 'lanczos4', 'reflect', 0.0)
    if not dev:
        ff, ff2, avgobj, pointdensity = ff.get(), ff2.get(), avgobj.get(), pointdensity.get()
    return ff, ff2, avgobj, pointdensity
