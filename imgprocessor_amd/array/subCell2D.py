"""Evenly sized sub-cells of a 2-D array - reference: imgProcessor/array/subCell2D.py.

``subCell2DSlices`` and ``subCell2DCoords`` are index arithmetic on the host and are what the
reference's are: the cell positions accumulate by repeated addition and are rounded with Python's
``round``.  ``ops.cell_edges`` holds the same positions as one table of edges per axis, clipped to the
frame - the form the device takes.

``subCell2DFnArray(arr, fn, shape)`` with an arbitrary Python function per cell is NOT built: a
function of the host cannot run on the device, and this package has no CPU fallbacks.  The one cell
function the reference's flat-field code uses - the thresholded mean of
camera/flatField/vignettingFromDiscreteSteps.py:228-234 - is ``ops.cell_means``, for all frames in
one pass.  ``subCell2DGenerator`` (slices applied to a host array) is plain numpy on the caller's side.
"""
from ..ops_steps import cell_edges


def _size(arr):
    return tuple(arr.shape[:2])


def subCell2DSlices(arr, shape, d01=None, p01=None):
    """Generator over the (i, j, row slice, column slice) of shape[0] x shape[1] evenly sized cells
    of `arr` (a host array or a DeviceArray: only its shape is read).

    Args:
       shape (tuple): number of sub-cells in y,x e.g. (10,15)
       d01 (tuple, optional): cell size in y and x
       p01 (tuple, optional): position of top left edge

    The slices are the reference's: bounds held at 0 but not clipped to the array (slicing clips)."""
    if p01 is not None:
        yinit, xinit = p01
    else:
        xinit, yinit = 0, 0
    g0, g1 = shape
    s0, s1 = _size(arr)
    if d01 is not None:
        d0, d1 = d01
    else:
        d0, d1 = s0 / g0, s1 / g1
    x, y = xinit, yinit
    y1 = d0 + yinit
    for i in range(g0):
        for j in range(g1):
            x1 = x + d1
            yield (i, j, slice(max(0, _rint(y)), max(0, _rint(y1))),
                   slice(max(0, _rint(x)), max(0, _rint(x1))))
            x = x1
        y = y1
        y1 = y + d0
        x = xinit


def subCell2DCoords(*args, **kwargs):
    """Same as subCell2DSlices but returning the corner coordinates ((x0, x0, x1), (y0, y1, y1))"""
    for _, _, s0, s1 in subCell2DSlices(*args, **kwargs):
        yield ((s1.start, s1.start, s1.stop),
               (s0.start, s0.stop, s0.stop))


def subCell2DEdges(arr, shape, d01=None, p01=None):
    """(row edges, column edges) of the same cells as two int32 tables clipped to the array, what
    ``ops.cell_means`` takes"""
    s0, s1 = _size(arr)
    g0, g1 = shape
    d0, d1 = d01 if d01 is not None else (s0 / g0, s1 / g1)
    p0, p1 = p01 if p01 is not None else (0, 0)
    return cell_edges(s0, g0, d0, p0), cell_edges(s1, g1, d1, p1)


def _rint(x):
    return int(round(x))
