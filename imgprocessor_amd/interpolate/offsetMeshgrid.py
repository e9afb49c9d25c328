"""``offsetMeshgrid`` - reference: imgProcessor/interpolate/offsetMeshgrid.py: cell averages
[grid] lie on an image, the top-left position of the grid within the image is [offset]; the result is
the meshgrid that upscales [grid] to [shape] resolution.

The two np.linspace axes are formed on the host (a start, a step and a stop each); a kernel writes the
two frame-sized arrays (csrc/steps.hip: ipa_offset_meshgrid_dev), bit for bit what np.meshgrid of
the two np.linspace gives.
"""
import numpy as np

from .. import ops


def offsetMeshgrid(offset, grid, shape, dtype=np.float64, ctx=None, device=False):
    """offset(y, x) e.g. (0, 0) if no offset; grid(ny, nx) resolution of the smaller grid;
    shape(y, x) -> output shape.  Returns (yy, xx) as host arrays, or as DeviceArrays with
    device=True (what polyfit2dGrid's outgrid and rescaleToGrid take without an upload).
    dtype float32 rounds the float64 positions once (np.float32 maps for a remap)."""
    yy, xx = ops.offset_meshgrid(offset, grid, shape, dtype=dtype, ctx=ctx)
    return (yy, xx) if device else (yy.get(), xx.get())
