"""filters/removeSinglePixels.py:4-30 on the device: clear every set pixel that has no set
neighbour among its <= 8 in-image neighbours."""
import numpy as np

from .. import ops
from ..device import DeviceArray


def removeSinglePixels(img):
    """clears, in place, every set pixel of ``img`` (a 2-D bool host array or a (h, w) uint8
    DeviceArray) none of whose in-image 8-neighbours is set"""
    if isinstance(img, DeviceArray):
        out = ops.remove_single_pixels(img)
        img.copy_from(out)
        return
    if not isinstance(img, np.ndarray) or img.ndim != 2:
        raise TypeError('removeSinglePixels takes a 2-D array')
    img[...] = ops.remove_single_pixels(img)
