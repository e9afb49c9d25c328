"""``imgAverage`` — reference: imgProcessor/transform/imgAverage.py:7-22.

The float64 mean of a list or an (n, h, w) stack of frames: the sum in frame order, then divided by
the number of frames, bit for bit numpy's ``out += f; out /= n`` (csrc/flat.hip, ops.stack_mean).
uint8 / uint16 / float32 / float64 frames, grey (h, w) or colour (h, w, 3); host arrays give a host
array, DeviceArrays a DeviceArray.  Frames are arrays, not file paths (TypeError).
"""
from .. import ops


def imgAverage(images, copy=True, ctx=None):
    """``copy`` is accepted for the reference's signature: the result is always a new array"""
    if not hasattr(images, 'shape'):
        if isinstance(images, (str, bytes)):
            raise TypeError('imgAverage takes arrays, not file paths')
        images = list(images)
        if any(isinstance(i, (str, bytes)) or hasattr(i, '__fspath__') for i in images):
            raise TypeError('imgAverage takes arrays, not file paths')
    if (images.shape[0] if hasattr(images, 'shape') else len(images)) < 1:
        raise ValueError('imgAverage: no images')
    return ops.stack_mean(images, ctx=ctx)
