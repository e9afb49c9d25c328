"""Non-local-means denoising on the device: what camera/CameraCalibration.py:461-474 gets from
skimage.restoration.denoise_nl_means, as a numpy-in, numpy-out filter."""
import numpy as np

from .. import ops


def denoiseNLMeans(img, **kw):
    """``img``: a 2-D (or (n, h, w) batch) float32 / float64 host array; keywords as
    ops.nl_means (patch_size=7, patch_distance=11, h=0.1, sigma=0.0).  Returns a new array."""
    if not isinstance(img, np.ndarray):
        raise TypeError('denoiseNLMeans takes a numpy array (ops.nl_means takes DeviceArrays)')
    return ops.nl_means(img, **kw)
