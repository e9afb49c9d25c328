"""Flat field from spot images: the reference's camera/flatField/vignettingFromSpotAverage.py
("Method B" of K. Bedrich, M. Bokalic et al., Electroluminescence imaging of PV devices: advanced
flat field calibration, 2017).

One small bright device - an LCD display, a one-cell mini module - is imaged at many positions of
the image plane.  Per frame the background is subtracted, the spot is found as the largest connected
component of ``minimum_filter(img > t, 3)`` (t: Otsu's threshold unless `thresh` is given) and its
values go into a sparse array that is scaled by its largest spot value at the end.  The result and
the mask of valid positions are what ``postProcessing(fitimg, 'POLY replace', mask=~mask)`` takes.

Every frame pass runs in HIP kernels (csrc/spot.hip through ``ops.otsu_threshold``,
``ops.spot_mask``, ``ops.label``, ``ops.largest_component``, ``ops.spot_take``; csrc/flat.hip for the
background and the final division).  Per frame only the range, the histogram's counts, the number of
components and a handful of scalars reach the host; the sparse array and the mask stay on the device
until the end.  Frames are uint8 / uint16 / float32 / float64 arrays, host arrays or DeviceArrays
(a list of frames or one stack); host frames give (float64 array, bool array), device frames
(float64 DeviceArray, uint8 DeviceArray).

As the reference is written:
  - ``averageSpot=True`` (the default) does not average the spot.  ``spot`` becomes the integer pair
    ``[r, c] = rint(center_of_mass(spot))`` and ``img[spot]`` then indexes ROWS r and c of the frame:
    mx2 is the maximum of those two rows, both rows are copied into the result and both rows of the
    mask are set; a spot whose column c is >= the number of rows raises IndexError before anything
    of that frame is written.  This is reproduced, as the project reproduces the reference's other
    oddities (CameraCalibration.calcDarkCurrent, LensDistortion.distortImage).
  - ``averageSpot=False`` copies the spot's pixels and takes their mean for mx2.
  - a frame without a component prints ``couldn't find spot in image`` and is skipped; no spot in
    any frame divides by zero as numpy does (NaN / inf, no exception).
  - the progress lines ``1/n``, ``2/n``, ... are printed.

Differences from the reference:
  - ``bgImages=None`` raises NotImplementedError (see utils/getBackground2.py).
  - frames are grey arrays, not file paths or colour frames (TypeError).
  - the mean of ``averageSpot=False`` is a sum in the device's fixed order divided by the count: it
    may differ from numpy's pairwise sum in the last digits (the bound of any summation order,
    count * 2**-53 * sum|x|), identical from call to call.
"""
from __future__ import print_function

import numpy as np

from ... import ops
from ...device import default_context
from ...ops_spot import _zeros
from ...utils.getBackground2 import getBackground2
from .flatFieldFromCloseDistance import _average_bg, _background, _ctx_of, _on_device, _stack


def vignettingFromSpotAverage(images, bgImages=None, averageSpot=True, thresh=None):
    """[images] --> frames of one small bright spot at different positions of the image plane

    Args:
        averageSpot(bool): see the module's text: True takes the two rows the reference takes
        thresh(float): marks the minimum spot value (estimated with Otsu's method otherwise)

    Returns:
        * array to be post processed
        * image mask containing valid positions
    """
    name = 'vignettingFromSpotAverage'
    if bgImages is None:
        getBackground2(None)
    dev, n, shape, st = _stack(name, images, (2, 3))
    if n and len(shape) == 3:
        raise TypeError('%s takes grey frames (got frames of shape %s)' % (name, shape))
    if n < 1:
        raise ValueError('%s: no images' % name)
    bg = _background(name, bgImages, shape)
    t = None if thresh is None else float(thresh)
    # ---- nothing above touches a device
    ctx = _ctx_of(st) if dev else default_context()
    h, w = shape
    d = _on_device(ctx, st)
    fitimg, mask = _zeros(ctx, (h, w), np.float64), _zeros(ctx, (h, w), np.uint8)
    mx = 0
    for c in range(n):
        print('%s/%s' % (c + 1, n))
        if c == 0:
            bg = _average_bg(ctx, bg)
        img = d.frame(c)
        # find spot:
        tc = ops.otsu_threshold(img, bg=bg) if t is None else t
        # take brightest spot
        spots, n_spots = ops.label(ops.spot_mask(img, tc, bg=bg))
        spot = ops.largest_component(spots, n_spots)
        if spot is None:
            print("couldn't find spot in image")
            continue
        label, size, (sum_y, sum_x) = spot
        if averageSpot:
            # np.rint(center_of_mass(spot)).astype(int), then img[spot]: two rows
            r, col = (int(v) for v in np.rint([sum_y / float(size), sum_x / float(size)]))
            if col >= h:
                raise IndexError('index %d is out of bounds for axis 0 with size %d' % (col, h))
            mx2 = ops.spot_take(img, rows=(r, col), bg=bg, fit=fitimg, mask=mask)[2]
        else:
            total, count = ops.spot_take(img, spots, label, bg=bg, fit=fitimg, mask=mask)[3:]
            mx2 = total / count
        if mx2 > mx:
            mx = mx2
    # scale [0...1]:
    ops.flat_scale(fitimg, div=mx, out=fitimg)
    return (fitimg, mask) if dev else (fitimg.get(), mask.get().astype(bool))
