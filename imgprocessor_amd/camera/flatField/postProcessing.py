"""``postProcessing`` — reference: imgProcessor/camera/flatField/postProcessing.py:11-74: close the
holes of a measured flat field before it goes into ``CameraCalibration.addFlatField``.  The methods
are those of K. Bedrich, M. Bokalic et al., "Electroluminescence imaging of PV devices: advanced flat
field calibration", 2017.

'POLY replace' (the field replaced by a 2-D polynomial fit of order 2 to its unmasked pixels) and 'POLY
repair' (the masked and the high-gradient areas replaced, iterated: postprocessing/polynomial.py) run
on the device.  The Kang-Weiss ('KW ...') and angle-of-view ('AoV ...') methods fit a function of the
pixel position through ``fancytools.fit.fit2dArrayToFn``, which does not exist here: they raise
NotImplementedError.
"""
from ...interpolate.polyfit2d import polyfit2dGrid
from .postprocessing.polynomial import polynomial

ppMETHODS = ['KW repair + Gauss', 'KW repair + Median',
             'KW replace', 'AoV replace', 'POLY replace',
             'POLY repair', 'KW repair', 'AoV repair']


def postProcessing(arr, method='KW replace + Gauss', mask=None, ctx=None):
    """arr: float32 / float64 flat field, host array or DeviceArray; mask: None or uint8 / bool of
    its shape, non-zero = invalid or empty.  The default method is the reference's - and, as there,
    not one of ppMETHODS: name a method."""
    assert method in ppMETHODS, \
        'post processing method (%s) must be one of %s' % (method, ppMETHODS)
    if method == 'POLY replace':
        return polyfit2dGrid(arr, mask, order=2, replace_all=True, ctx=ctx)
    if method == 'POLY repair':
        return polynomial(arr, mask, replace_all=False, ctx=ctx)
    raise NotImplementedError('postProcessing: %r needs fancytools.fit.fit2dArrayToFn, which this package '
                              'does not have; the POLY methods run on the device' % method)
