"""``getBackground2`` — reference: imgProcessor/utils/getBackground2.py:5-12."""
import numbers


def getBackground2(bgImages=None, img=None):
    """the background of the flat-field measurements: a number is returned as it is, a list or an
    (n, h, w) stack of background frames gives their ``imgAverage``.

    ``bgImages=None`` raises NotImplementedError: the reference takes the level from a resized
    histogram of ``img`` through imgSignal.scaleSignalCutParams and ``fancytools.findXAt``, which is
    not available here and is not part of the HIP path."""
    if bgImages is None:
        raise NotImplementedError(
            'getBackground2: estimating the background from the histogram of the image '
            '(scaleSignalCutParams, fancytools.findXAt) is not part of the HIP path: pass '
            'background frames or a number')
    if isinstance(bgImages, numbers.Number) and not isinstance(bgImages, bool):
        return bgImages
    from ..transform.imgAverage import imgAverage
    return imgAverage(bgImages)
