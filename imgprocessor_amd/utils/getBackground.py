"""``getBackground`` — reference: imgProcessor/utils/getBackground.py:8-20."""
import numpy as np

from ..device import DeviceArray


def getBackground(bgImages):
    """None gives 0; one frame (alone, or a list / stack of one) gives that frame; more than one
    gives their single-time-effect-free average (DarkCurrentMap.averageSameExpTimes)"""
    if bgImages is None:
        return 0
    many = isinstance(bgImages, (tuple, list)) or (
        isinstance(bgImages, (np.ndarray, DeviceArray)) and bgImages.ndim == 3)
    if not many:
        return bgImages
    n = bgImages.shape[0] if isinstance(bgImages, DeviceArray) else len(bgImages)
    frames = [bgImages.frame(k) for k in range(n)] if isinstance(bgImages, DeviceArray) else bgImages
    if n > 1:
        from ..camera.DarkCurrentMap import averageSameExpTimes
        return averageSameExpTimes(frames)
    return frames[0]
