from .geometry import (genericCameraMatrix, sortCorners, getPerspectiveTransform,  # noqa: F401
                       getOptimalNewCameraMatrix, perspectiveTransform)
from .getBackground import getBackground  # noqa: F401
from .getBackground2 import getBackground2  # noqa: F401
