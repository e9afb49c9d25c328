from .vignettingFromDiscreteSteps import (rescaleToGrid, vignettingFromDiscreteSteps,  # noqa: F401
                                          positionsFromRaster, positionsFromTopLeftCorner)
from .flatFieldFromCloseDistance import (flatFieldFromCloseDistance,  # noqa: F401
                                         flatFieldFromCloseDistance2)
from .sensitivity import sensitivity  # noqa: F401
from .postProcessing import postProcessing, ppMETHODS  # noqa: F401
from .postprocessing.polynomial import polynomial  # noqa: F401
from .postprocessing.function import function  # noqa: F401
from .vignettingFromSpotAverage import vignettingFromSpotAverage  # noqa: F401
