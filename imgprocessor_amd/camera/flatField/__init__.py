from .vignettingFromDiscreteSteps import rescaleToGrid  # noqa: F401
from .flatFieldFromCloseDistance import (flatFieldFromCloseDistance,  # noqa: F401
                                         flatFieldFromCloseDistance2)
from .sensitivity import sensitivity  # noqa: F401
