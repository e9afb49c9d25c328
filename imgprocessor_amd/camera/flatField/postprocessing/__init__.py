from .polynomial import polynomial  # noqa: F401
from .function import function  # noqa: F401
