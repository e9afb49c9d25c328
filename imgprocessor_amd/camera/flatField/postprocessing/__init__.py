from .polynomial import polynomial  # noqa: F401
