"""Index arithmetic on arrays of cells (reference: imgProcessor/array/)."""
from .subCell2D import subCell2DSlices, subCell2DCoords  # noqa: F401
