"""Feature detection (reference: imgProcessor/features/)."""
from .SingleTimeEffectDetection import SingleTimeEffectDetection  # noqa: F401
