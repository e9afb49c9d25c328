"""Signal-to-noise maps (reference: imgProcessor/measure/SNR/)."""
from .SNR import SNR, getBackgroundLevel  # noqa: F401
