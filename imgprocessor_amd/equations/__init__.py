"""The vignetting models the flat-field post-processing fits (reference: imgProcessor/equations/):
``vignetting.vignetting`` (Kang-Weiss) and ``angleOfView.angleOfView``.  Host numpy functions."""
