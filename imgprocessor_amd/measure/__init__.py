"""Image quality measures (reference: imgProcessor/measure/)."""
