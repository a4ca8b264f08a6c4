"""Drop-in for `loss.reconstruction`: BrightnessConstancy on the device (ebfi_amd/bcloss.py)."""
from ebfi_amd.bcloss import BrightnessConstancy  # noqa: F401

__all__ = ["BrightnessConstancy"]
