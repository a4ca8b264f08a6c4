"""Drop-in for `myutils.gradients`: the Sobel operator on the device (ebfi_amd/bcloss.py)."""
from ebfi_amd.bcloss import Sobel  # noqa: F401

__all__ = ["Sobel"]
