"""Drop-in for `loss.flow`: EventWarping and AveragedIWE on the device (ebfi_amd/iwe.py), with the three helpers the reference
module imports from myutils.iwe."""
from ebfi_amd.iwe import EventWarping, AveragedIWE  # noqa: F401
from ebfi_amd.iwe import purge_unfeasible, get_interpolation, interpolate  # noqa: F401

__all__ = ["EventWarping", "AveragedIWE", "purge_unfeasible", "get_interpolation", "interpolate"]
