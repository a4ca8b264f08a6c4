"""Drop-in for `myutils.iwe`: the reference module's five functions, on the device (ebfi_amd/iwe.py)."""
from ebfi_amd.iwe import purge_unfeasible, get_interpolation, interpolate, deblur_events, compute_pol_iwe  # noqa: F401

__all__ = ["purge_unfeasible", "get_interpolation", "interpolate", "deblur_events", "compute_pol_iwe"]
