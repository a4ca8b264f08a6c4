"""Drop-in for `dataloader.encodings`: every public function of the reference module, on the device (ebfi_amd/encodings.py)."""
from ebfi_amd.encodings import *  # noqa: F401,F403
from ebfi_amd.encodings import __all__  # noqa: F401
