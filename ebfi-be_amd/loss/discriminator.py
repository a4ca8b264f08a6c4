"""Import-path shim: the reference's loss/discriminator.py on top of ebfi_amd.gan (the STGAN discriminator only)."""
from ebfi_amd.gan import ST_Discriminator  # noqa: F401
