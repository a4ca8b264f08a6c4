"""Import-path shim: the reference's loss/adversarial.py on top of ebfi_amd.gan (gan_type='STGAN' only)."""
from ebfi_amd.gan import Adversarial  # noqa: F401
