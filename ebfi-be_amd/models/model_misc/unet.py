"""Drop-in for `models.model_misc.unet`: the recurrent U-Nets (MultiResUNet, which is not recurrent, is not provided)."""
from ebfi_amd.unet import BaseUNet, BaseUNet_legacy, SRUNetRecurrent, UNetFlow, UNetRecurrent  # noqa: F401
