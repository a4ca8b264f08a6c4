"""Import-path shim: keeps the reference module layout importable on top of ebfi_amd."""
from .restore import CharbonnierLoss, perceptual_loss, psnr_loss, ssim_loss  # noqa: F401
