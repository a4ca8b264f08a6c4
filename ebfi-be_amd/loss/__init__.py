"""Import-path shim: keeps the reference module layout importable on top of ebfi_amd."""
from .adversarial import Adversarial  # noqa: F401
from .discriminator import ST_Discriminator  # noqa: F401
from .flow import EventWarping, AveragedIWE  # noqa: F401
from .reconstruction import BrightnessConstancy  # noqa: F401
from .restore import CharbonnierLoss, perceptual_loss, psnr_loss, ssim_loss  # noqa: F401
from ebfi_amd.loss import Ternary, LaplacianLoss, LaplacianPyramid, GaussianConv  # noqa: F401
