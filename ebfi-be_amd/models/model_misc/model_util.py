"""Drop-in for the helpers of `models.model_misc.model_util` the models use."""
from ebfi_amd.model import CropSize, initialize_weights  # noqa: F401
from ebfi_amd.unet import skip_concat, skip_sum  # noqa: F401
