"""Drop-in for the classes of `models.model_misc.submodules` the models use."""
from ebfi_amd.model import ConvLayer  # noqa: F401
from ebfi_amd.recurrent import (ConvGRU, ConvLSTM, RecurrentConvLayer, ResidualBlock, TransposedConvLayer,  # noqa: F401
                                UpsampleConvLayer)
