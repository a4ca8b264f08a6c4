"""The recurrent U-Nets of the reference's models/model_misc/unet.py on the device: UNetFlow ({'image', 'flow'}), UNetRecurrent
(the E2VID-style reconstruction net) and SRUNetRecurrent (its x2 variant), over BaseUNet / BaseUNet_legacy.  Each takes the
reference's `unet_kwargs` dict, keeps the reference's state-dict keys and carries its recurrent state in `self.states` from call
to call (set `net.states = [None] * net.num_encoders` to reset).

Where the work runs: head, encoders, residual blocks, decoders and the prediction layer are ConvLayer / ebfi_amd.recurrent
modules -- at kernel_size in {3, 5} (5 is the reference's default), norm=None and use_upsample_conv=True every convolution is a
csrc/conv2d.hip kernel, forward and both gradients, and the cells and the up-sampling are csrc/recurrent.hip.  The 5x5 layers
(head, stride-2 encoders, decoders, SRUNetRecurrent's skip up-samplers) run exact fp32 in every compute mode (ebfi_conv5x5_*);
their weight gradients are fixed-order slab reductions like the 3x3 ones, so a step stays bit-reproducible.  TransposedConvLayer
(use_upsample_conv=False) still goes to torch, reported through conv.left_native; with norm in {"BN", "IN"} the layers take
ConvLayer's non-fused route.  The skip additions, the skip concatenations, the crop or
pad in front of them and a final torch activation stay torch element-wise ops.  MultiResUNet is not here (it is not recurrent).
"""
import torch
import torch.nn as nn
import torch.nn.functional as F

from .model import ConvLayer
from .recurrent import RecurrentConvLayer, ResidualBlock, TransposedConvLayer, UpsampleConvLayer


def _fit(x1, x2):
    """x1 zero-padded to x2's size as ZeroPad2d does it; a negative pad crops (an odd size up-sampled is one pixel too large)."""
    dy, dx = x2.shape[2] - x1.shape[2], x2.shape[3] - x1.shape[3]
    return x1 if dy == 0 and dx == 0 else F.pad(x1, (dx // 2, dx - dx // 2, dy // 2, dy - dy // 2))


def skip_concat(x1, x2):
    return torch.cat([_fit(x1, x2), x2], dim=1)


def skip_sum(x1, x2):
    return _fit(x1, x2) + x2


_SKIP = {"sum": skip_sum, "concat": skip_concat}


class BaseUNet(nn.Module):
    """unet.py:19-111: the sizes and the builders shared by the nets below."""

    def __init__(self, base_num_channels, num_encoders, num_residual_blocks, num_output_channels, skip_type, norm,
                 use_upsample_conv, num_bins, recurrent_block_type=None, kernel_size=5, channel_multiplier=2):
        super().__init__()
        self.base_num_channels = base_num_channels
        self.num_encoders = num_encoders
        self.num_residual_blocks = num_residual_blocks
        self.num_output_channels = num_output_channels
        self.kernel_size = kernel_size
        self.skip_type = skip_type
        self.norm = norm
        self.num_bins = num_bins
        self.recurrent_block_type = recurrent_block_type
        self.channel_multiplier = channel_multiplier
        self.skip_ftn = _SKIP[skip_type]
        self.UpsampleLayer = UpsampleConvLayer if use_upsample_conv else TransposedConvLayer
        assert self.num_output_channels > 0
        self.encoder_input_sizes = [int(base_num_channels * pow(channel_multiplier, i)) for i in range(num_encoders)]
        self.encoder_output_sizes = [int(base_num_channels * pow(channel_multiplier, i + 1)) for i in range(num_encoders)]
        self.max_num_channels = self.encoder_output_sizes[-1]

    def _skip_width(self, channels):
        return channels if self.skip_type == "sum" else 2 * channels

    def build_head(self):
        return ConvLayer(self.num_bins, self.base_num_channels, kernel_size=self.kernel_size, stride=1, padding=self.kernel_size // 2)

    def build_recurrent_encoders(self):
        return nn.ModuleList(RecurrentConvLayer(i, o, kernel_size=self.kernel_size, stride=2, padding=self.kernel_size // 2,
                                                recurrent_block_type=self.recurrent_block_type, norm=self.norm)
                             for i, o in zip(self.encoder_input_sizes, self.encoder_output_sizes))

    def build_resblocks(self):
        return nn.ModuleList(ResidualBlock(self.max_num_channels, self.max_num_channels, norm=self.norm)
                             for _ in range(self.num_residual_blocks))

    def _upsampler(self, in_channels, out_channels, **extra):
        return self.UpsampleLayer(self._skip_width(in_channels), out_channels, kernel_size=self.kernel_size,
                                  padding=self.kernel_size // 2, norm=self.norm, **extra)

    def build_decoders(self):
        return nn.ModuleList(self._upsampler(i, o) for i, o in zip(reversed(self.encoder_output_sizes), reversed(self.encoder_input_sizes)))

    def build_prediction_layer(self, num_output_channels, norm=None):
        return ConvLayer(self._skip_width(self.base_num_channels), num_output_channels, 1, activation=None, norm=norm)

    def encode(self, x):
        """head, recurrent encoders (the states advance), residual blocks -> (x, head, the encoder outputs)."""
        x = head = self.head(x)
        blocks = []
        for i, encoder in enumerate(self.encoders):
            x, self.states[i] = encoder(x, self.states[i])
            blocks.append(x)
        for resblock in self.resblocks:
            x = resblock(x)
        return x, head, blocks


class BaseUNet_legacy(BaseUNet):
    """unet.py:114-167 (ECCV20): the same sizes and builders; build_resblocks assigns `self.resblocks` itself."""

    def build_resblocks(self):
        self.resblocks = BaseUNet.build_resblocks(self)


def _final_activation(unet_kwargs):
    kwargs = dict(unet_kwargs)
    return kwargs, getattr(torch, kwargs.pop("final_activation", "none"), None)


class UNetFlow(BaseUNet_legacy):
    """unet.py:170-227.  forward(x [N, num_bins, H, W]) -> {'image': [N, 1, H, W], 'flow': [N, 2, H, W]}."""

    def __init__(self, unet_kwargs):
        super().__init__(**dict(unet_kwargs, num_output_channels=3))
        self.head = self.build_head()
        self.encoders = self.build_recurrent_encoders()
        self.build_resblocks()
        self.decoders = self.build_decoders()
        self.pred = self.build_prediction_layer(num_output_channels=3)
        self.states = [None] * self.num_encoders

    def forward(self, x):
        x, head, blocks = self.encode(x)
        for i, decoder in enumerate(self.decoders):
            x = decoder(self.skip_ftn(x, blocks[self.num_encoders - i - 1]))
        img_flow = self.pred(self.skip_ftn(x, head))
        return {"image": img_flow[:, 0:1, :, :], "flow": img_flow[:, 1:3, :, :]}


class UNetRecurrent(BaseUNet):
    """unet.py:230-301.  forward(x) -> [N, 1, H, W]; `final_activation` names a torch function ('sigmoid') or 'none'."""

    def __init__(self, unet_kwargs):
        kwargs, self.final_activation = _final_activation(unet_kwargs)
        super().__init__(**dict(kwargs, num_output_channels=1))
        self.head = self.build_head()
        self.encoders = self.build_recurrent_encoders()
        self.resblocks = self.build_resblocks()
        self.decoders = self.build_decoders()
        self.pred = self.build_prediction_layer(self.num_output_channels, self.norm)
        self.states = [None] * self.num_encoders

    def forward(self, x):
        x, head, blocks = self.encode(x)
        for i, decoder in enumerate(self.decoders):
            x = decoder(self.skip_ftn(x, blocks[self.num_encoders - i - 1]))
        img = self.pred(self.skip_ftn(x, head))
        return img if self.final_activation is None else self.final_activation(img)


class SRUNetRecurrent(BaseUNet):
    """unet.py:393-498.  forward(x) -> [N, num_output_channels, 2H, 2W]: the first decoder up-samples by 4, and every skip
    (the encoder outputs and the head) passes through an up-sampling layer of its own."""

    def __init__(self, unet_kwargs):
        kwargs, self.final_activation = _final_activation(unet_kwargs)
        super().__init__(**kwargs)
        self.head = self.build_head()
        self.encoders = self.build_recurrent_encoders()
        self.resblocks = self.build_resblocks()
        self.decoders = self.build_SRdecoders()
        self.skip_upsampler = self.build_skip_upsampler()
        self.pred = self.build_prediction_layer(self.num_output_channels, self.norm)
        self.states = [None] * self.num_encoders

    def build_SRdecoders(self):
        sizes = zip(reversed(self.encoder_output_sizes), reversed(self.encoder_input_sizes))
        return nn.ModuleList(self._upsampler(i, o, scale=4 if k == 0 else 2) for k, (i, o) in enumerate(sizes))

    def build_skip_upsampler(self):
        return nn.ModuleList(self._upsampler(c, c, scale=2) for c in self.encoder_output_sizes[::-1] + [self.base_num_channels])

    def forward(self, x):
        x, head, blocks = self.encode(x)
        for i, decoder in enumerate(self.decoders):
            x = decoder(self.skip_ftn(x, self.skip_upsampler[i](blocks[self.num_encoders - i - 1])))
        img = self.pred(self.skip_ftn(x, self.skip_upsampler[-1](head)))
        return img if self.final_activation is None else self.final_activation(img)
