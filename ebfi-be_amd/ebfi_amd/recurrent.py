"""The recurrent building blocks of the reference's models/model_misc/submodules.py on the device: ConvLSTM, ConvGRU,
RecurrentConvLayer, ResidualBlock, UpsampleConvLayer and TransposedConvLayer, with the reference's constructor signatures,
parameter names and state-dict keys.

Where the work runs.  Every convolution goes through ebfi_amd.conv (csrc/conv2d.hip: kernel sizes 1, 3, 5 and 7; the 5x5
layers of RecurrentConvLayer and UpsampleConvLayer at the reference's default kernel size run exact fp32); the cell tails between them and the
bilinear up-sampling are csrc/recurrent.hip, one launch each and one per backward:

  ConvLSTM   cat(x, h) -> Gates (native conv, no activation) -> ebfi_lstm_cell_forward.  Backward recomputes the sigmoids and
             tanh from the saved pre-activations and hands the gate convolution the gradient of its output.
  ConvGRU    cat(x, h) -> update_gate, reset_gate (two native convs: parameters and launches stay two) ->
             ebfi_gru_reset_forward writes cat(x, h * sigmoid(reset)) -> out_gate -> ebfi_gru_update_forward.
  UpsampleConvLayer   ebfi_bilinear_up_forward (scale 2 or 4, align_corners=False; the backward is a gather, no atomics), then
             ConvLayer's fused conv + activation.

On CPU tensors, for a dtype other than float32 and under autocast the modules evaluate the reference's expressions in torch (as
ConvLayer does); a CUDA float32 tensor always takes the kernels: a missing library is an error, not a fallback.
TransposedConvLayer keeps nn.ConvTranspose2d and is reported through conv.left_native like any shape outside the kernels.
"""
import torch
import torch.nn as nn
import torch.nn.functional as F
from torch.autograd import Function

from . import _native as N
from . import conv
from .model import ConvLayer


def _native_ok(*tensors):
    return all(t is None or (t.is_cuda and t.dtype == torch.float32) for t in tensors) and not torch.is_autocast_enabled()


def _c(t):
    return None if t is None else t.contiguous()


# ------------------------------------------------------------------------------------------------------------ cell kernels
class LSTMCellFunction(Function):
    """(gates [B, 4C, H, W] pre-activations, prev_cell or None) -> (hidden, cell)."""

    @staticmethod
    def forward(ctx, gates, prev_cell):
        gates, prev_cell = gates.contiguous(), _c(prev_cell)
        B, C4, H, W = gates.shape
        C = C4 // 4
        hidden = torch.empty((B, C, H, W), dtype=gates.dtype, device=gates.device)
        cell = torch.empty_like(hidden)
        with torch.cuda.device_of(gates):
            N.check(N.lib().ebfi_lstm_cell_forward(N.ptr(gates), N.ptr(prev_cell), N.ptr(hidden), N.ptr(cell), B, C, H * W,
                                                   N.stream_ptr(gates.device)), "ebfi_lstm_cell_forward")
        ctx.set_materialize_grads(False)
        ctx.save_for_backward(gates, prev_cell, cell)
        return hidden, cell

    @staticmethod
    def backward(ctx, grad_hidden, grad_cell):
        gates, prev_cell, cell = ctx.saved_tensors
        B, C, H, W = cell.shape
        grad_gates = torch.empty_like(gates)
        if grad_hidden is None and grad_cell is None:
            return grad_gates.zero_(), None
        grad_prev = torch.empty_like(cell) if prev_cell is not None and ctx.needs_input_grad[1] else None
        with torch.cuda.device_of(gates):
            N.check(N.lib().ebfi_lstm_cell_backward(N.ptr(gates), N.ptr(prev_cell), N.ptr(cell), N.ptr(_c(grad_hidden)),
                                                    N.ptr(_c(grad_cell)), N.ptr(grad_gates), N.ptr(grad_prev), B, C, H * W,
                                                    N.stream_ptr(gates.device)), "ebfi_lstm_cell_backward")
        return grad_gates, grad_prev


class GRUResetFunction(Function):
    """(reset_pre [B, C, H, W], x [B, Cx, H, W], h or None) -> cat(x, h * sigmoid(reset_pre))."""

    @staticmethod
    def forward(ctx, reset_pre, x, h):
        reset_pre, x, h = reset_pre.contiguous(), x.contiguous(), _c(h)
        B, C, H, W = reset_pre.shape
        Cx = x.shape[1]
        out = torch.empty((B, Cx + C, H, W), dtype=x.dtype, device=x.device)
        with torch.cuda.device_of(x):
            N.check(N.lib().ebfi_gru_reset_forward(N.ptr(reset_pre), N.ptr(x), N.ptr(h), N.ptr(out), B, Cx, C, H * W,
                                                   N.stream_ptr(x.device)), "ebfi_gru_reset_forward")
        ctx.save_for_backward(reset_pre, h)
        ctx.Cx = Cx
        return out

    @staticmethod
    def backward(ctx, grad_out):
        reset_pre, h = ctx.saved_tensors
        B, C, H, W = reset_pre.shape
        grad_out = grad_out.contiguous()
        grad_x = torch.empty((B, ctx.Cx, H, W), dtype=grad_out.dtype, device=grad_out.device) if ctx.needs_input_grad[1] else None
        grad_reset = torch.empty_like(reset_pre)
        grad_h = torch.empty_like(reset_pre) if h is not None and ctx.needs_input_grad[2] else None
        with torch.cuda.device_of(grad_out):
            N.check(N.lib().ebfi_gru_reset_backward(N.ptr(grad_out), N.ptr(reset_pre), N.ptr(h), N.ptr(None), N.ptr(grad_x),
                                                    N.ptr(grad_reset), N.ptr(grad_h), B, ctx.Cx, C, H * W,
                                                    N.stream_ptr(grad_out.device)), "ebfi_gru_reset_backward")
        return grad_reset, grad_x, grad_h


class GRUUpdateFunction(Function):
    """(update_pre, out_pre [B, C, H, W], h or None) -> h * (1 - sigmoid(update_pre)) + tanh(out_pre) * sigmoid(update_pre)."""

    @staticmethod
    def forward(ctx, update_pre, out_pre, h):
        update_pre, out_pre, h = update_pre.contiguous(), out_pre.contiguous(), _c(h)
        B, C, H, W = update_pre.shape
        new = torch.empty_like(update_pre)
        with torch.cuda.device_of(new):
            N.check(N.lib().ebfi_gru_update_forward(N.ptr(update_pre), N.ptr(out_pre), N.ptr(h), N.ptr(new), B, C, H * W,
                                                    N.stream_ptr(new.device)), "ebfi_gru_update_forward")
        ctx.save_for_backward(update_pre, out_pre, h)
        return new

    @staticmethod
    def backward(ctx, grad_new):
        update_pre, out_pre, h = ctx.saved_tensors
        B, C, H, W = update_pre.shape
        grad_new = grad_new.contiguous()
        grad_u, grad_o = torch.empty_like(update_pre), torch.empty_like(update_pre)
        grad_h = torch.empty_like(update_pre) if h is not None and ctx.needs_input_grad[2] else None
        with torch.cuda.device_of(grad_new):
            N.check(N.lib().ebfi_gru_update_backward(N.ptr(update_pre), N.ptr(out_pre), N.ptr(h), N.ptr(grad_new), N.ptr(grad_u),
                                                     N.ptr(grad_o), N.ptr(grad_h), B, C, H * W, N.stream_ptr(grad_new.device)),
                    "ebfi_gru_update_backward")
        return grad_u, grad_o, grad_h


class BilinearUpFunction(Function):
    @staticmethod
    def forward(ctx, x, scale):
        x = x.contiguous()
        B, C, H, W = x.shape
        out = torch.empty((B, C, scale * H, scale * W), dtype=x.dtype, device=x.device)
        with torch.cuda.device_of(x):
            N.check(N.lib().ebfi_bilinear_up_forward(N.ptr(x), N.ptr(out), B * C, H, W, scale, N.stream_ptr(x.device)),
                    "ebfi_bilinear_up_forward")
        ctx.geo = (B, C, H, W, scale)
        return out

    @staticmethod
    def backward(ctx, grad_out):
        B, C, H, W, scale = ctx.geo
        grad_out = grad_out.contiguous()
        grad_x = torch.empty((B, C, H, W), dtype=grad_out.dtype, device=grad_out.device)
        with torch.cuda.device_of(grad_out):
            N.check(N.lib().ebfi_bilinear_up_backward(N.ptr(grad_out), N.ptr(grad_x), B * C, H, W, scale,
                                                      N.stream_ptr(grad_out.device)), "ebfi_bilinear_up_backward")
        return grad_x, None


def bilinear_up(x, scale):
    """F.interpolate(x, scale_factor=scale, mode='bilinear', align_corners=False); scale 2 or 4 on the device kernel."""
    if _native_ok(x) and x.dim() == 4 and scale in (2, 4) and x.numel() > 0:
        return BilinearUpFunction.apply(x, int(scale))
    return F.interpolate(x, scale_factor=scale, mode="bilinear", align_corners=False)


def _gate_conv(x, c):
    """A gate convolution without activation whose consumer (a cell kernel) hands back the gradient of its output."""
    if conv.supported(x, c.weight, c.stride, c.padding, c.dilation, c.groups):
        return conv.conv_bias_act(x, c.weight, c.bias, c.stride[0], c.padding[0], conv.ACT_NONE, 0.0, grad_preact=True)
    conv.left_native(x, c.weight, c.stride, c.padding, c.dilation, c.groups)
    return c(x)


# ------------------------------------------------------------------------------------------------------------ the cells
class ConvLSTM(nn.Module):
    """submodules.py:460-519.  forward(input_, prev_state=None) -> (hidden, cell); prev_state = (hidden, cell)."""

    def __init__(self, input_size, hidden_size, kernel_size):
        super().__init__()
        self.input_size = input_size
        self.hidden_size = hidden_size
        self.zero_tensors = {}
        self.Gates = nn.Conv2d(input_size + hidden_size, 4 * hidden_size, kernel_size, padding=kernel_size // 2)

    def _zeros(self, x):
        size = (x.shape[0], self.hidden_size) + tuple(x.shape[2:])
        key = (size, x.dtype, x.device)
        if key not in self.zero_tensors:
            self.zero_tensors[key] = torch.zeros(size, dtype=x.dtype, device=x.device)
        return self.zero_tensors[key]

    def forward(self, input_, prev_state=None):
        prev_hidden, prev_cell = prev_state if prev_state is not None else (self._zeros(input_), None)
        stacked = torch.cat((input_, prev_hidden), 1)
        if _native_ok(input_, prev_hidden, prev_cell):
            return LSTMCellFunction.apply(_gate_conv(stacked, self.Gates), prev_cell)
        in_gate, remember_gate, out_gate, cell_gate = self.Gates(stacked).chunk(4, 1)
        in_gate, remember_gate, out_gate = torch.sigmoid(in_gate), torch.sigmoid(remember_gate), torch.sigmoid(out_gate)
        cell = in_gate * torch.tanh(cell_gate)
        if prev_cell is not None:
            cell = remember_gate * prev_cell + cell
        return out_gate * torch.tanh(cell), cell


class ConvGRU(nn.Module):
    """submodules.py:522-562.  forward(input_, prev_state) -> new state; orthogonal weights, zero biases."""

    def __init__(self, input_size, hidden_size, kernel_size):
        super().__init__()
        padding = kernel_size // 2
        self.input_size = input_size
        self.hidden_size = hidden_size
        self.reset_gate = nn.Conv2d(input_size + hidden_size, hidden_size, kernel_size, padding=padding)
        self.update_gate = nn.Conv2d(input_size + hidden_size, hidden_size, kernel_size, padding=padding)
        self.out_gate = nn.Conv2d(input_size + hidden_size, hidden_size, kernel_size, padding=padding)
        for gate in (self.reset_gate, self.update_gate, self.out_gate):
            nn.init.orthogonal_(gate.weight)
            nn.init.constant_(gate.bias, 0.0)

    def forward(self, input_, prev_state):
        h = prev_state
        zeros = None
        if h is None:
            zeros = torch.zeros((input_.shape[0], self.hidden_size) + tuple(input_.shape[2:]), dtype=input_.dtype, device=input_.device)
        stacked = torch.cat([input_, zeros if h is None else h], dim=1)
        if _native_ok(input_, h):
            update_pre = _gate_conv(stacked, self.update_gate)
            reset_pre = _gate_conv(stacked, self.reset_gate)
            out_pre = _gate_conv(GRUResetFunction.apply(reset_pre, input_, h), self.out_gate)
            return GRUUpdateFunction.apply(update_pre, out_pre, h)
        h = zeros if h is None else h
        update = torch.sigmoid(self.update_gate(stacked))
        reset = torch.sigmoid(self.reset_gate(stacked))
        out_inputs = torch.tanh(self.out_gate(torch.cat([input_, h * reset], dim=1)))
        return h * (1 - update) + out_inputs * update


# ------------------------------------------------------------------------------------------------------------ the layers
class RecurrentConvLayer(nn.Module):
    """submodules.py:347-389: ConvLayer, then a ConvLSTM or ConvGRU of kernel size 3.  forward(x, prev_state) -> (x, state)."""

    def __init__(self, in_channels, out_channels, kernel_size=3, stride=1, padding=0, recurrent_block_type="convlstm",
                 activation="ReLU", norm=None, BN_momentum=0.1):
        super().__init__()
        assert recurrent_block_type in ["convlstm", "convgru"]
        self.recurrent_block_type = recurrent_block_type
        block = ConvLSTM if recurrent_block_type == "convlstm" else ConvGRU
        self.conv = ConvLayer(in_channels, out_channels, kernel_size, stride, padding, activation, norm, BN_momentum=BN_momentum)
        self.recurrent_block = block(input_size=out_channels, hidden_size=out_channels, kernel_size=3)

    def forward(self, x, prev_state):
        state = self.recurrent_block(self.conv(x), prev_state)
        return (state[0] if self.recurrent_block_type == "convlstm" else state), state


class ResidualBlock(nn.Module):
    """submodules.py:392-457.  Without a norm both convolutions are native (the first with its ReLU fused)."""

    def __init__(self, in_channels, out_channels, stride=1, downsample=None, norm=None, BN_momentum=0.1, activation="ReLU",
                 final_activation=True):
        super().__init__()
        self.final_activation = final_activation
        bias = norm != "BN"
        self.conv1 = nn.Conv2d(in_channels, out_channels, kernel_size=3, stride=stride, padding=1, bias=bias)
        self.norm = norm
        if norm == "BN":
            self.bn1 = nn.BatchNorm2d(out_channels, momentum=BN_momentum)
            self.bn2 = nn.BatchNorm2d(out_channels, momentum=BN_momentum)
        elif norm == "IN":
            self.bn1 = nn.InstanceNorm2d(out_channels)
            self.bn2 = nn.InstanceNorm2d(out_channels)
        self.activation = getattr(nn, activation)()
        self.conv2 = nn.Conv2d(out_channels, out_channels, kernel_size=3, stride=1, padding=1, bias=bias)
        self.downsample = downsample

    def _conv(self, x, c, act):
        """conv (+ the activation when `act` and it can be fused) -> (output, whether the activation is still to be applied)."""
        if _native_ok(x) and conv.supported(x, c.weight, c.stride, c.padding, c.dilation, c.groups):
            fuse = conv.activation_code(self.activation) if act else None
            code, slope = fuse if fuse is not None else (conv.ACT_NONE, 0.0)
            return conv.conv_bias_act(x, c.weight, c.bias, c.stride[0], c.padding[0], code, slope), act and fuse is None
        conv.left_native(x, c.weight, c.stride, c.padding, c.dilation, c.groups)
        return c(x), act

    def forward(self, x):
        normed = self.norm in ("BN", "IN")
        out, pending = self._conv(x, self.conv1, act=not normed)
        if normed:
            out, pending = self.bn1(out), True
        if pending:
            out = self.activation(out)
        out, _ = self._conv(out, self.conv2, act=False)
        if normed:
            out = self.bn2(out)
        out = out + (self.downsample(x) if self.downsample else x)
        return self.activation(out) if self.final_activation else out


class UpsampleConvLayer(ConvLayer):
    """submodules.py:298-344: bilinear up-sampling (align_corners=False) by `scale`, then conv (+ norm) (+ activation): the
    parameter container and its keys are ConvLayer's (`conv2d`, `norm_layer`)."""

    def __init__(self, in_channels, out_channels, kernel_size, stride=1, padding=0, activation="ReLU", norm=None, scale=2):
        super().__init__(in_channels, out_channels, kernel_size, stride, padding, activation, norm)
        self.scale = scale

    def forward(self, x):
        return super().forward(bilinear_up(x, self.scale))


class TransposedConvLayer(nn.Module):
    """submodules.py:247-295: ConvTranspose2d x2 (+ norm) (+ activation).  No native kernel: it runs on torch and says so."""

    def __init__(self, in_channels, out_channels, kernel_size, padding=0, activation="relu", norm=None):
        super().__init__()
        self.transposed_conv2d = nn.ConvTranspose2d(in_channels, out_channels, kernel_size, stride=2, padding=padding,
                                                    output_padding=1, bias=(norm != "BN"))
        self.activation = getattr(torch, activation) if activation is not None else None
        self.norm = norm
        if norm == "BN":
            self.norm_layer = nn.BatchNorm2d(out_channels)
        elif norm == "IN":
            self.norm_layer = nn.InstanceNorm2d(out_channels, track_running_stats=True)

    def forward(self, x):
        c = self.transposed_conv2d
        conv.left_native(x, c.weight, c.stride, c.padding, c.dilation, c.groups)
        out = c(x)
        if self.norm in ("BN", "IN"):
            out = self.norm_layer(out)
        return out if self.activation is None else self.activation(out)
