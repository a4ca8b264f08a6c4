"""Modulated deformable convolution v2 -- host side.

Mirrors the reference's ``models/DCNv2/dcn_v2.py``: the autograd op ``_DCNv2`` / ``dcn_v2_conv``
(:17-95, argument order ``(input, offset, mask, weight, bias, stride, padding, dilation,
deformable_groups)``), and the modules ``DCNv2`` (:98-146), ``DCN`` (:149-194) and ``DCN_sep``
(:197-227) with the same parameter names (``weight``, ``bias``, ``conv_offset_mask.*``), the same
initialisation and the same argument checks as the extension wrappers
(src/cuda/dcn_v2_cuda.cu:38-62,110-111).  Compute: ``ebfi_dcn_forward`` / ``ebfi_dcn_backward``.

Deformable PS-ROI pooling (:230-435) likewise: the autograd op ``_DCNv2Pooling`` / ``dcn_v2_pooling`` (argument order
``(input, rois, offset, spatial_scale, pooled_size, output_dim, no_trans, group_size, part_size, sample_per_part,
trans_std)``) and the modules ``DCNv2Pooling`` and ``DCNPooling`` (``offset_mask_fc.*``).  Compute:
``ebfi_dcn_pooling_forward`` / ``ebfi_dcn_pooling_backward``; the law and the two places where it is defined instead of
reading out of bounds (``C == output_dim * group_size**2``, ROIs with a batch index outside the batch) are in
include/ebfi_hip.h.

Not mirrored (out of scope): the ONNX wrapper.
"""
import logging
import math

import torch
from torch import nn
from torch.autograd import Function
from torch.autograd.function import once_differentiable
from torch.nn.modules.utils import _pair

from . import _native as N

logger = logging.getLogger("base")


def _geometry(input, weight, stride, padding, dilation, dg):
    B, C, H, W = input.shape
    Co, Cw, kh, kw = weight.shape
    if C != Cw:
        raise RuntimeError("Input shape and kernel channels wont match: (%d vs %d)." % (C, Cw))
    (sh, sw), (ph, pw), (dh, dw) = stride, padding, dilation
    return [int(v) for v in (B, C, H, W, Co, kh, kw, sh, sw, ph, pw, dh, dw, dg)]


def _out_hw(geo):
    B, C, H, W, Co, kh, kw, sh, sw, ph, pw, dh, dw, dg = geo
    return ((H + 2 * ph - (dh * (kh - 1) + 1)) // sh + 1, (W + 2 * pw - (dw * (kw - 1) + 1)) // sw + 1)


def _check_offset_mask(geo, offset, mask):
    B, C, H, W, Co, kh, kw, sh, sw, ph, pw, dh, dw, dg = geo
    Ho, Wo = _out_hw(geo)
    if tuple(offset.shape) != (B, dg * 2 * kh * kw, Ho, Wo):
        raise RuntimeError("offset must be %s, got %s" % ((B, dg * 2 * kh * kw, Ho, Wo), tuple(offset.shape)))
    if tuple(mask.shape) != (B, dg * kh * kw, Ho, Wo):
        raise RuntimeError("mask must be %s, got %s" % ((B, dg * kh * kw, Ho, Wo), tuple(mask.shape)))


PRODUCTS = ("fp32", "bf16x3")


def dcn_v2_forward(input, weight, bias, offset, mask, stride, padding, dilation, dg, product="fp32"):
    """`product`: matrix-core operands of the 64 x C*kh*kw x 64 product -- "fp32" (exact, the kernel the reference's
    known-answer tests pin; also the faster one) or "bf16x3" (split precision, ~1e-5).  It is an explicit
    argument of the op, never taken from ambient process state."""
    if product not in PRODUCTS:
        raise ValueError("product must be one of %s" % (PRODUCTS,))
    for name, t in (("input", input), ("weight", weight), ("bias", bias), ("offset", offset), ("mask", mask)):
        if not t.is_cuda:
            raise NotImplementedError("%s must be a GPU tensor: libebfi_hip.so has no CPU path" % name)
    geo = _geometry(input, weight, stride, padding, dilation, dg)
    _check_offset_mask(geo, offset, mask)
    # the reference reads these through raw data pointers (no contiguity check); be explicit instead
    input, weight, bias = input.contiguous(), weight.contiguous(), bias.contiguous()
    offset, mask = offset.contiguous(), mask.contiguous()
    Ho, Wo = _out_hw(geo)
    out = torch.empty((geo[0], geo[4], Ho, Wo), dtype=input.dtype, device=input.device)
    code = N.dtype_code(input)
    if code == N.EBFI_F32 and product == "bf16x3":
        code = N.EBFI_F32_BF16X3MMA
    with torch.cuda.device_of(input):
        rc = N.lib().ebfi_dcn_forward(N.ptr(input), N.ptr(weight), N.ptr(bias), N.ptr(offset), N.ptr(mask),
                                      N.ptr(out), *geo, code, N.stream_ptr(input.device))
    N.check(rc, "ebfi_dcn_forward")
    return out


def dcn_v2_backward(input, weight, bias, offset, mask, grad_output, stride, padding, dilation, dg):
    if not input.is_contiguous():
        raise RuntimeError("input tensor has to be contiguous")
    if not weight.is_contiguous():
        raise RuntimeError("weight tensor has to be contiguous")
    for name, t in (("input", input), ("weight", weight), ("bias", bias), ("offset", offset), ("mask", mask),
                    ("grad_output", grad_output)):
        if not t.is_cuda:
            raise NotImplementedError("%s must be a GPU tensor: libebfi_hip.so has no CPU path" % name)
    geo = _geometry(input, weight, stride, padding, dilation, dg)
    _check_offset_mask(geo, offset, mask)
    offset, mask, grad_output = offset.contiguous(), mask.contiguous(), grad_output.contiguous()
    gx, gw, gb = torch.empty_like(input), torch.empty_like(weight), torch.empty_like(bias)
    go, gm = torch.empty_like(offset), torch.empty_like(mask)
    lib = N.lib()
    need = lib.ebfi_dcn_backward_workspace(*geo, N.dtype_code(input))
    ws = torch.empty(max(int(need), 4), dtype=torch.uint8, device=input.device)
    with torch.cuda.device_of(input):
        rc = lib.ebfi_dcn_backward(N.ptr(input), N.ptr(weight), N.ptr(bias), N.ptr(offset), N.ptr(mask),
                                   N.ptr(grad_output), N.ptr(gx), N.ptr(go), N.ptr(gm), N.ptr(gw), N.ptr(gb),
                                   *geo, N.ptr(ws), int(need), N.dtype_code(input), N.stream_ptr(input.device))
    N.check(rc, "ebfi_dcn_backward")
    return gx, go, gm, gw, gb


class _DCNv2(Function):
    @staticmethod
    def forward(ctx, input, offset, mask, weight, bias, stride, padding, dilation, deformable_groups):
        ctx.stride, ctx.padding, ctx.dilation = _pair(stride), _pair(padding), _pair(dilation)
        ctx.kernel_size = _pair(weight.shape[2:4])
        ctx.deformable_groups = deformable_groups
        output = dcn_v2_forward(input, weight, bias, offset, mask, ctx.stride, ctx.padding, ctx.dilation,
                                deformable_groups)
        ctx.save_for_backward(input, offset, mask, weight, bias)
        return output

    @staticmethod
    @once_differentiable
    def backward(ctx, grad_output):
        input, offset, mask, weight, bias = ctx.saved_tensors
        gx, go, gm, gw, gb = dcn_v2_backward(input, weight, bias, offset, mask, grad_output, ctx.stride,
                                             ctx.padding, ctx.dilation, ctx.deformable_groups)
        return gx, go, gm, gw, gb, None, None, None, None


dcn_v2_conv = _DCNv2.apply


class DCNv2(nn.Module):
    def __init__(self, in_channels, out_channels, kernel_size, stride, padding, dilation=1, deformable_groups=1):
        super().__init__()
        self.in_channels, self.out_channels = in_channels, out_channels
        self.kernel_size, self.stride = _pair(kernel_size), _pair(stride)
        self.padding, self.dilation = _pair(padding), _pair(dilation)
        self.deformable_groups = deformable_groups
        self.weight = nn.Parameter(torch.empty(out_channels, in_channels, *self.kernel_size))
        self.bias = nn.Parameter(torch.empty(out_channels))
        self.reset_parameters()

    def reset_parameters(self):
        fan = self.in_channels * self.kernel_size[0] * self.kernel_size[1]
        bound = 1.0 / math.sqrt(fan)
        self.weight.data.uniform_(-bound, bound)
        self.bias.data.zero_()

    def _taps(self):
        return self.deformable_groups * self.kernel_size[0] * self.kernel_size[1]

    def _apply_op(self, input, offset, mask):
        return dcn_v2_conv(input, offset, mask, self.weight, self.bias, self.stride, self.padding, self.dilation,
                           self.deformable_groups)

    def forward(self, input, offset, mask):
        assert 2 * self._taps() == offset.shape[1]
        assert self._taps() == mask.shape[1]
        return self._apply_op(input, offset, mask)


class _SelfOffsetMixin:
    """conv_offset_mask: zero-initialised conv producing 3*dg*kh*kw channels, split in thirds as
    (o1, o2, mask); offset = cat(o1, o2), mask = sigmoid(mask)  (dcn_v2.py:165-182)."""

    def _make_offset_conv(self):
        self.conv_offset_mask = nn.Conv2d(self.in_channels, 3 * self._taps(), kernel_size=self.kernel_size,
                                          stride=self.stride, padding=self.padding, bias=True)
        self.init_offset()

    def init_offset(self):
        self.conv_offset_mask.weight.data.zero_()
        self.conv_offset_mask.bias.data.zero_()

    def _offset_mask(self, feat):
        o1, o2, mask = torch.chunk(self.conv_offset_mask(feat), 3, dim=1)
        return torch.cat((o1, o2), dim=1), torch.sigmoid(mask)


class DCN(DCNv2, _SelfOffsetMixin):
    def __init__(self, in_channels, out_channels, kernel_size, stride, padding, dilation=1, deformable_groups=1):
        super().__init__(in_channels, out_channels, kernel_size, stride, padding, dilation, deformable_groups)
        self._make_offset_conv()

    def forward(self, input):
        offset, mask = self._offset_mask(input)
        return self._apply_op(input, offset, mask)


class DCN_sep(DCNv2, _SelfOffsetMixin):
    """Offsets and masks come from a second feature map (dcn_v2.py:197-227)."""

    def __init__(self, in_channels, out_channels, kernel_size, stride, padding, dilation=1, deformable_groups=1):
        super().__init__(in_channels, out_channels, kernel_size, stride, padding, dilation, deformable_groups)
        self._make_offset_conv()

    def forward(self, input, fea):
        offset, mask = self._offset_mask(fea)
        offset_mean = torch.mean(torch.abs(offset))
        # the reference's magnitude warning is a host sync (:221-223): skipped while a hipGraph is being captured
        if not (offset.is_cuda and torch.cuda.is_current_stream_capturing()) and offset_mean > 100:
            logger.warning("Offset mean is {}, larger than 100.".format(offset_mean))
        return self._apply_op(input, offset, mask)


# ------------------------------------------------------------------ deformable PS-ROI pooling
def _pool_geometry(input, rois, trans, no_trans, output_dim, group_size, pooled_size, part_size, sample_per_part):
    """Shape checks of both pooling passes; returns (B, C, H, W, R, nc)."""
    if input.dim() != 4:
        raise RuntimeError("input must be [B, C, H, W], got %s" % (tuple(input.shape),))
    if rois.dim() != 2 or rois.shape[1] != 5:
        raise RuntimeError("rois must be [R, 5] (batch index, x1, y1, x2, y2), got %s" % (tuple(rois.shape),))
    B, C, H, W = (int(v) for v in input.shape)
    R = int(rois.shape[0])
    D, G, P, part, spp = int(output_dim), int(group_size), int(pooled_size), int(part_size), int(sample_per_part)
    if min(B, C, H, W, D, G, P, part, spp) < 1:
        raise RuntimeError("sizes must be >= 1: input %s, output_dim %d, group_size %d, pooled_size %d, part_size %d, "
                           "sample_per_part %d" % (tuple(input.shape), D, G, P, part, spp))
    if C != D * G * G:
        raise RuntimeError("input channels must equal output_dim * group_size**2: %d vs %d * %d**2" % (C, D, G))
    if no_trans:
        nc = 1
    else:
        if trans.dim() != 4 or trans.shape[1] % 2 or trans.shape[1] < 2 or tuple(trans.shape[2:]) != (part, part):
            raise RuntimeError("offset must be [>= %d, 2 * classes, %d, %d], got %s" % (R, part, part, tuple(trans.shape)))
        if trans.shape[0] < R:
            raise RuntimeError("offset has %d rows for %d rois" % (trans.shape[0], R))
        nc = int(trans.shape[1]) // 2
        if D % nc:
            raise RuntimeError("output_dim %d is not a multiple of the %d classes of offset" % (D, nc))
    return B, C, H, W, R, nc


def _pool_require_gpu(**tensors):
    for name, t in tensors.items():
        if not t.is_cuda:
            raise NotImplementedError("%s must be a GPU tensor: libebfi_hip.so has no CPU path" % name)


def dcn_v2_pooling_forward(input, rois, trans, no_trans, spatial_scale, output_dim, group_size, pooled_size, part_size,
                           sample_per_part, trans_std):
    """(output, count), both [R, output_dim, pooled_size, pooled_size]; `trans` may be the empty tensor when no_trans."""
    no_trans = bool(no_trans)
    if no_trans:
        _pool_require_gpu(input=input, rois=rois)
    else:
        _pool_require_gpu(input=input, rois=rois, offset=trans)
    B, C, H, W, R, nc = _pool_geometry(input, rois, trans, no_trans, output_dim, group_size, pooled_size, part_size,
                                       sample_per_part)
    # the reference reads these through raw data pointers after .contiguous(); be explicit too
    input, rois = input.contiguous(), rois.contiguous()
    trans = None if no_trans else trans.contiguous()
    out = torch.empty((R, int(output_dim), int(pooled_size), int(pooled_size)), dtype=input.dtype, device=input.device)
    count = torch.empty_like(out)
    code = N.dtype_code(input)
    with torch.cuda.device_of(input):
        rc = N.lib().ebfi_dcn_pooling_forward(N.ptr(input), N.ptr(rois), N.ptr(trans), N.ptr(out), N.ptr(count),
                                              B, C, H, W, R, nc, int(no_trans), float(spatial_scale), int(output_dim),
                                              int(group_size), int(pooled_size), int(part_size), int(sample_per_part),
                                              float(trans_std), code, N.stream_ptr(input.device))
    N.check(rc, "ebfi_dcn_pooling_forward")
    return out, count


def dcn_v2_pooling_backward(grad_output, input, rois, trans, count, no_trans, spatial_scale, output_dim, group_size,
                            pooled_size, part_size, sample_per_part, trans_std):
    """(grad_input, grad_trans); grad_trans has the shape of `trans` (rows past the rois, and all of it when no_trans, 0)."""
    no_trans = bool(no_trans)
    if no_trans:
        _pool_require_gpu(grad_output=grad_output, input=input, rois=rois, count=count)
    else:
        _pool_require_gpu(grad_output=grad_output, input=input, rois=rois, offset=trans, count=count)
    B, C, H, W, R, nc = _pool_geometry(input, rois, trans, no_trans, output_dim, group_size, pooled_size, part_size,
                                       sample_per_part)
    oshape = (R, int(output_dim), int(pooled_size), int(pooled_size))
    if tuple(grad_output.shape) != oshape or tuple(count.shape) != oshape:
        raise RuntimeError("grad_output and count must be %s, got %s and %s" % (oshape, tuple(grad_output.shape),
                                                                                tuple(count.shape)))
    input, rois = input.contiguous(), rois.contiguous()
    grad_output, count = grad_output.contiguous(), count.contiguous()
    if R == 0:     # (the entry point writes nothing for an empty call)
        return torch.zeros_like(input), (input.new_zeros(0) if no_trans else torch.zeros_like(trans))
    gx = torch.empty_like(input)
    if no_trans:
        trans, gt, Rt = None, None, R
    else:
        trans = trans.contiguous()
        gt, Rt = torch.empty_like(trans), int(trans.shape[0])
    code = N.dtype_code(input)
    with torch.cuda.device_of(input):
        rc = N.lib().ebfi_dcn_pooling_backward(N.ptr(grad_output), N.ptr(input), N.ptr(rois), N.ptr(trans), N.ptr(count),
                                               N.ptr(gx), N.ptr(gt), Rt, B, C, H, W, R, nc, int(no_trans),
                                               float(spatial_scale), int(output_dim), int(group_size), int(pooled_size),
                                               int(part_size), int(sample_per_part), float(trans_std), code,
                                               N.stream_ptr(input.device))
    N.check(rc, "ebfi_dcn_pooling_backward")
    return gx, (gt if gt is not None else input.new_zeros(0))


class _DCNv2Pooling(Function):
    @staticmethod
    def forward(ctx, input, rois, offset, spatial_scale, pooled_size, output_dim, no_trans, group_size=1, part_size=None,
                sample_per_part=4, trans_std=0.0):
        ctx.spatial_scale = spatial_scale
        ctx.no_trans = int(no_trans)
        ctx.output_dim = output_dim
        ctx.group_size = group_size
        ctx.pooled_size = pooled_size
        ctx.part_size = pooled_size if part_size is None else part_size
        ctx.sample_per_part = sample_per_part
        ctx.trans_std = trans_std
        output, output_count = dcn_v2_pooling_forward(input, rois, offset, ctx.no_trans, ctx.spatial_scale, ctx.output_dim,
                                                      ctx.group_size, ctx.pooled_size, ctx.part_size, ctx.sample_per_part,
                                                      ctx.trans_std)
        ctx.save_for_backward(input, rois, offset, output_count)
        return output

    @staticmethod
    @once_differentiable
    def backward(ctx, grad_output):
        input, rois, offset, output_count = ctx.saved_tensors
        grad_input, grad_offset = dcn_v2_pooling_backward(grad_output, input, rois, offset, output_count, ctx.no_trans,
                                                          ctx.spatial_scale, ctx.output_dim, ctx.group_size,
                                                          ctx.pooled_size, ctx.part_size, ctx.sample_per_part, ctx.trans_std)
        if ctx.no_trans:
            grad_offset = None
        return grad_input, None, grad_offset, None, None, None, None, None, None, None, None


dcn_v2_pooling = _DCNv2Pooling.apply


class DCNv2Pooling(nn.Module):
    def __init__(self, spatial_scale, pooled_size, output_dim, no_trans, group_size=1, part_size=None, sample_per_part=4,
                 trans_std=0.0):
        super().__init__()
        self.spatial_scale = spatial_scale
        self.pooled_size = pooled_size
        self.output_dim = output_dim
        self.no_trans = no_trans
        self.group_size = group_size
        self.part_size = pooled_size if part_size is None else part_size
        self.sample_per_part = sample_per_part
        self.trans_std = trans_std

    def _pool(self, input, rois, offset, no_trans):
        return dcn_v2_pooling(input, rois, offset, self.spatial_scale, self.pooled_size, self.output_dim, no_trans,
                              self.group_size, self.part_size, self.sample_per_part, self.trans_std)

    def forward(self, input, rois, offset):
        # (the reference asserts C == output_dim and then indexes (d * G + gh) * G + gw: in bounds for group_size 1 only)
        assert input.shape[1] == self.output_dim * self.group_size ** 2
        if self.no_trans:
            offset = input.new()
        return self._pool(input, rois, offset, self.no_trans)


class DCNPooling(DCNv2Pooling):
    """Offsets and a mask from the ROI-aligned features themselves (dcn_v2.py:338-435): pool without offsets, run
    offset_mask_fc (last layer zero-initialised), pool again with the offsets and multiply by sigmoid(mask)."""

    def __init__(self, spatial_scale, pooled_size, output_dim, no_trans, group_size=1, part_size=None, sample_per_part=4,
                 trans_std=0.0, deform_fc_dim=1024):
        super().__init__(spatial_scale, pooled_size, output_dim, no_trans, group_size, part_size, sample_per_part, trans_std)
        self.deform_fc_dim = deform_fc_dim
        if not no_trans:
            self.offset_mask_fc = nn.Sequential(
                nn.Linear(self.pooled_size * self.pooled_size * self.output_dim, self.deform_fc_dim),
                nn.ReLU(inplace=True),
                nn.Linear(self.deform_fc_dim, self.deform_fc_dim),
                nn.ReLU(inplace=True),
                nn.Linear(self.deform_fc_dim, self.pooled_size * self.pooled_size * 3))
            self.offset_mask_fc[4].weight.data.zero_()
            self.offset_mask_fc[4].bias.data.zero_()

    def forward(self, input, rois):
        assert input.shape[1] == self.output_dim * self.group_size ** 2
        offset = input.new()
        if self.no_trans:
            return self._pool(input, rois, offset, self.no_trans)      # only roi_align
        n = rois.shape[0]
        roi = self._pool(input, rois, offset, True)
        offset_mask = self.offset_mask_fc(roi.view(n, -1)).view(n, 3, self.pooled_size, self.pooled_size)
        o1, o2, mask = torch.chunk(offset_mask, 3, dim=1)
        offset = torch.cat((o1, o2), dim=1)
        return self._pool(input, rois, offset, self.no_trans) * torch.sigmoid(mask)
