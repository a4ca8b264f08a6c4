"""Training loss of the hot path (device side).

Reference: loss/restore.py:149-213 (LaplacianLoss: 5-level Laplacian pyramid, L1 *sum*, level
weight 2**i), :111-145 (Ternary census, 7x7), combined as in train_ours.py:258-268.  On the GPU the 5x5
blur and the whole census term run as kernel pairs of libebfi_hip.so (csrc/imgops.hip); CPU tensors (host-logic
tests) take the equivalent shifted-slice formulation below.
"""
import os

import torch
import torch.nn as nn
import torch.nn.functional as F

from . import _native as N


class _Gauss5(torch.autograd.Function):
    """5x5 binomial blur with reflect padding on the gfx950 kernel pair (csrc/imgops.hip)."""

    @staticmethod
    def forward(ctx, x, factor):
        x = x.contiguous()
        ctx.factor = float(factor)
        out = torch.empty_like(x)
        H, W = x.shape[-2:]
        with torch.cuda.device_of(x):
            rc = N.lib().ebfi_gauss5_forward(N.ptr(x), N.ptr(out), x.numel() // (H * W), H, W, ctx.factor,
                                             N.stream_ptr(x.device))
        N.check(rc, "ebfi_gauss5_forward")
        return out

    @staticmethod
    def backward(ctx, g):
        g = g.contiguous()
        gin = torch.empty_like(g)
        H, W = g.shape[-2:]
        with torch.cuda.device_of(g):
            rc = N.lib().ebfi_gauss5_backward(N.ptr(g), N.ptr(gin), g.numel() // (H * W), H, W, ctx.factor,
                                              N.stream_ptr(g.device))
        N.check(rc, "ebfi_gauss5_backward")
        return gin, None


class _Census(torch.autograd.Function):
    """Whole Ternary loss (transform of both images, distance, mask, mean) on the kernel pair of csrc/imgops.hip."""

    @staticmethod
    def forward(ctx, x, y):
        x, y = x.contiguous(), y.contiguous()
        B, C, H, W = x.shape
        lib = N.lib()
        partial = torch.empty(int(lib.ebfi_census_partials(B, H, W)), dtype=torch.float32, device=x.device)
        with torch.cuda.device_of(x):
            rc = lib.ebfi_census_forward(N.ptr(x), N.ptr(y), N.ptr(partial), B, C, H, W, N.stream_ptr(x.device))
        N.check(rc, "ebfi_census_forward")
        ctx.save_for_backward(x, y)
        return partial.sum() / float(B * H * W)

    @staticmethod
    def backward(ctx, g):
        x, y = ctx.saved_tensors
        B, C, H, W = x.shape
        g = g.contiguous().float().reshape(1)
        gx = torch.empty_like(x)
        with torch.cuda.device_of(x):
            rc = N.lib().ebfi_census_backward(N.ptr(x), N.ptr(y), N.ptr(g), N.ptr(gx), B, C, H, W, N.stream_ptr(x.device))
        N.check(rc, "ebfi_census_backward")
        return gx, None


class _CensusPair(torch.autograd.Function):
    """coef_a * census(a, target) + coef_b * census(b, target) (b may be None) on the two-prediction kernels of csrc/imgops.hip:
    the target's tile and its per-tap transform are formed once for both, and the fixed-order sum of the per-tile partials, the
    mean and the weighting are one small launch instead of torch reductions and 0-dim arithmetic."""

    @staticmethod
    def forward(ctx, a, b, target, coef_a, coef_b):
        a, target = a.contiguous(), target.contiguous()
        b = b.contiguous() if b is not None else None
        B, C, H, W = a.shape
        lib = N.lib()
        partial = torch.empty(2 * int(lib.ebfi_census_partials(B, H, W)), dtype=torch.float32, device=a.device)
        loss = torch.empty((), dtype=torch.float32, device=a.device)
        with torch.cuda.device_of(a):
            rc = lib.ebfi_census_pair_forward(N.ptr(a), N.ptr(b) if b is not None else None, N.ptr(target), float(coef_a),
                                              float(coef_b), N.ptr(partial), N.ptr(loss), B, C, H, W, N.stream_ptr(a.device))
        N.check(rc, "ebfi_census_pair_forward")
        ctx.save_for_backward(*((a, target) if b is None else (a, target, b)))
        ctx.coefs = (float(coef_a), float(coef_b))
        return loss

    @staticmethod
    def backward(ctx, g):
        a, target = ctx.saved_tensors[:2]
        b = ctx.saved_tensors[2] if len(ctx.saved_tensors) > 2 else None
        B, C, H, W = a.shape
        g = g.contiguous().float().reshape(1)
        ga = torch.empty_like(a)
        gb = torch.empty_like(b) if b is not None else None
        with torch.cuda.device_of(a):
            rc = N.lib().ebfi_census_pair_backward(N.ptr(a), N.ptr(b) if b is not None else None, N.ptr(target), ctx.coefs[0],
                                                   ctx.coefs[1], N.ptr(g), N.ptr(ga), N.ptr(gb) if b is not None else None,
                                                   B, C, H, W, N.stream_ptr(a.device))
        N.check(rc, "ebfi_census_pair_backward")
        return ga, gb, None, None, None


def census_pair(a, b, target, coef_a, coef_b):
    """coef_a * Ternary()(a, target) + coef_b * Ternary()(b, target) for fp32 device images (b None: the first term alone)."""
    N.require_gpu(a, target)
    if a.dim() != 4 or a.shape != target.shape or (b is not None and b.shape != a.shape) or min(a.shape[-2:]) <= 6:
        raise ValueError("census_pair takes [B, C, H, W] images of one shape with H, W > 6, got %s" % (tuple(a.shape),))
    if any(t is not None and t.dtype != torch.float32 for t in (a, b, target)) or target.requires_grad:
        raise ValueError("census_pair takes float32 images and a target that needs no gradient")
    return _CensusPair.apply(a, b, target, coef_a, coef_b)


class _LapLoss(torch.autograd.Function):
    """coef_a * Lap(a, target) + coef_b * Lap(b, target) (restore.py:166-213) as ONE pyramid of the difference planes
    [a - target ; b - target] on csrc/laploss.hip: the pyramid is linear, so lap_i(x) - lap_i(y) = lap_i(x - y)."""

    LEVELS = 5

    @staticmethod
    def usable(a, b, target):
        H, W = a.shape[-2:]
        m = 1 << (_LapLoss.LEVELS - 1)
        ok = lambda t: t.is_cuda and t.dtype == torch.float32 and t.shape == a.shape
        return a.dim() == 4 and ok(a) and ok(target) and (b is None or ok(b)) and H % m == 0 and W % m == 0 and \
            2 * H // m >= 3 and 2 * W // m >= 3 and not target.requires_grad

    @staticmethod
    def forward(ctx, a, b, target, coef_a, coef_b):
        a, target = a.contiguous(), target.contiguous()
        b = b.contiguous() if b is not None else None
        B, C, H, W = a.shape
        ppt, L = B * C, _LapLoss.LEVELS
        planes = ppt * (2 if b is not None else 1)
        lib = N.lib()
        ws = torch.empty(int(lib.ebfi_laploss_workspace_floats(planes, H, W, L)), dtype=torch.float32, device=a.device)
        partial = torch.empty(int(lib.ebfi_laploss_partials(planes, H, W, L)), dtype=torch.float32, device=a.device)
        with torch.cuda.device_of(a):
            rc = lib.ebfi_laploss_forward(N.ptr(a), N.ptr(b) if b is not None else None, N.ptr(target), float(coef_a),
                                          float(coef_b), N.ptr(ws), N.ptr(partial), ppt, H, W, L, N.stream_ptr(a.device))
        N.check(rc, "ebfi_laploss_forward")
        ctx.ws, ctx.shape, ctx.two = ws, (B, C, H, W), b is not None
        return partial.sum()

    @staticmethod
    def backward(ctx, g):
        if ctx.ws is None:
            raise RuntimeError("laploss: the workspace of this forward was already consumed by a backward pass")
        B, C, H, W = ctx.shape
        n = 2 if ctx.two else 1
        g = g.contiguous().float().reshape(1)
        out = torch.empty((n * B, C, H, W), dtype=torch.float32, device=g.device)
        with torch.cuda.device_of(out):
            rc = N.lib().ebfi_laploss_backward(N.ptr(g), N.ptr(ctx.ws), N.ptr(out), n * B * C, H, W, _LapLoss.LEVELS,
                                               N.stream_ptr(out.device))
        N.check(rc, "ebfi_laploss_backward")
        ctx.ws = None
        return out[:B], (out[B:] if ctx.two else None), None, None, None


class GaussianConv(nn.Module):
    """5x5 binomial blur with reflect padding (restore.py:149-163).  The kernel is separable
    ([1,4,6,4,1]/16 twice), so it is applied as shifted-slice sums: no library convolution involved."""

    def __init__(self):
        super().__init__()
        k1 = torch.tensor([1., 4., 6., 4., 1.])
        self.kernel = nn.Parameter((k1[:, None] * k1[None, :] / 256).repeat(3, 1, 1, 1), requires_grad=False)
        self.taps = (1.0 / 16, 4.0 / 16, 6.0 / 16, 4.0 / 16, 1.0 / 16)

    def forward(self, x, factor=1):
        H, W = x.shape[-2:]
        if x.is_cuda and x.dtype == torch.float32 and H >= 3 and W >= 3:
            return _Gauss5.apply(x, factor)
        p = F.pad(x, (2, 2, 2, 2), mode="reflect")     # CPU tensors (host-logic tests): shifted-slice sums
        h = sum(t * p[..., :, j:j + W] for j, t in enumerate(self.taps))
        v = sum(t * h[..., i:i + H, :] for i, t in enumerate(self.taps))
        return v * factor if factor != 1 else v


class LaplacianPyramid(nn.Module):
    def __init__(self, max_level=5):
        super().__init__()
        self.gaussian_conv = GaussianConv()
        self.max_level = max_level

    def expand(self, x):
        B, C, H, W = x.shape
        up = x.new_zeros(B, C, 2 * H, 2 * W)
        up[:, :, ::2, ::2] = x                      # zero insertion (restore.py:189-197)
        return self.gaussian_conv(up, factor=4)

    def forward(self, X):
        pyramid, cur = [], X
        for _ in range(self.max_level - 1):
            reduced = F.avg_pool2d(self.gaussian_conv(cur), 2)
            pyramid.append(cur - self.expand(reduced))
            cur = reduced
        pyramid.append(cur)
        return pyramid


class LaplacianLoss(nn.Module):
    def __init__(self):
        super().__init__()
        self.lap = LaplacianPyramid()

    def forward(self, x, y, y_pyramid=None):
        """y_pyramid: optional precomputed pyramid of the target (it is shared by both loss terms of a step)."""
        yp = y_pyramid if y_pyramid is not None else self.lap(y)
        return sum((2 ** i) * F.l1_loss(a, b, reduction="sum") for i, (a, b) in enumerate(zip(self.lap(x), yp)))


class Ternary(nn.Module):
    def __init__(self, patch_size=7):
        super().__init__()
        self.patch_size = patch_size
        n = patch_size * patch_size
        self.register_buffer("w", torch.eye(n).view(n, 1, patch_size, patch_size), persistent=False)

    def transform(self, t):
        g = t.mean(dim=1, keepdim=True)
        H, W = g.shape[-2:]
        k, r = self.patch_size, self.patch_size // 2
        gp = F.pad(g, (r, r, r, r))                  # zero padding, like conv2d(padding=r)
        patches = torch.cat([gp[..., i:i + H, j:j + W] for i in range(k) for j in range(k)], dim=1)
        d = patches - g
        return d / torch.sqrt(0.81 + d ** 2)

    def forward(self, x, y, y_transform=None):
        if x.is_cuda and x.dtype == torch.float32 and y.dtype == torch.float32 and self.patch_size == 7 and \
                not y.requires_grad and x.shape[-1] > 6 and x.shape[-2] > 6:
            return _Census.apply(x, y)
        ty = y_transform if y_transform is not None else self.transform(y).detach()
        diff = self.transform(x) - ty
        dist = (diff ** 2 / (0.1 + diff ** 2)).mean(dim=1, keepdim=True)
        p = self.patch_size // 2
        mask = torch.zeros_like(dist)
        mask[:, :, p:-p, p:-p] = 1
        return (dist * mask).mean()


class TrainLoss(nn.Module):
    """train_ours.py:258-268; the model returns (SharpPre, Sharp) = its (Sharp, Final)."""

    def __init__(self, detail_enabled=True):
        super().__init__()
        self.Lap, self.census, self.detail_enabled = LaplacianLoss(), Ternary(), detail_enabled

    def forward(self, sharp_pre, sharp, target, iteration=0, accu_step=1):
        c_sharp, c_pre = (0.1, 1.0) if iteration < 10e3 else (1.0, 0.1)
        if not self.detail_enabled:
            c_sharp, c_pre, sharp_pre = 1.0, 0.0, None
        if _LapLoss.usable(sharp, sharp_pre, target):
            # one difference pyramid for both Laplacian terms; the census kernels work on the images themselves
            total = _LapLoss.apply(sharp, sharp_pre, target, c_sharp, c_pre) + census_pair(sharp, sharp_pre, target, c_sharp, c_pre)
            return total / accu_step
        with torch.no_grad():     # the target side of both terms is the same: compute it once
            yp = self.Lap.lap(target)
            ty = None if target.is_cuda else self.census.transform(target)   # the GPU census kernel works on the images
        term = lambda p: self.Lap(p, target, yp) + self.census(p, target, ty)
        if sharp_pre is None:
            return term(sharp) / accu_step
        return (c_sharp * term(sharp) + c_pre * term(sharp_pre)) / accu_step


class PerceptualTerm:
    """weight * mean over the batch of LPIPS as a term of the training loss (the reference builds perceptual_loss beside
    Lap and census, train_ours.py:765, with the AlexNet trunk): `model` is any LPIPS model with `loss` -- an
    ebfi_amd.lpips.AlexLPIPSLoss, the reference's trunk, or a VggLPIPS -- whose weights are no parameters of the trained
    model and enter no checkpoint.  term(pred, target) -> 0-dim tensor with a graph into pred; images in [0, 1]."""

    def __init__(self, model, weight):
        if not hasattr(model, "loss"):
            raise NotImplementedError("PerceptualTerm needs an LPIPS model with a backward (ebfi_amd.lpips.VggLPIPS); %s is a "
                                      "score only" % type(model).__name__)
        if not float(weight) > 0:
            raise ValueError("PerceptualTerm: the weight must be positive, got %r (leave the term out instead)" % (weight,))
        self.model, self.weight = model, float(weight)

    def __call__(self, pred, target):
        return self.weight * self.model.loss(pred, target.detach(), normalize=True).mean()


# ------------------------------------------------------------------------------------------------ Charbonnier (validation)
_cb_workspaces = {}


def _cb_workspace(device, stream, shape):
    key = (device, stream, shape)
    ws = _cb_workspaces.get(key)
    if ws is None:
        nbytes = N.lib().ebfi_charbonnier_workspace(*shape)
        ws = torch.empty(max(nbytes // 8, 2), dtype=torch.float64, device=device)   # (float64: 16-byte aligned storage)
        _cb_workspaces[key] = ws
    return ws


def _cb_check(x, y, eps):
    N.require_gpu(x, y)
    if x.dim() != 4 or x.shape != y.shape:
        raise ValueError("Charbonnier loss takes two [N, C, H, W] tensors of one shape, got %s and %s"
                         % (tuple(x.shape), tuple(y.shape)))
    if x.dtype != torch.float32 or y.dtype != torch.float32:
        raise ValueError("Charbonnier loss takes float32 tensors, got %s / %s" % (x.dtype, y.dtype))
    if x.device != y.device:
        raise ValueError("x on %s, y on %s" % (x.device, y.device))
    if not eps > 0:
        raise ValueError("eps must be positive, got %r" % (eps,))
    # the kernels read rows through arbitrary strides but need unit column stride
    x = x if x.stride(3) == 1 or x.shape[3] == 1 else x.contiguous()
    y = y if y.stride(3) == 1 or y.shape[3] == 1 else y.contiguous()
    return x, y


def _cb_strides(t):
    return N.i64x4(tuple(t.stride())[:3] + (1,))


def _cb_forward(x, y, eps):
    n, c, h, w = (int(v) for v in x.shape)
    out = torch.empty(n, dtype=torch.float32, device=x.device)
    if n == 0 or c * h * w == 0:
        return out.zero_()
    with torch.cuda.device_of(x):
        stream = N.stream_ptr(x.device)
        ws = _cb_workspace(x.device, stream.value, (n, c, h, w))
        rc = N.lib().ebfi_charbonnier_forward(N.ptr(x), _cb_strides(x), N.ptr(y), _cb_strides(y), n, c, h, w, float(eps),
                                              N.ptr(ws), ws.numel() * 8, N.ptr(out), stream)
    N.check(rc, "ebfi_charbonnier_forward")
    return out


@torch.no_grad()
def charbonnier_per_sample(x, y, eps=1e-3):
    """[N] float32 device tensor: sum over C, H, W of sqrt((x - y)^2 + eps) per sample of an fp32 pair [N, C, H, W] (tensors or
    strided views with unit column stride).  No autograd; two launches on the current stream, nothing is copied back."""
    x, y = _cb_check(x, y, eps)
    return _cb_forward(x, y, eps)


class _Charbonnier(torch.autograd.Function):
    """sum(sqrt((x - y)^2 + eps)) on the kernel pair of csrc/charbonnier.hip."""

    @staticmethod
    def forward(ctx, x, y, eps):
        ctx.eps = float(eps)
        ctx.save_for_backward(x, y)
        return _cb_forward(x, y, eps).sum()

    @staticmethod
    def backward(ctx, g):
        x, y = ctx.saved_tensors
        n, c, h, w = (int(v) for v in x.shape)
        g = g.contiguous().float().reshape(1)
        gx = torch.empty((n, c, h, w), dtype=torch.float32, device=x.device)
        if gx.numel():
            with torch.cuda.device_of(x):
                rc = N.lib().ebfi_charbonnier_backward(N.ptr(x), _cb_strides(x), N.ptr(y), _cb_strides(y), n, c, h, w, ctx.eps,
                                                       N.ptr(g), N.ptr(gx), N.stream_ptr(x.device))
            N.check(rc, "ebfi_charbonnier_backward")
        return (gx if ctx.needs_input_grad[0] else None), (-gx if ctx.needs_input_grad[1] else None), None


class CharbonnierLoss(nn.Module):
    """Charbonnier loss with the reference's call contract (loss/restore.py:95-105): forward(x, y) -> 0-dim tensor,
    sum(sqrt((x - y)^2 + eps)) over ALL elements (a sum, not a mean; eps under the root).  Device tensors only."""

    def __init__(self, eps=1e-3):
        super().__init__()
        self.eps = eps

    def forward(self, x, y):
        x, y = _cb_check(x, y, self.eps)
        return _Charbonnier.apply(x, y, self.eps)


# ------------------------------------------------------------------------------------------------ duty head + MSE (stage 1)
_dh_workspaces = {}


def _dh_workspace(device, stream, shape):
    key = (device, stream, shape)
    ws = _dh_workspaces.get(key)
    if ws is None:
        nbytes = N.lib().ebfi_duty_head_workspace(*shape)
        ws = torch.empty(max(nbytes // 8, 2), dtype=torch.float64, device=device)   # (float64: 16-byte aligned storage)
        _dh_workspaces[key] = ws
    return ws


def _dh_check(ex, duty):
    N.require_gpu(ex, duty)
    if ex.dim() != 4 or ex.shape[1] != 1:
        raise ValueError("the duty head takes a [B, 1, H, W] map, got %s" % (tuple(ex.shape),))
    if ex.dtype != torch.float32:
        raise ValueError("the duty head takes a float32 map, got %s" % ex.dtype)
    if ex.shape[0] == 0 or ex.shape[2] * ex.shape[3] == 0:
        raise ValueError("the duty head needs a non-empty map, got %s" % (tuple(ex.shape),))
    if duty is not None:
        if duty.numel() != ex.shape[0] or duty.dtype != torch.float32 or duty.device != ex.device:
            raise ValueError("duty must be a float32 [B, 1] tensor on the map's device, got %s %s on %s for B = %d"
                             % (duty.dtype, tuple(duty.shape), duty.device, ex.shape[0]))
        duty = duty.detach().reshape(-1).contiguous()
    # rows are read through arbitrary strides, columns need unit stride
    return (ex if ex.stride(3) == 1 or ex.shape[3] == 1 else ex.contiguous()), duty


def _dh_forward(ex, duty, scale):
    b, _, h, w = (int(v) for v in ex.shape)
    Ex = torch.empty((b, 1), dtype=torch.float32, device=ex.device)
    loss = torch.empty((), dtype=torch.float32, device=ex.device) if duty is not None else None
    with torch.cuda.device_of(ex):
        stream = N.stream_ptr(ex.device)
        ws = _dh_workspace(ex.device, stream.value, (b, h, w))
        rc = N.lib().ebfi_duty_head_forward(N.ptr(ex), N.i64x4(tuple(ex.stride())[:3] + (1,)), N.ptr(duty), b, h, w, float(scale),
                                            N.ptr(ws), ws.numel() * 8, N.ptr(Ex), N.ptr(loss), stream)
    N.check(rc, "ebfi_duty_head_forward")
    return Ex, loss


@torch.no_grad()
def duty_head(ex):
    """Ex [B, 1] = sigmoid(mean over H, W) of an fp32 map [B, 1, H, W] (the tail of ExposureDecision.forward, reference
    model_singleframe.py:75-76) on the kernels of csrc/dutyhead.hip.  No autograd; two launches, nothing is copied back."""
    ex, _ = _dh_check(ex, None)
    return _dh_forward(ex, None, 1.0)[0]


class _DutyMSE(torch.autograd.Function):
    """(scale * MSELoss(sigmoid(mean(ex)), duty), Ex) on the kernels of csrc/dutyhead.hip; Ex is not differentiable."""

    @staticmethod
    def forward(ctx, ex, duty, scale):
        Ex, loss = _dh_forward(ex, duty, scale)
        ctx.scale, ctx.shape = float(scale), tuple(int(v) for v in ex.shape)
        ctx.save_for_backward(Ex, duty)
        ctx.mark_non_differentiable(Ex)
        return loss, Ex

    @staticmethod
    def backward(ctx, g, _g_ex):
        Ex, duty = ctx.saved_tensors
        b, _, h, w = ctx.shape
        g = g.contiguous().float().reshape(1)
        grad = torch.empty(ctx.shape, dtype=torch.float32, device=Ex.device)
        with torch.cuda.device_of(Ex):
            rc = N.lib().ebfi_duty_head_backward(N.ptr(g), N.ptr(Ex), N.ptr(duty), b, h, w, ctx.scale, N.ptr(grad),
                                                 N.stream_ptr(Ex.device))
        N.check(rc, "ebfi_duty_head_backward")
        return grad, None, None


class DutyMSELoss(nn.Module):
    """Stage-1 loss of the reference (train_ours_exposuredecision.py:250-252) from the map in front of ExposureDecision's pooling:
    forward(ex [B, 1, H, W], duty [B, 1]) -> MSELoss(sigmoid(AVGPool(ex)).view(-1, 1), duty) * scale, a 0-dim tensor; pass
    scale = 1 / accu_step.  `Ex` holds the [B, 1] exposure estimate of the last call (detached).  Device tensors only."""

    def __init__(self, scale=1.0):
        super().__init__()
        self.scale = float(scale)
        self.Ex = None

    def forward(self, ex, duty):
        ex, duty = _dh_check(ex, duty)
        if duty is None:
            raise ValueError("DutyMSELoss needs the ground-truth duty")
        loss, self.Ex = _DutyMSE.apply(ex, duty, self.scale)
        return loss
