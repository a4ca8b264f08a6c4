"""loss/reconstruction.py and myutils/gradients.py on the device (csrc/bcloss.hip): ``Sobel`` and ``BrightnessConstancy``
(Paredes-Valles et al., CVPR'21, section 3.4) with the reference's constructor, attributes and method signatures --
``generative_model``, ``temporal_consistency`` and ``regularization``, each one device scalar with its gradients.

The law is what the reference's code does.  ``flow`` is ``[B, 2, H, W]`` (channel 0 horizontal, channel 1 vertical) in units
of ``S = max(H, W)``; the reference normalises ``g = 2 * (p - f * S) / (n - 1) - 1`` and calls ``grid_sample`` without
``align_corners``, so the sampled coordinate is ``((g + 1) * n - 1) / 2`` -- not ``p - f * S`` --, bilinear, zero padding.
``generative_model`` masks the flow by ``inputs["inp_cnt"]`` (1 where the channel sum is positive, the sum itself elsewhere),
samples the Sobel images of ``img``, and returns ``sum(((A[:, 0:1] - A[:, 1:2]) + (Sx * fx + Sy * fy) * S) ** 2)`` with ``A`` the
``AveragedIWE`` of the masked flow, which carries no gradient.  ``|.|`` has subgradient 0 at 0.

The gradient of ``grid_sample`` into the sampled image is a scatter; eager PyTorch on a GPU runs it with float atomics, whose
order changes from run to run.  Here every destination pixel adds its float32 addends in ascending source-pixel index, then
corner order (a stable integer sort and one owner per pixel), the per-pixel arithmetic is float64 of the float32 inputs, and
the sums are float64 in a fixed order: two calls give the same bits, and every call can be captured in a graph -- nothing
synchronises, allocates inside the library or reads a value back.

Defined here where the reference is not: ``H < 2`` or ``W < 2`` is refused (the reference divides by ``n - 1``); an image with
``C != 1`` is refused in ``generative_model`` and ``temporal_consistency`` (the reference's own shapes then disagree); a
non-finite sample coordinate samples 0 and passes no gradient to the image or the grid.  float32 GPU tensors only; float64,
CPU tensors, mixed devices and ``B * H * W >= 2**32 - 1`` are refused; the two sampling terms, whose backward sorts four
32-bit entries per pixel, also refuse ``4 * B * H * W >= 2**32``.  The caller's tensors are never written.
"""
import torch
import torch.nn as nn

from . import _native as N
from .iwe import AveragedIWE, _events, _mask
from .iwe import _limits as _iwe_limits

__all__ = ["Sobel", "BrightnessConstancy"]


# ------------------------------------------------------------------ argument plumbing
def _validate(what, **tensors):
    """float32 GPU tensors on one device.  Nothing is copied."""
    for name, t in tensors.items():
        if not torch.is_tensor(t):
            raise TypeError("%s: %s must be a tensor, got %s" % (what, name, type(t).__name__))
        if t.dtype != torch.float32:
            raise TypeError("%s: %s is %s; the reconstruction kernels take float32 tensors, convert with .float()" % (what, name, t.dtype))
    N.require_gpu(*tensors.values())
    devices = {t.device for t in tensors.values()}
    if len(devices) > 1:
        raise ValueError("%s: tensors on different devices %s" % (what, sorted(str(d) for d in devices)))


def _limits(what, B, H, W, sorts=True):
    """``sorts``: the term's backward sorts four entries per pixel, whose positions are 32-bit."""
    if B < 1:
        raise ValueError("%s: the batch must hold at least one item, got B = %d" % (what, B))
    if H < 2 or W < 2:
        raise ValueError("%s: H and W must be at least 2, got H = %d, W = %d (the sample coordinate divides by n - 1)" % (what, H, W))
    if B * H * W >= 2 ** 32 - 1:
        raise ValueError("%s: B * H * W = %d >= 2**32 - 1" % (what, B * H * W))
    if sorts and 4 * B * H * W >= 2 ** 32:
        raise ValueError("%s: 4 * B * H * W = %d >= 2**32: scatter positions are 32-bit" % (what, 4 * B * H * W))


def _image4(what, name, t):
    if t.dim() != 4:
        raise ValueError("%s: %s must be [B, C, H, W], got %r" % (what, name, tuple(t.shape)))
    return tuple(int(s) for s in t.shape)


def _one_channel(what, name, t, B, H, W):
    if t.dim() != 4 or tuple(t.shape) != (B, 1, H, W):
        raise ValueError("%s: %s must be [%d, 1, %d, %d] (one channel), got %r" % (what, name, B, H, W, tuple(t.shape)))


def _flow(what, flow, H, W):
    if flow.dim() != 4 or flow.shape[1] != 2 or tuple(flow.shape[2:]) != (H, W):
        raise ValueError("%s: flow must be [B, 2, %d, %d], got %r" % (what, H, W, tuple(flow.shape)))
    return int(flow.shape[0])


def _buffer(fn, B, H, W, dev):
    need = int(fn(B, H, W))
    return torch.empty(max(need, 16), dtype=torch.uint8, device=dev), need


def _strides(flow):
    return [int(s) for s in flow.stride()]


def _scalar(grad):
    return grad.detach().to(torch.float32).contiguous()


# ------------------------------------------------------------------ myutils/gradients.py
class _Sobel(torch.autograd.Function):
    @staticmethod
    def forward(ctx, x):
        B, C, H, W = x.shape
        xd = x.detach().contiguous()
        gradx = torch.empty((B * C, 1, H, W), dtype=torch.float32, device=x.device)
        grady = torch.empty_like(gradx)
        with torch.cuda.device_of(x):
            rc = N.lib().ebfi_sobel_forward(N.ptr(xd), B * C, H, W, N.ptr(gradx), N.ptr(grady), N.stream_ptr(x.device))
        N.check(rc, "ebfi_sobel_forward")
        ctx.shape = (B, C, H, W)
        return gradx, grady

    @staticmethod
    def backward(ctx, ggx, ggy):
        B, C, H, W = ctx.shape
        ggx = None if ggx is None else ggx.detach().to(torch.float32).contiguous()
        ggy = None if ggy is None else ggy.detach().to(torch.float32).contiguous()
        some = ggx if ggx is not None else ggy
        if some is None:
            return None
        grad = torch.empty((B, C, H, W), dtype=torch.float32, device=some.device)
        with torch.cuda.device_of(some):
            rc = N.lib().ebfi_sobel_backward(N.ptr(ggx), N.ptr(ggy), B * C, H, W, N.ptr(grad), N.stream_ptr(some.device))
        N.check(rc, "ebfi_sobel_backward")
        return grad


class Sobel(nn.Module):
    """Spatial gradients by Sobel filters (reference myutils/gradients.py): ``x`` ``[B, C, H, W]`` is viewed as
    ``[B * C, 1, H, W]``, padded by replication, correlated with the two 3 x 3 kernels and divided by 8.  Returns
    ``(gradx, grady)``, both ``[B * C, 1, H, W]``, differentiable in ``x``."""

    def __init__(self, device):
        super().__init__()
        # the attributes a caller of the reference may read; the kernels have the pad and both filters built in
        smooth, slope = torch.tensor([1.0, 2.0, 1.0]), torch.tensor([-1.0, 0.0, 1.0])
        self.a = torch.outer(smooth, slope).view(1, 1, 3, 3).to(device)      # horizontal derivative
        self.b = torch.outer(slope, smooth).view(1, 1, 3, 3).to(device)      # vertical derivative
        self.pad = nn.ReplicationPad2d(1)

    def forward(self, x):
        what = "Sobel"
        _validate(what, x=x)
        B, C, H, W = _image4(what, "x", x)
        _limits(what, B * C, H, W, sorts=False)
        return _Sobel.apply(x)


# ------------------------------------------------------------------ loss/reconstruction.py
class _Generative(torch.autograd.Function):
    @staticmethod
    def forward(ctx, flow, img, cnt, avg, scaling):
        B, _, H, W = flow.shape
        C = int(cnt.shape[1])
        dev = flow.device
        f, im = flow.detach(), img.detach().contiguous()
        resid = torch.empty((B, H, W), dtype=torch.float32, device=dev)
        loss = torch.empty((), dtype=torch.float32, device=dev)
        ws, need = _buffer(N.lib().ebfi_bc_forward_workspace, B, H, W, dev)
        with torch.cuda.device_of(flow):
            rc = N.lib().ebfi_bc_generative_forward(N.ptr(f), *_strides(f), N.ptr(im), N.ptr(cnt), C, N.ptr(avg), B, H, W,
                                                    float(scaling), N.ptr(resid), N.ptr(loss), N.ptr(ws), need, N.stream_ptr(dev))
        N.check(rc, "ebfi_bc_generative_forward")
        ctx.save_for_backward(f, im, cnt, resid)
        ctx.scaling = float(scaling)
        return loss

    @staticmethod
    def backward(ctx, grad_loss):
        f, im, cnt, resid = ctx.saved_tensors
        B, _, H, W = f.shape
        dev = f.device
        g = _scalar(grad_loss)
        grad_flow = torch.empty((B, 2, H, W), dtype=torch.float32, device=dev) if ctx.needs_input_grad[0] else None
        grad_img = torch.empty((B, 1, H, W), dtype=torch.float32, device=dev) if ctx.needs_input_grad[1] else None
        fn = N.lib().ebfi_bc_workspace if grad_img is not None else N.lib().ebfi_bc_forward_workspace
        ws, need = _buffer(fn, B, H, W, dev)
        with torch.cuda.device_of(f):
            rc = N.lib().ebfi_bc_generative_backward(N.ptr(f), *_strides(f), N.ptr(im), N.ptr(cnt), int(cnt.shape[1]), N.ptr(resid),
                                                     B, H, W, ctx.scaling, N.ptr(g), N.ptr(grad_flow), N.ptr(grad_img), N.ptr(ws),
                                                     need, N.stream_ptr(dev))
        N.check(rc, "ebfi_bc_generative_backward")
        return grad_flow, grad_img, None, None, None


class _Temporal(torch.autograd.Function):
    @staticmethod
    def forward(ctx, flow, prev_img, img, scaling, weight):
        B, _, H, W = flow.shape
        dev = flow.device
        f, prev, im = flow.detach(), prev_img.detach().contiguous(), img.detach().contiguous()
        resid = torch.empty((B, H, W), dtype=torch.float32, device=dev)
        loss = torch.empty((), dtype=torch.float32, device=dev)
        ws, need = _buffer(N.lib().ebfi_bc_forward_workspace, B, H, W, dev)
        with torch.cuda.device_of(flow):
            rc = N.lib().ebfi_bc_temporal_forward(N.ptr(f), *_strides(f), N.ptr(prev), N.ptr(im), B, H, W, float(scaling),
                                                  float(weight), N.ptr(resid), N.ptr(loss), N.ptr(ws), need, N.stream_ptr(dev))
        N.check(rc, "ebfi_bc_temporal_forward")
        ctx.save_for_backward(f, prev, resid)
        ctx.args = (float(scaling), float(weight))
        return loss

    @staticmethod
    def backward(ctx, grad_loss):
        f, prev, resid = ctx.saved_tensors
        scaling, weight = ctx.args
        B, _, H, W = f.shape
        dev = f.device
        g = _scalar(grad_loss)
        new = lambda c, need: torch.empty((B, c, H, W), dtype=torch.float32, device=dev) if need else None
        grad_flow, grad_prev, grad_img = (new(c, ctx.needs_input_grad[k]) for k, c in enumerate((2, 1, 1)))
        fn = N.lib().ebfi_bc_workspace if grad_prev is not None else N.lib().ebfi_bc_forward_workspace
        ws, need = _buffer(fn, B, H, W, dev)
        with torch.cuda.device_of(f):
            rc = N.lib().ebfi_bc_temporal_backward(N.ptr(f), *_strides(f), N.ptr(prev), N.ptr(resid), B, H, W, scaling, weight,
                                                   N.ptr(g), N.ptr(grad_flow), N.ptr(grad_prev), N.ptr(grad_img), N.ptr(ws), need,
                                                   N.stream_ptr(dev))
        N.check(rc, "ebfi_bc_temporal_backward")
        return grad_flow, grad_prev, grad_img, None, None


class _TotalVariation(torch.autograd.Function):
    @staticmethod
    def forward(ctx, img, weight):
        B, C, H, W = img.shape
        dev = img.device
        im = img.detach().contiguous()
        loss = torch.empty((), dtype=torch.float32, device=dev)
        ws, need = _buffer(N.lib().ebfi_bc_forward_workspace, B * C, H, W, dev)
        with torch.cuda.device_of(img):
            rc = N.lib().ebfi_bc_tv_forward(N.ptr(im), B * C, H, W, float(weight), N.ptr(loss), N.ptr(ws), need, N.stream_ptr(dev))
        N.check(rc, "ebfi_bc_tv_forward")
        ctx.save_for_backward(im)
        ctx.weight = float(weight)
        return loss

    @staticmethod
    def backward(ctx, grad_loss):
        (im,) = ctx.saved_tensors
        B, C, H, W = im.shape
        g = _scalar(grad_loss)
        grad = torch.empty_like(im)
        with torch.cuda.device_of(im):
            rc = N.lib().ebfi_bc_tv_backward(N.ptr(im), B * C, H, W, ctx.weight, N.ptr(g), N.ptr(grad), N.stream_ptr(im.device))
        N.check(rc, "ebfi_bc_tv_backward")
        return grad, None


class BrightnessConstancy(nn.Module):
    """Self-supervised image reconstruction loss (reference loss/reconstruction.py): the generative model of event cameras
    (squared L2 of the brightness increment predicted from the image gradients and the flow against the averaged image of
    warped events), temporal consistency (L1 of the warping error between two reconstructed frames) and total variation."""

    def __init__(self, config, device):
        super().__init__()
        loader = config["loader"]
        self.device, self.res = device, loader["resolution"]
        self.flow_scaling = max(self.res)                      # flows are in units of the longer image side
        self.weights = config["loss"]["reconstruction_regul_weight"]      # (total variation, temporal consistency)
        self.sobel, self.averaged_iwe = Sobel(device), AveragedIWE(config, device)
        # the pixel-index image [1, 2, H, W] = (row, column) a caller of the reference may read; the kernels compute it from
        # the thread index
        rows, cols = torch.arange(float(self.res[0])), torch.arange(float(self.res[1]))
        self.indices = torch.stack(torch.meshgrid(rows, cols, indexing="ij")).unsqueeze(0).to(device)

    def _sizes(self, what, flow):
        H, W = int(self.res[0]), int(self.res[1])
        B = _flow(what, flow, H, W)
        _limits(what, B, H, W)
        return B, H, W

    def generative_model(self, flow, img, inputs):
        """``flow`` [B, 2, H, W], ``img`` [B, 1, H, W] (the last reconstructed image), ``inputs`` the dataloader dictionary with
        ``inp_cnt`` [B, C, H, W], ``inp_list`` [B, N, 4] and ``inp_pol_mask`` [B, N, 2].  Gradients into ``flow`` and ``img``."""
        what = "generative_model"
        if not torch.is_tensor(flow):
            raise TypeError("%s: flow must be a tensor, got %s" % (what, type(flow).__name__))
        for key in ("inp_cnt", "inp_list", "inp_pol_mask"):
            if not torch.is_tensor(inputs[key]):
                raise TypeError("%s: inputs[%r] must be a tensor, got %s" % (what, key, type(inputs[key]).__name__))
        cnt, event_list, pol_mask = (inputs[k].to(flow.device) for k in ("inp_cnt", "inp_list", "inp_pol_mask"))
        _validate(what, flow=flow, img=img, inp_cnt=cnt, inp_list=event_list, inp_pol_mask=pol_mask)
        B, H, W = self._sizes(what, flow)
        _one_channel(what, "img", img, B, H, W)
        if cnt.dim() != 4 or cnt.shape[1] < 1 or (int(cnt.shape[0]),) + tuple(cnt.shape[2:]) != (B, H, W):
            raise ValueError("%s: inputs['inp_cnt'] must be [%d, C, %d, %d], got %r" % (what, B, H, W, tuple(cnt.shape)))
        # what AveragedIWE would refuse, before any device work
        n_items, n_events = _events(what, event_list)
        if n_items != B:
            raise ValueError("%s: inputs['inp_list'] holds %d items, the flow %d" % (what, n_items, B))
        _mask(what, "inputs['inp_pol_mask']", pol_mask, B, n_events, 2)
        _iwe_limits(what, B, n_events, H, W)
        if int(self.averaged_iwe.batch_size) != B:
            raise ValueError("%s: config['loader']['batch_size'] = %d, but the flow holds %d items (AveragedIWE loops over "
                             "batch_size items of it)" % (what, int(self.averaged_iwe.batch_size), B))
        cnt = cnt.detach().contiguous()
        f = flow.detach()
        masked = torch.empty((B, 2, H, W), dtype=torch.float32, device=flow.device)
        with torch.cuda.device_of(flow):
            rc = N.lib().ebfi_bc_mask_flow(N.ptr(f), *_strides(f), N.ptr(cnt), int(cnt.shape[1]), B, H, W, N.ptr(masked),
                                           N.stream_ptr(flow.device))
        N.check(rc, "ebfi_bc_mask_flow")
        avg = self.averaged_iwe(masked, event_list, pol_mask)
        return _Generative.apply(flow, img, cnt, avg, self.flow_scaling)

    def temporal_consistency(self, flow, prev_img, img):
        """``weights[1]`` times the L1 norm of ``img - sample(prev_img)`` under the flow as given.  Gradients into all three."""
        what = "temporal_consistency"
        _validate(what, flow=flow, prev_img=prev_img, img=img)
        B, H, W = self._sizes(what, flow)
        _one_channel(what, "prev_img", prev_img, B, H, W)
        _one_channel(what, "img", img, B, H, W)
        return _Temporal.apply(flow, prev_img, img, self.flow_scaling, self.weights[1])

    def regularization(self, img):
        """``weights[0]`` times the total variation of ``img`` [B, C, H, W] with forward differences."""
        what = "regularization"
        _validate(what, img=img)
        B, C, H, W = _image4(what, "img", img)
        _limits(what, B * C, H, W, sorts=False)
        return _TotalVariation.apply(img, self.weights[0])
