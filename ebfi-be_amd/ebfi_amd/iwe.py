"""loss/flow.py and myutils/iwe.py on the device (csrc/iwe.hip): ``purge_unfeasible``, ``get_interpolation``, ``interpolate``,
``deblur_events`` and ``compute_pol_iwe`` with the reference's signatures and defaults, the contrast-maximisation loss
``EventWarping`` (Zhu et al., CVPR'19, section 3.2) with its gradient into the flow, and ``AveragedIWE``.

The event layout is the code's, not the docstrings': ``event_list[b, n] = (ts, y, x, p)``, float32 ``[B, N, 4]``.

The reference adds fractional float32 weights with ``scatter_add_``; on a GPU eager PyTorch runs that, and the gradient's
scatter back into the flow, with float atomics, whose order changes from run to run.  Here the law is the reference run with
one thread: every pixel receives its addends in ascending list position, fp32, unfused.  The library sorts the list entries by
pixel (stable, integer arithmetic only) and lets one thread per pixel add its run in order; the gradient is a gather over the
events sorted by source pixel.  Two calls give the same bits, and every call can be captured in a graph: nothing synchronises,
allocates inside the library or reads a value back.

Defined here where the reference is not: an index outside ``[0, H * W)`` handed to ``interpolate`` is dropped (the reference
raises); an event whose source pixel is outside the image or not integral takes flow 0 and weight 0 (the reference's ``gather``
raises or asserts); a non-finite warped coordinate gets weight 0 (the reference's ``.long()`` of it is undefined) -- a NaN in
the flow still reaches the loss through the smoothness term.  Unfeasible corners get index ``0.0`` where the reference may
store ``-0.0``.

float32 GPU tensors only; float64, CPU tensors, mixed devices, ``4 * B * N >= 2**32`` and ``B * H * W >= 2**32 - 1`` are
refused.  The caller's tensors are never written.  ``BrightnessConstancy`` (loss/reconstruction.py), the consumer of
``AveragedIWE``, is in ebfi_amd/bcloss.py.
"""
import torch
import torch.nn as nn

from . import _native as N

__all__ = ["purge_unfeasible", "get_interpolation", "interpolate", "deblur_events", "compute_pol_iwe", "EventWarping",
           "AveragedIWE"]


# ------------------------------------------------------------------ argument plumbing
def _validate(what, **tensors):
    """float32 GPU tensors on one device; None is skipped.  Nothing is copied."""
    given = {k: t for k, t in tensors.items() if t is not None}
    for name, t in given.items():
        if not torch.is_tensor(t):
            raise TypeError("%s: %s must be a tensor, got %s" % (what, name, type(t).__name__))
        if t.dtype != torch.float32:
            raise TypeError("%s: %s is %s; the warping kernels take float32 tensors, convert with .float()" % (what, name, t.dtype))
    N.require_gpu(*given.values())
    devices = {t.device for t in given.values()}
    if len(devices) > 1:
        raise ValueError("%s: tensors on different devices %s" % (what, sorted(str(d) for d in devices)))


def _dense(t):
    return None if t is None else t.detach().contiguous()


def _check(what, **tensors):
    """_validate, then detached contiguous tensors in the order given (flow maps do not come here: the kernels read them
    through their strides)."""
    _validate(what, **tensors)
    return [_dense(t) for t in tensors.values()]


def _limits(what, B, n, H, W):
    if B < 1 or H < 1 or W < 1:
        raise ValueError("%s: batch size and resolution must be at least 1, got B = %d, H = %d, W = %d" % (what, B, H, W))
    if 4 * B * n >= 2 ** 32:
        raise ValueError("%s: 4 * B * N = %d >= 2**32: list positions are 32-bit" % (what, 4 * B * n))
    if B * H * W >= 2 ** 32 - 1:
        raise ValueError("%s: B * H * W = %d >= 2**32 - 1: pixel keys are 32-bit" % (what, B * H * W))


def _events(what, event_list):
    if event_list.dim() != 3 or event_list.shape[2] != 4:
        raise ValueError("%s: event_list must be [B, N, 4] = (ts, y, x, p), got %r" % (what, tuple(event_list.shape)))
    return int(event_list.shape[0]), int(event_list.shape[1])


def _flow(what, flow, B, H, W):
    if flow.dim() != 4 or tuple(flow.shape) != (B, 2, H, W):
        raise ValueError("%s: flow must be [%d, 2, %d, %d], got %r" % (what, B, H, W, tuple(flow.shape)))


def _mask(what, name, mask, B, n, cols):
    if mask.dim() != 3 or tuple(mask.shape) != (B, n, cols):
        raise ValueError("%s: %s must be [%d, %d, %d], got %r" % (what, name, B, n, cols, tuple(mask.shape)))


def _workspace(B, n, H, W, dev):
    need = int(N.lib().ebfi_iwe_workspace(B, n, H, W))
    return torch.empty(max(need, 16), dtype=torch.uint8, device=dev), need


def _strides(flow):
    return [int(s) for s in flow.stride()]


# ------------------------------------------------------------------ myutils/iwe.py
@torch.no_grad()
def purge_unfeasible(x, res):
    """Zero the locations outside the image and return the mask that did it (reference myutils/iwe.py:4-17).  Elementwise
    and order-free: plain tensor arithmetic on the device of ``x``."""
    H, W = res[0], res[1]
    y, x_ = x[..., 0:1], x[..., 1:2]
    outside = (y < 0) | (y >= H) | (x_ < 0) | (x_ >= W)        # (a NaN is not outside: it keeps mask 1, as in the reference)
    mask = (~outside).to(x.dtype)
    return x * mask, mask


@torch.no_grad()
def get_interpolation(events, flow, tref, res, flow_scaling, round_idx=False):
    """Warp the events by their per-event flow ``[B, N, 2] = (y, x)`` to ``tref`` and return ``(idx, weights)``, float32
    ``[B, M, 1]`` with ``M = N`` (``round_idx``) or ``4 N`` (top-left, top-right, bottom-left, bottom-right lists in turn)."""
    what = "get_interpolation"
    events, flow = _check(what, events=events, flow=flow)
    B, n = _events(what, events)
    H, W = int(res[0]), int(res[1])
    if tuple(flow.shape) != (B, n, 2):
        raise ValueError("%s: flow must be the per-event flow [%d, %d, 2], got %r" % (what, B, n, tuple(flow.shape)))
    _limits(what, B, n, H, W)
    m = n if round_idx else 4 * n
    idx = torch.empty((B, m, 1), dtype=torch.float32, device=events.device)
    weights = torch.empty((B, m, 1), dtype=torch.float32, device=events.device)
    with torch.cuda.device_of(events):
        rc = N.lib().ebfi_iwe_get_interpolation(N.ptr(events), N.ptr(flow), B, n, float(tref), H, W, float(flow_scaling),
                                                1 if round_idx else 0, N.ptr(idx), N.ptr(weights), N.stream_ptr(events.device))
    N.check(rc, "ebfi_iwe_get_interpolation")
    return idx, weights


@torch.no_grad()
def interpolate(idx, weights, res, polarity_mask=None):
    """Image ``[B, 1, H, W]`` of the warped events: every pixel adds ``weights * polarity_mask`` of its list entries in
    ascending list position.  ``idx`` ``[B, M, 1]``, int64 (as the reference passes it) or float32 (truncated).  An index
    outside ``[0, H * W)`` is dropped (the reference raises)."""
    what = "interpolate"
    if not torch.is_tensor(idx) or idx.dtype not in (torch.int64, torch.float32):
        raise TypeError("%s: idx must be an int64 or float32 tensor, got %s" % (what, getattr(idx, "dtype", type(idx).__name__)))
    weights, polarity_mask = _check(what, weights=weights, polarity_mask=polarity_mask)
    N.require_gpu(idx)
    if idx.device != weights.device:
        raise ValueError("%s: tensors on different devices %s" % (what, sorted((str(idx.device), str(weights.device)))))
    if idx.dim() != 3 or idx.shape[2] != 1:
        raise ValueError("%s: idx must be [B, M, 1], got %r" % (what, tuple(idx.shape)))
    B, m = int(idx.shape[0]), int(idx.shape[1])
    H, W = int(res[0]), int(res[1])
    for name, t in (("weights", weights), ("polarity_mask", polarity_mask)):
        if t is not None and tuple(t.shape) != (B, m, 1):
            raise ValueError("%s: %s must be [%d, %d, 1], got %r" % (what, name, B, m, tuple(t.shape)))
    n4 = (m + 3) // 4
    _limits(what, B, n4, H, W)
    idx = idx.detach().contiguous()
    out = torch.empty((B, 1, H, W), dtype=torch.float32, device=weights.device)
    ws, need = _workspace(B, n4, H, W, weights.device)
    with torch.cuda.device_of(weights):
        rc = N.lib().ebfi_iwe_interpolate(N.ptr(idx), 1 if idx.dtype == torch.int64 else 0, N.ptr(weights), N.ptr(polarity_mask),
                                          B, m, H, W, N.ptr(out), N.ptr(ws), need, N.stream_ptr(weights.device))
    N.check(rc, "ebfi_iwe_interpolate")
    return out


def _deblur(what, flow, event_list, res, flow_scaling, round_idx, mask_a, mask_b):
    planes = 2 if mask_b is not None else 1
    _validate(what, flow=flow, event_list=event_list, mask_a=mask_a, mask_b=mask_b)
    flow, event_list, mask_a, mask_b = flow.detach(), _dense(event_list), _dense(mask_a), _dense(mask_b)
    B, n = _events(what, event_list)
    H, W = int(res[0]), int(res[1])
    flow = flow.reshape(B, 2, H, W) if flow.dim() == 3 else flow       # (the reference views the flow as [B, 2, H * W] itself)
    _flow(what, flow, B, H, W)
    for name, t in (("the first mask", mask_a), ("the second mask", mask_b)):
        if t is not None:
            _mask(what, name, t, B, n, 1)
    _limits(what, B, n, H, W)
    out = torch.empty((B, planes, H, W), dtype=torch.float32, device=event_list.device)
    ws, need = _workspace(B, n, H, W, event_list.device)
    with torch.cuda.device_of(event_list):
        rc = N.lib().ebfi_iwe_deblur(N.ptr(flow), *_strides(flow), N.ptr(event_list), B, n, H, W, float(flow_scaling),
                                     1 if round_idx else 0, planes, N.ptr(mask_a), N.ptr(mask_b), 1, N.ptr(out), N.ptr(ws), need,
                                     N.stream_ptr(event_list.device))
    N.check(rc, "ebfi_iwe_deblur (%s)" % what)
    return out


@torch.no_grad()
def deblur_events(flow, event_list, res, flow_scaling=128, round_idx=True, polarity_mask=None):
    """Image ``[B, 1, H, W]`` of the events warped to ``tref = 1`` by the flow at their source pixels.  ``polarity_mask``
    ``[B, N, 1]``; the bilinear form needs one, as in the reference."""
    if not round_idx and polarity_mask is None:
        raise TypeError("deblur_events: round_idx=False needs a polarity_mask (the reference concatenates it four times)")
    return _deblur("deblur_events", flow, event_list, res, flow_scaling, round_idx, polarity_mask, None)


@torch.no_grad()
def compute_pol_iwe(flow, event_list, res, pos_mask, neg_mask, flow_scaling=128, round_idx=True):
    """Per-polarity image ``[B, 2, H, W]`` of the warped events: one warp and one sort serve both masks."""
    if pos_mask is None or neg_mask is None:
        raise TypeError("compute_pol_iwe: pos_mask and neg_mask are required")
    return _deblur("compute_pol_iwe", flow, event_list, res, flow_scaling, round_idx, pos_mask, neg_mask)


# ------------------------------------------------------------------ loss/flow.py
class _Warping(torch.autograd.Function):
    """The fused loss of one flow.  The images of both directions and the source-pixel index of the events are the
    caller-owned buffers the gradient kernel reads."""

    @staticmethod
    def forward(ctx, flow, events, pol_mask, index, index_bytes, H, W, flow_scaling, weight):
        B, n = int(events.shape[0]), int(events.shape[1])
        dev = events.device
        f = flow.detach()
        images = torch.empty((2, B, 4, H * W), dtype=torch.float32, device=dev)
        loss = torch.empty((), dtype=torch.float32, device=dev)
        ws, need = _workspace(B, n, H, W, dev)
        with torch.cuda.device_of(events):
            rc = N.lib().ebfi_iwe_warping_forward(N.ptr(f), *_strides(f), N.ptr(events), N.ptr(pol_mask), B, n, H, W,
                                                  float(flow_scaling), float(weight), N.ptr(images), N.ptr(loss), N.ptr(ws), need,
                                                  N.stream_ptr(dev))
        N.check(rc, "ebfi_iwe_warping_forward")
        ctx.save_for_backward(f, events, pol_mask, images, index)
        ctx.args = (index_bytes, H, W, float(flow_scaling), float(weight))
        return loss

    @staticmethod
    def backward(ctx, grad_loss):
        f, events, pol_mask, images, index = ctx.saved_tensors
        index_bytes, H, W, flow_scaling, weight = ctx.args
        B, n = int(events.shape[0]), int(events.shape[1])
        dev = events.device
        g = grad_loss.detach().to(torch.float32).contiguous()
        grad_flow = torch.empty((B, 2, H, W), dtype=torch.float32, device=dev)
        with torch.cuda.device_of(events):
            rc = N.lib().ebfi_iwe_warping_backward(N.ptr(f), *_strides(f), N.ptr(events), N.ptr(pol_mask), B, n, H, W,
                                                   flow_scaling, weight, N.ptr(images), N.ptr(index), index_bytes, N.ptr(g),
                                                   N.ptr(grad_flow), N.stream_ptr(dev))
        N.check(rc, "ebfi_iwe_warping_backward")
        return (grad_flow,) + (None,) * 8


class EventWarping(nn.Module):
    """Contrast-maximisation loss (reference loss/flow.py:15-110): the per-pixel, per-polarity image of averaged stamps of the
    events after motion compensation, forward (``tref = 1``) and backward (``tref = 0``), plus a Charbonnier smoothness term of
    the flow.  Differentiable in the flows; one device scalar."""

    def __init__(self, config, device):
        super(EventWarping, self).__init__()
        self.device, self.weight = device, config["loss"]["flow_regul_weight"]      # (the smoothness term's coefficient)

    def forward(self, flow_list, event_list, pol_mask, resolution):
        what = "EventWarping"
        H, W = int(resolution[0]), int(resolution[1])
        self.flow_scaling = max(resolution)
        flow_list = list(flow_list)
        named = {"flow_list[%d]" % k: flow for k, flow in enumerate(flow_list)}
        _validate(what, event_list=event_list, pol_mask=pol_mask, **named)
        event_list, pol_mask = _dense(event_list), _dense(pol_mask)
        B, n = _events(what, event_list)
        _mask(what, "pol_mask", pol_mask, B, n, 2)
        _limits(what, B, n, H, W)
        flows = []
        for flow in flow_list:                                 # (as given: strided and non-leaf flows keep their graph)
            flow = flow.reshape(B, 2, H, W) if flow.dim() == 3 else flow
            _flow(what, flow, B, H, W)
            flows.append(flow)
        dev = event_list.device
        # by source pixel: one sort for every flow and both directions; B N entries, kept until the last backward
        index_bytes = int(N.lib().ebfi_iwe_index_bytes(B, n, H, W))
        index = torch.empty(max(index_bytes, 16), dtype=torch.uint8, device=dev)
        with torch.cuda.device_of(event_list):
            rc = N.lib().ebfi_iwe_source_index(N.ptr(event_list), B, n, H, W, N.ptr(index), index_bytes, N.stream_ptr(dev))
        N.check(rc, "ebfi_iwe_source_index")
        loss = 0
        for flow in flows:
            loss = loss + _Warping.apply(flow, event_list, pol_mask, index, index_bytes, H, W, self.flow_scaling, self.weight)
        return loss


class AveragedIWE(nn.Module):
    """Image ``[B, 2, H, W]`` of the per-pixel, per-polarity average number of warped events (reference loss/flow.py:113-232):
    the rounded warp's counts, each divided by the number of distinct source pixels that feed the pixel.  Forward only, as
    the rounded indices carry no gradient in the reference either."""

    def __init__(self, config, device):
        super(AveragedIWE, self).__init__()
        loader = config["loader"]
        self.device, self.res, self.batch_size = device, loader["resolution"], loader["batch_size"]
        self.flow_scaling = max(self.res)                      # flows are in units of the longer image side

    @torch.no_grad()
    def forward(self, flow, event_list, pol_mask):
        what = "AveragedIWE"
        H, W = int(self.res[0]), int(self.res[1])
        _validate(what, flow=flow, event_list=event_list, pol_mask=pol_mask)
        flow, event_list, pol_mask = flow.detach(), _dense(event_list), _dense(pol_mask)
        B, n = _events(what, event_list)
        if int(self.batch_size) != int(flow.shape[0]):
            raise ValueError("%s: config['loader']['batch_size'] = %d, but the flow holds %d items (the reference loops over "
                             "batch_size items of it)" % (what, int(self.batch_size), int(flow.shape[0])))
        flow = flow.reshape(B, 2, H, W) if flow.dim() == 3 else flow
        _flow(what, flow, B, H, W)
        _mask(what, "pol_mask", pol_mask, B, n, 2)
        _limits(what, B, n, H, W)
        dev = event_list.device
        if n == 0:
            return torch.zeros((B, 2, H, W), dtype=torch.float32, device=dev)
        out = torch.empty((B, 2, H, W), dtype=torch.float32, device=dev)
        ws, need = _workspace(B, n, H, W, dev)
        with torch.cuda.device_of(event_list):
            rc = N.lib().ebfi_iwe_averaged(N.ptr(flow), *_strides(flow), N.ptr(event_list), N.ptr(pol_mask), B, n, H, W,
                                           float(self.flow_scaling), N.ptr(out), N.ptr(ws), need, N.stream_ptr(dev))
        N.check(rc, "ebfi_iwe_averaged")
        return out
