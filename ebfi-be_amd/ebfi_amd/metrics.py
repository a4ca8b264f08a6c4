"""Evaluation metrics on the device (reference: loss/restore.py:43-92 psnr_loss / ssim_loss, nn.MSELoss, and the averaging of
myutils/utils.py:123-144 MetricTracker).

``frame_metrics(pred, target)`` scores every frame of an [N, C, H, W] fp32 pair with ``ebfi_image_metrics`` -- two launches on
the current stream, no host synchronisation -- and returns device tensors ``(psnr, ssim, mse)`` of shape [N].  Definitions
(include/ebfi_hip.h): PSNR with the reference's per-channel data range (one-channel images clipped to [0, 1], range 1), SSIM
of scikit-image's structural_similarity defaults (7x7 uniform window, sample covariance, interior mean) with data range
``ssim_data_range`` (2.0: what the reference's float32 call without data_range uses), MSE over C*H*W.  A NaN or inf in a
frame makes its three values NaN.  LPIPS is ebfi_amd.lpips: it needs two weight files named by the caller (the reference's
v0.1 heads and torchvision's AlexNet trunk), which no download supplies here; without them it is left out and LPIPS_UNAVAILABLE
says why.
"""
import torch

from . import _native as N

LPIPS_UNAVAILABLE = ("LPIPS is not computed: its AlexNet trunk weights come from a torchvision download that this package "
                     "cannot rely on (the reference repository carries only the linear heads)")

_workspaces = {}


def _workspace(device, stream, shape):
    key = (device, stream, shape)
    ws = _workspaces.get(key)
    if ws is None:
        nbytes = N.lib().ebfi_image_metrics_workspace(*shape)
        ws = torch.empty(max(nbytes // 8, 1), dtype=torch.float64, device=device)   # (float64: 16-byte aligned storage)
        _workspaces[key] = ws
    return ws


@torch.no_grad()
def frame_metrics(pred, target, ssim_data_range=2.0):
    """(psnr, ssim, mse), each a float32 device tensor [N], of pred vs target [N, C, H, W] (fp32 tensors or strided views
    with unit column stride; both on the same GPU).  Runs on the current stream; nothing is copied back."""
    N.require_gpu(pred, target)
    if pred.dim() != 4 or pred.shape != target.shape:
        raise ValueError("frame_metrics takes two [N, C, H, W] tensors of one shape, got %s and %s"
                         % (tuple(pred.shape), tuple(target.shape)))
    if pred.dtype != torch.float32 or target.dtype != torch.float32:
        raise ValueError("frame_metrics takes float32 tensors, got %s / %s" % (pred.dtype, target.dtype))
    if pred.device != target.device:
        raise ValueError("pred on %s, target on %s" % (pred.device, target.device))
    n, c, h, w = (int(v) for v in pred.shape)
    if h < 7 or w < 7:
        raise ValueError("SSIM needs H, W >= 7 (its window is 7x7), got %d x %d" % (h, w))
    # the kernel reads rows through arbitrary strides but needs unit column stride
    pred = pred if pred.stride(3) == 1 or w == 1 else pred.contiguous()
    target = target if target.stride(3) == 1 or w == 1 else target.contiguous()
    psnr = torch.empty(n, dtype=torch.float32, device=pred.device)
    ssim = torch.empty_like(psnr)
    mse = torch.empty_like(psnr)
    if n == 0:
        return psnr, ssim, mse
    with torch.cuda.device_of(pred):
        stream = N.stream_ptr(pred.device)
        ws = _workspace(pred.device, stream.value, (n, c, h, w))
        rc = N.lib().ebfi_image_metrics(N.ptr(pred), N.i64x4(pred.stride()), N.ptr(target), N.i64x4(target.stride()), n, c, h, w,
                                        float(ssim_data_range), N.ptr(ws), ws.numel() * 8, N.ptr(psnr), N.ptr(ssim), N.ptr(mse),
                                        stream)
    N.check(rc, "ebfi_image_metrics")
    return psnr, ssim, mse


class MetricTracker:
    """Running averages per key, as myutils/utils.py:123-144 keeps them: update(key, value, n) adds value * n to the key's
    total and n to its count; result() is {key: total / count} (0.0 for a key never updated)."""

    def __init__(self, keys):
        self.keys = list(keys)
        self.reset()

    def reset(self):
        self._total = {k: 0.0 for k in self.keys}
        self._count = {k: 0 for k in self.keys}

    def update(self, key, value, n=1):
        self._total[key] += float(value) * n
        self._count[key] += n

    def avg(self, key):
        return self._total[key] / self._count[key] if self._count[key] else 0.0

    def result(self):
        return {k: self.avg(k) for k in self.keys}
