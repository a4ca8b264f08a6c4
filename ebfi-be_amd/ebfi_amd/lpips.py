"""LPIPS on the device (reference: loss/restore.py:10-40 perceptual_loss(net='alex') and the PerceptualSimilarity package it
wraps, version 0.1, eval mode, spatial=False).

``load_alex_lpips(lin_path, backbone_path, device)`` reads the two weight files a machine that ran the reference holds -- the
linear heads ``loss/PerceptualSimilarity/models/weights/v0.1/alex.pth`` and torchvision's AlexNet state dict
(``alexnet-owt-7be5be79.pth`` of the torch hub cache) -- checks every key and shape, and packs the parameters once.  Calling the
returned object on an [N, C, H, W] fp32 pair (C in {1, 3}; H, W >= 31) runs ``ebfi_lpips_alex`` -- the AlexNet trunk as
implicit-GEMM convolutions on fp32 MFMA, then the normalised, head-weighted distances, all on the current stream with no host
synchronisation -- and returns the float32 device tensor lpips [N].  Definition: include/ebfi_hip.h.
"""
import torch

from . import _native as N

NET = "alex"
CONV_KEYS = ("features.0", "features.3", "features.6", "features.8", "features.10")
CONV_SHAPES = ((64, 3, 11, 11), (192, 64, 5, 5), (384, 192, 3, 3), (256, 384, 3, 3), (256, 256, 3, 3))
LIN_KEYS = tuple("lin%d.model.1.weight" % l for l in range(5))
MIN_SIZE = 31      # the smallest H / W AlexNet's trunk accepts


def _state_dict(path, what):
    sd = torch.load(path, map_location="cpu", weights_only=True)
    if not isinstance(sd, dict):
        raise ValueError("%s: %s is not a state dict (got %s)" % (what, path, type(sd).__name__))
    return sd


def _take(sd, key, shape, path):
    if key not in sd:
        raise KeyError("%s has no key %r" % (path, key))
    t = sd[key]
    if not torch.is_tensor(t) or tuple(t.shape) != tuple(shape):
        raise ValueError("%s: %r has shape %s, expected %s" % (path, key, tuple(getattr(t, "shape", ())), tuple(shape)))
    return t.detach().to(torch.float32).contiguous()


def read_alex_weights(lin_path, backbone_path):
    """The 5 conv weights, 5 biases and 5 head vectors as CPU float32 tensors, from the reference's v0.1 alex.pth and a
    torchvision AlexNet state dict (classifier.* is ignored).  A missing or mis-shaped key raises, naming it."""
    lin = _state_dict(lin_path, "the LPIPS linear heads")
    trunk = _state_dict(backbone_path, "the AlexNet trunk")
    ws, bs, hs = [], [], []
    for key, shape, lkey in zip(CONV_KEYS, CONV_SHAPES, LIN_KEYS):
        ws.append(_take(trunk, key + ".weight", shape, backbone_path))
        bs.append(_take(trunk, key + ".bias", shape[:1], backbone_path))
        hs.append(_take(lin, lkey, (1, shape[0], 1, 1), lin_path).reshape(-1))
    return ws, bs, hs


class AlexLPIPS:
    """LPIPS v0.1 with the AlexNet trunk; parameters packed once on `device`."""

    def __init__(self, conv_w, conv_b, lin_w, device):
        self.device = torch.device(device)
        if self.device.type != "cuda":
            raise NotImplementedError("LPIPS runs on an MI355X through libebfi_hip.so only (got device %s)" % self.device)
        if self.device.index is None:
            self.device = torch.device("cuda", torch.cuda.current_device())
        h = N.lib()
        ws = [w.to(self.device, torch.float32).contiguous() for w in conv_w]
        bs = [b.to(self.device, torch.float32).contiguous() for b in conv_b]
        hs = [v.to(self.device, torch.float32).contiguous() for v in lin_w]
        nbytes = h.ebfi_lpips_params_bytes()
        self.params = torch.empty(nbytes // 4, dtype=torch.float32, device=self.device)
        arr = lambda ts: (N._vp * 5)(*[t.data_ptr() for t in ts])   # noqa: E731
        with torch.cuda.device_of(self.params):
            rc = h.ebfi_lpips_pack_params(arr(ws), arr(bs), arr(hs), N.ptr(self.params), nbytes, N.stream_ptr(self.device))
        N.check(rc, "ebfi_lpips_pack_params")
        self._keep = (ws, bs, hs)      # (the pack kernels read them on the stream)
        self._workspaces = {}

    def _workspace(self, stream, shape):
        key = (stream, shape)
        ws = self._workspaces.get(key)
        if ws is None:
            self._workspaces.clear()   # (one config-5 workspace is 1.2 GB: keep only the latest shape)
            nbytes = N.lib().ebfi_lpips_workspace(*shape)
            ws = torch.empty(max(nbytes // 8, 1), dtype=torch.float64, device=self.device)
            self._workspaces[key] = ws
        return ws

    @torch.no_grad()
    def __call__(self, pred, target, normalize=True, per_layer=False):
        """lpips [N] (float32, on the device) of pred vs target [N, C, H, W], C in {1, 3}: normalize=True takes [0, 1]
        images, False [-1, 1] ones.  per_layer=True also returns the [N, 5] layer terms.  Strided views with unit column
        stride are read in place."""
        N.require_gpu(pred, target)
        if pred.dim() != 4 or pred.shape != target.shape:
            raise ValueError("LPIPS takes two [N, C, H, W] tensors of one shape, got %s and %s"
                             % (tuple(pred.shape), tuple(target.shape)))
        if pred.dtype != torch.float32 or target.dtype != torch.float32:
            raise ValueError("LPIPS takes float32 tensors, got %s / %s" % (pred.dtype, target.dtype))
        if pred.device != self.device or target.device != self.device:
            raise ValueError("pred on %s, target on %s, weights on %s" % (pred.device, target.device, self.device))
        n, c, hgt, wid = (int(v) for v in pred.shape)
        if c not in (1, 3):
            raise ValueError("LPIPS takes 1 or 3 channels, got %d (loss.perceptual_loss averages other counts per channel)" % c)
        if hgt < MIN_SIZE or wid < MIN_SIZE:
            raise ValueError("LPIPS (AlexNet) needs H, W >= %d, got %d x %d" % (MIN_SIZE, hgt, wid))
        pred = pred if pred.stride(3) == 1 else pred.contiguous()
        target = target if target.stride(3) == 1 else target.contiguous()
        out = torch.empty(n, dtype=torch.float32, device=self.device)
        layers = torch.empty(n, 5, dtype=torch.float32, device=self.device) if per_layer else None
        if n:
            with torch.cuda.device_of(pred):
                stream = N.stream_ptr(self.device)
                ws = self._workspace(stream.value, (n, c, hgt, wid))
                rc = N.lib().ebfi_lpips_alex(N.ptr(pred), N.i64x4(pred.stride()), N.ptr(target), N.i64x4(target.stride()), n, c, hgt,
                                             wid, 1 if normalize else 0, N.ptr(self.params), N.ptr(ws), ws.numel() * 8, N.ptr(out),
                                             N.ptr(layers), stream)
            N.check(rc, "ebfi_lpips_alex")
        return (out, layers) if per_layer else out


def load_alex_lpips(lin_path, backbone_path, device="cuda", net=NET):
    """AlexLPIPS from the reference's v0.1 heads (lin_path) and a torchvision AlexNet state dict (backbone_path)."""
    if net != NET:
        raise NotImplementedError("LPIPS net=%r is not implemented: only 'alex' has device kernels here (the reference also "
                                  "offers 'vgg' and 'squeeze')" % (net,))
    return AlexLPIPS(*read_alex_weights(lin_path, backbone_path), device)
