"""LPIPS on the device (reference: loss/restore.py:10-40 perceptual_loss(net='alex') and the PerceptualSimilarity package it
wraps, version 0.1, eval mode, spatial=False).

``load_alex_lpips(lin_path, backbone_path, device)`` reads the two weight files a machine that ran the reference holds -- the
linear heads ``loss/PerceptualSimilarity/models/weights/v0.1/alex.pth`` and torchvision's AlexNet state dict
(``alexnet-owt-7be5be79.pth`` of the torch hub cache) -- checks every key and shape, and packs the parameters once.  Calling the
returned object on an [N, C, H, W] fp32 pair (C in {1, 3}; H, W >= 31) runs ``ebfi_lpips_alex`` -- the AlexNet trunk as
implicit-GEMM convolutions on fp32 MFMA, then the normalised, head-weighted distances, all on the current stream with no host
synchronisation -- and returns the float32 device tensor lpips [N].  Definition: include/ebfi_hip.h.

``load_vgg_lpips(lin_path, backbone_path, device)`` is the VGG-16 variant (perceptual_loss(net='vgg')): the heads
``.../weights/v0.1/vgg.pth`` and torchvision's ``vgg16-397923af.pth``; H, W >= 16; ``ebfi_lpips_vgg`` runs the 13 convolutions on
the library's exact-fp32 3x3 forward and one tap kernel per layer.  ``load_lpips(net, ...)`` dispatches over 'alex' and 'vgg'.

``VggLPIPS.loss(pred, target)`` is the same value as a training loss (the reference builds perceptual_loss beside its Laplacian
and census terms, train_ours.py:765 -- with its default trunk, AlexNet): one autograd node whose forward,
``ebfi_lpips_vgg_forward_train``, keeps the 13 ReLU maps of the pred images and the 5 tap maps of the target images, and whose
backward, ``ebfi_lpips_vgg_backward``, runs one fused tap adjoint per layer (distance gradient plus the max-pool's routed
gradient) and the 13 data gradients of the library's exact-fp32 3x3 kernel.  pred gets the gradient, the target none.

``AlexLPIPSLoss`` (``load_alex_lpips(..., train=True)``) is the AlexNet trunk with the same ``loss``: the reference's own
training term.  Its forward, ``ebfi_lpips_alex_forward_train``, is the score's kernels on a workspace that also holds two
gradient maps; its backward, ``ebfi_lpips_alex_backward``, runs five tap adjoints (the 3x3/s2 pools' gradient gathered inside),
an exact-fp32 MFMA data gradient for conv5 .. conv2 (3x3 and 5x5) and a direct one for the 11x11 stride-4 layer, whose
epilogue writes the gradient of pred.  ``AlexLPIPS`` itself stays a score and has no ``loss``: the data-gradient
weights are packed only for the loss class.
"""
import weakref

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
    """LPIPS v0.1 with the AlexNet trunk; parameters packed once on `device`.  A score only: AlexLPIPSLoss adds the training
    loss (and the weights its data gradients read); VggLPIPS.loss is the VGG-16 one."""

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


class AlexLPIPSLoss(AlexLPIPS):
    """AlexLPIPS with `loss`: the reference's training term (perceptual_loss with its default net, train_ours.py:765).  Beside
    the score's parameters it packs the conv weights in the layouts the data gradients read (ebfi_lpips_alex_pack_grad_params)."""

    def __init__(self, conv_w, conv_b, lin_w, device):
        super().__init__(conv_w, conv_b, lin_w, device)
        h = N.lib()
        nbytes = h.ebfi_lpips_alex_grad_params_bytes()
        self.grad_params = torch.empty(nbytes // 4, dtype=torch.float32, device=self.device)
        ws = self._keep[0]
        with torch.cuda.device_of(self.grad_params):
            rc = h.ebfi_lpips_alex_pack_grad_params((N._vp * 5)(*[t.data_ptr() for t in ws]), N.ptr(self.grad_params), nbytes,
                                                    N.stream_ptr(self.device))
        N.check(rc, "ebfi_lpips_alex_pack_grad_params")
        self._train_pool = []

    def _train_workspace(self, stream, shape):
        """As VggLPIPS._train_workspace: one buffer per (stream, shape), a second only while two forwards await their backward,
        nothing allocated inside a capture."""
        return _take_train_workspace(self, stream, shape, N.lib().ebfi_lpips_alex_train_workspace,
                                     "LPIPS (AlexNet): ebfi_lpips_alex_forward_train")

    def _forward_train(self, pred, target, normalize, entry):
        n, c, hgt, wid = (int(v) for v in pred.shape)
        out = torch.empty(n, dtype=torch.float32, device=self.device)
        with torch.cuda.device_of(pred):
            rc = N.lib().ebfi_lpips_alex_forward_train(N.ptr(pred), N.i64x4(pred.stride()), N.ptr(target), N.i64x4(target.stride()),
                                                       n, c, hgt, wid, 1 if normalize else 0, N.ptr(self.params), N.ptr(entry.buf),
                                                       entry.buf.numel() * 8, N.ptr(out), None, N.stream_ptr(self.device))
        N.check(rc, "ebfi_lpips_alex_forward_train")
        return out

    def _backward(self, grad_out, shape, normalize, entry):
        n, c, hgt, wid = shape
        grad_out = grad_out.to(torch.float32).contiguous()
        grad_pred = torch.empty(shape, dtype=torch.float32, device=self.device)
        with torch.cuda.device_of(grad_pred):
            rc = N.lib().ebfi_lpips_alex_backward(N.ptr(grad_out), N.ptr(self.params), N.ptr(self.grad_params), N.ptr(entry.buf),
                                                  entry.buf.numel() * 8, n, c, hgt, wid, 1 if normalize else 0, N.ptr(grad_pred),
                                                  N.i64x4(grad_pred.stride()), N.stream_ptr(self.device))
        N.check(rc, "ebfi_lpips_alex_backward")
        return grad_pred

    def loss(self, pred, target, normalize=True):
        """lpips [N] of pred vs target as `__call__` returns it, bit for bit, with a graph: its backward is the gradient with
        respect to pred (ebfi_lpips_alex_backward).  The target gets none, and one that requires grad is refused."""
        if target.requires_grad:
            raise ValueError("AlexLPIPSLoss.loss has no gradient for the target: pass target.detach() (got a target that requires "
                             "grad)")
        N.require_gpu(pred, target)
        if pred.dim() != 4 or pred.shape != target.shape:
            raise ValueError("LPIPS takes two [N, C, H, W] tensors of one shape, got %s and %s"
                             % (tuple(pred.shape), tuple(target.shape)))
        if pred.dtype != torch.float32 or target.dtype != torch.float32:
            raise ValueError("LPIPS takes float32 tensors, got %s / %s" % (pred.dtype, target.dtype))
        if pred.device != self.device or target.device != self.device:
            raise ValueError("pred on %s, target on %s, weights on %s" % (pred.device, target.device, self.device))
        c, hgt, wid = (int(v) for v in pred.shape[1:])
        if c not in (1, 3):
            raise ValueError("LPIPS takes 1 or 3 channels, got %d (loss.perceptual_loss averages other counts per channel)" % c)
        if hgt < MIN_SIZE or wid < MIN_SIZE:
            raise ValueError("LPIPS (AlexNet) needs H, W >= %d, got %d x %d" % (MIN_SIZE, hgt, wid))
        pred = pred if pred.stride(3) == 1 else pred.contiguous()
        target = target if target.stride(3) == 1 else target.contiguous()
        if pred.shape[0] == 0:
            return pred.new_zeros(0) + 0.0 * pred.sum()
        return _TrainLoss.apply(pred, target, self, bool(normalize))


def load_alex_lpips(lin_path, backbone_path, device="cuda", net=NET, train=False):
    """AlexLPIPS from the reference's v0.1 heads (lin_path) and a torchvision AlexNet state dict (backbone_path); train=True:
    AlexLPIPSLoss, the same score with `loss`."""
    if net != NET:
        raise NotImplementedError("LPIPS net=%r is not implemented: only 'alex' has device kernels here (the reference also "
                                  "offers 'vgg' and 'squeeze')" % (net,))
    return (AlexLPIPSLoss if train else AlexLPIPS)(*read_alex_weights(lin_path, backbone_path), device)


# ------------------------------------------------------------------ the VGG-16 variant
VGG_CONV_KEYS = tuple("features.%d" % i for i in (0, 2, 5, 7, 10, 12, 14, 17, 19, 21, 24, 26, 28))
VGG_CHANNELS = (3, 64, 64, 128, 128, 256, 256, 256, 512, 512, 512, 512, 512, 512)
VGG_CONV_SHAPES = tuple((VGG_CHANNELS[i + 1], VGG_CHANNELS[i], 3, 3) for i in range(13))
VGG_HEAD_CHANNELS = (64, 128, 256, 512, 512)     # conv1_2, conv2_2, conv3_3, conv4_3, conv5_3
VGG_MIN_SIZE = 16                                # four floor-mode 2x2 pools must leave a pixel
VGG_WORKSPACE_BUDGET = 2 << 30                   # bytes: N is scored in chunks whose workspace stays under it


def read_vgg_weights(lin_path, backbone_path):
    """The 13 conv weights, 13 biases and 5 head vectors as CPU float32 tensors, from the reference's v0.1 vgg.pth and a
    torchvision VGG-16 state dict (classifier.* is ignored).  A missing or mis-shaped key raises, naming it."""
    lin = _state_dict(lin_path, "the LPIPS linear heads")
    trunk = _state_dict(backbone_path, "the VGG-16 trunk")
    ws = [_take(trunk, key + ".weight", shape, backbone_path) for key, shape in zip(VGG_CONV_KEYS, VGG_CONV_SHAPES)]
    bs = [_take(trunk, key + ".bias", shape[:1], backbone_path) for key, shape in zip(VGG_CONV_KEYS, VGG_CONV_SHAPES)]
    hs = [_take(lin, lkey, (1, c, 1, 1), lin_path).reshape(-1) for lkey, c in zip(LIN_KEYS, VGG_HEAD_CHANNELS)]
    return ws, bs, hs


class VggLPIPS:
    """LPIPS v0.1 with the VGG-16 trunk; parameters packed once on `device`.  The call contract of AlexLPIPS."""

    NET = "vgg"
    MIN_SIZE = VGG_MIN_SIZE

    def __init__(self, conv_w, conv_b, lin_w, device):
        self.device = torch.device(device)
        if self.device.type != "cuda":
            raise NotImplementedError("LPIPS runs on an MI355X through libebfi_hip.so only (got device %s)" % self.device)
        if self.device.index is None:
            self.device = torch.device("cuda", torch.cuda.current_device())
        if len(conv_w) != 13 or len(conv_b) != 13 or len(lin_w) != 5:
            raise ValueError("VggLPIPS takes 13 conv weights, 13 biases and 5 heads, got %d / %d / %d"
                             % (len(conv_w), len(conv_b), len(lin_w)))
        h = N.lib()
        ws = [w.to(self.device, torch.float32).contiguous() for w in conv_w]
        bs = [b.to(self.device, torch.float32).contiguous() for b in conv_b]
        hs = [v.to(self.device, torch.float32).contiguous() for v in lin_w]
        for got, want in zip(ws, VGG_CONV_SHAPES):
            if tuple(got.shape) != want:
                raise ValueError("VggLPIPS: a conv weight of shape %s, expected %s" % (tuple(got.shape), want))
        nbytes = h.ebfi_lpips_vgg_params_bytes()
        self.params = torch.empty(nbytes // 4, dtype=torch.float32, device=self.device)
        arr = lambda ts: (N._vp * len(ts))(*[t.data_ptr() for t in ts])   # noqa: E731
        with torch.cuda.device_of(self.params):
            rc = h.ebfi_lpips_vgg_pack_params(arr(ws), arr(bs), arr(hs), N.ptr(self.params), nbytes, N.stream_ptr(self.device))
        N.check(rc, "ebfi_lpips_vgg_pack_params")
        self._keep = (ws, bs, hs)      # (the pack kernels read them on the stream)
        self._workspaces = {}
        self._train_pool = []
        self.chunk = None              # pairs per call of the entry point; None: as many as VGG_WORKSPACE_BUDGET holds

    def _chunk(self, n, c, hgt, wid):
        """Pairs scored per call: every pair's result is independent of its neighbours, so the split changes no bit."""
        if self.chunk is not None:
            return max(1, int(self.chunk))
        per_pair = N.lib().ebfi_lpips_vgg_workspace(1, c, hgt, wid)
        return max(1, min(n, VGG_WORKSPACE_BUDGET // max(per_pair, 1)))

    def _workspace(self, stream, shape):
        key = (stream, shape)
        ws = self._workspaces.get(key)
        if ws is None:
            self._workspaces.clear()   # (keep only the latest shape)
            nbytes = N.lib().ebfi_lpips_vgg_workspace(*shape)
            if nbytes <= 0:
                raise ValueError("LPIPS (VGG-16): ebfi_lpips_vgg refuses the shape %s" % (shape,))
            ws = torch.empty(max(nbytes // 8, 1), dtype=torch.float64, device=self.device)
            self._workspaces[key] = ws
        return ws

    def _check(self, pred, target):
        """The pair as the entry points take it (unit column stride), or the error that names what is wrong with it."""
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
        if hgt < VGG_MIN_SIZE or wid < VGG_MIN_SIZE:
            raise ValueError("LPIPS (VGG-16) needs H, W >= %d, got %d x %d" % (VGG_MIN_SIZE, hgt, wid))
        pred = pred if pred.stride(3) == 1 else pred.contiguous()
        target = target if target.stride(3) == 1 else target.contiguous()
        return pred, target

    def _train_workspace(self, stream, shape):
        """A training workspace of (stream, shape) that no pending backward still reads.  One is enough for a loss evaluated once
        per step, and it is then the same buffer in every step; a second forward before the first one's backward --
        perceptual_loss's per-channel loop -- takes a second buffer.  Buffers of other shapes are dropped.  Inside a stream
        capture nothing should be allocated, and the capture runs on a stream of its own: it takes a free buffer of the shape
        whatever stream the eager passes before it left it on (every captured step here runs eagerly first).  A buffer that a
        captured graph replays on is kept for good and never handed to an eager call."""
        return _take_train_workspace(self, stream, shape, N.lib().ebfi_lpips_vgg_train_workspace,
                                     "LPIPS (VGG-16): ebfi_lpips_vgg_forward_train")

    def _forward_train(self, pred, target, normalize, entry):
        n, c, hgt, wid = (int(v) for v in pred.shape)
        out = torch.empty(n, dtype=torch.float32, device=self.device)
        with torch.cuda.device_of(pred):
            rc = N.lib().ebfi_lpips_vgg_forward_train(N.ptr(pred), N.i64x4(pred.stride()), N.ptr(target), N.i64x4(target.stride()), n,
                                                      c, hgt, wid, 1 if normalize else 0, N.ptr(self.params), N.ptr(entry.buf),
                                                      entry.buf.numel() * 8, N.ptr(out), None, N.stream_ptr(self.device))
        N.check(rc, "ebfi_lpips_vgg_forward_train")
        return out

    def _backward(self, grad_out, shape, normalize, entry):
        n, c, hgt, wid = shape
        grad_out = grad_out.to(torch.float32).contiguous()
        grad_pred = torch.empty(shape, dtype=torch.float32, device=self.device)
        with torch.cuda.device_of(grad_pred):
            rc = N.lib().ebfi_lpips_vgg_backward(N.ptr(grad_out), N.ptr(self.params), N.ptr(entry.buf), entry.buf.numel() * 8, n, c,
                                                 hgt, wid, 1 if normalize else 0, N.ptr(grad_pred), N.i64x4(grad_pred.stride()),
                                                 N.stream_ptr(self.device))
        N.check(rc, "ebfi_lpips_vgg_backward")
        return grad_pred

    def loss(self, pred, target, normalize=True):
        """lpips [N] of pred vs target as `__call__` returns it, bit for bit, with a graph: its backward is the gradient with
        respect to pred (ebfi_lpips_vgg_backward: the tap adjoints and the 13 data gradients on the device).  The target gets
        none, and one that requires grad is refused.  All pairs go through one call: the workspace (ebfi_lpips_vgg_train_workspace)
        keeps the 13 ReLU maps of the pred images."""
        if target.requires_grad:
            raise ValueError("VggLPIPS.loss has no gradient for the target: pass target.detach() (got a target that requires grad)")
        pred, target = self._check(pred, target)
        if pred.shape[0] == 0:
            return pred.new_zeros(0) + 0.0 * pred.sum()
        return _TrainLoss.apply(pred, target, self, bool(normalize))

    @torch.no_grad()
    def __call__(self, pred, target, normalize=True, per_layer=False):
        """lpips [N] (float32, on the device) of pred vs target [N, C, H, W], C in {1, 3}: normalize=True takes [0, 1]
        images, False [-1, 1] ones.  per_layer=True also returns the [N, 5] layer terms.  Strided views with unit column
        stride are read in place."""
        pred, target = self._check(pred, target)
        n, c, hgt, wid = (int(v) for v in pred.shape)
        out = torch.empty(n, dtype=torch.float32, device=self.device)
        layers = torch.empty(n, 5, dtype=torch.float32, device=self.device) if per_layer else None
        if n:
            step = self._chunk(n, c, hgt, wid)
            with torch.cuda.device_of(pred):
                stream = N.stream_ptr(self.device)
                ws = self._workspace(stream.value, (min(step, n), c, hgt, wid))
                for i in range(0, n, step):
                    m = min(step, n - i)
                    p, t = pred[i:i + m], target[i:i + m]
                    rc = N.lib().ebfi_lpips_vgg(N.ptr(p), N.i64x4(p.stride()), N.ptr(t), N.i64x4(t.stride()), m, c, hgt, wid,
                                                1 if normalize else 0, N.ptr(self.params), N.ptr(ws), ws.numel() * 8,
                                                N.ptr(out[i:i + m]), N.ptr(layers[i:i + m]) if per_layer else None, stream)
                    N.check(rc, "ebfi_lpips_vgg")
        return (out, layers) if per_layer else out


def _take_train_workspace(model, stream, shape, size_of, what):
    """The pool rule of `model._train_pool` (VggLPIPS._train_workspace states it); `size_of(*shape)` is the entry point's size."""
    capturing = torch.cuda.is_current_stream_capturing()
    model._train_pool = [e for e in model._train_pool if e.shape == shape or e.captured]
    for entry in model._train_pool:
        if entry.shape == shape and entry.free() and (capturing or (entry.stream == stream and not entry.captured)):
            entry.captured = entry.captured or capturing
            return entry
    nbytes = size_of(*shape)
    if nbytes <= 0:
        raise ValueError("%s refuses the shape %s" % (what, shape))
    buf = torch.empty(max(nbytes // 8, 1), dtype=torch.float64, device=model.device)
    entry = _TrainWorkspace(buf, stream, shape, capturing)
    model._train_pool.append(entry)
    return entry


class _TrainWorkspace:
    """A training workspace and who reads it: the forward that filled it claims it until its backward has run (or its graph
    node has been dropped without one)."""

    class _Claim:
        __slots__ = ("__weakref__",)

    def __init__(self, buf, stream, shape, captured):
        self.buf, self.stream, self.shape, self.captured = buf, stream, shape, captured
        self._owner, self.generation = None, 0

    def free(self):
        return self._owner is None or self._owner() is None

    def claim(self):
        token = self._Claim()
        self._owner = weakref.ref(token)
        self.generation += 1
        return token, self.generation

    def release(self):
        self._owner = None


class _TrainLoss(torch.autograd.Function):
    """lpips [N] of VggLPIPS.loss / AlexLPIPSLoss.loss: the model's forward_train and backward around one workspace."""

    @staticmethod
    def forward(ctx, pred, target, model, normalize):
        entry = model._train_workspace(N.stream_ptr(model.device).value, tuple(int(v) for v in pred.shape))
        out = model._forward_train(pred, target, normalize, entry)
        ctx.model, ctx.normalize, ctx.entry, ctx.shape = model, normalize, entry, tuple(int(v) for v in pred.shape)
        ctx.claim, ctx.generation = entry.claim()
        return out

    @staticmethod
    def backward(ctx, grad_out):
        if ctx.entry.generation != ctx.generation:
            raise RuntimeError("%s.loss: a later forward has overwritten the workspace of this one (its backward had "
                               "already run once)" % type(ctx.model).__name__)
        grad_pred = ctx.model._backward(grad_out, ctx.shape, ctx.normalize, ctx.entry)
        ctx.entry.release()
        return grad_pred, None, None, None


def load_vgg_lpips(lin_path, backbone_path, device="cuda"):
    """VggLPIPS from the reference's v0.1 heads (lin_path: vgg.pth) and a torchvision VGG-16 state dict (backbone_path)."""
    return VggLPIPS(*read_vgg_weights(lin_path, backbone_path), device)


NETS = ("alex", "vgg")


def load_lpips(net, lin_path, backbone_path, device="cuda", train=False):
    """The LPIPS model of `net`: 'alex' or 'vgg'.  'squeeze', the reference's third choice, has no device kernels here.
    train=True makes 'alex' an AlexLPIPSLoss (with `loss`); VggLPIPS has its `loss` either way."""
    if net == "alex":
        return load_alex_lpips(lin_path, backbone_path, device=device, **({"train": True} if train else {}))
    if net == "vgg":
        return load_vgg_lpips(lin_path, backbone_path, device=device)
    raise NotImplementedError("LPIPS net=%r is not implemented: 'alex' and 'vgg' have device kernels here (the reference also "
                              "offers 'squeeze')" % (net,))
