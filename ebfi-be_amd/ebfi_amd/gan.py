"""The STGAN adversarial loss: 'GAN': Adversarial(PatchSize, gan_type='STGAN') of the reference's loss dictionary
(train_ours.py:757-767, loss/adversarial.py, loss/discriminator.py:208-263) on the device.

The law is written out in include/ebfi_hip.h (section "STGAN adversarial loss") and restated in float64 by tests/stgan_ref.py.
`ST_Discriminator` keeps torch modules as PARAMETER CONTAINERS only -- their names, shapes and default initialisation are the
reference's, so state dicts interchange -- and computes by hand: the sixteen 3x3 convolutions call the exact-fp32 entry points
of csrc/conv2d.hip directly (never ebfi_amd.conv: the discriminator sees neither the process-wide compute mode, the weight
bank, the fp16 scale book, the deferred weight-gradient queue nor the overflow guard, all of which are active around it inside
a training step), and everything between them is csrc/stgan.hip -- the classifier's two linear layers too: skinny products
with fixed-order sums, so that a captured step replays the bits of an eager one (the BLAS behind F.linear did not).  There is no
autograd inside: the discriminator's step writes its parameter gradients into two flat buffers (one per pass) that ONE Adamax
launch reads, and the generator's pass is a single autograd node with a gradient into `fake` only.  Everything is launched on
the current stream without a host read, so a call can be captured into a hipGraph.
"""
import torch
import torch.nn as nn
from torch.autograd import Function

from . import _native as N

SLOPE, BN_EPS, BN_MOMENTUM = 0.2, 1e-5, 0.1
# (ci, co, stride) of a branch's eight blocks; None = the branch's input channels
BRANCH = ((None, 8, 1), (8, 8, 2), (8, 16, 1), (16, 16, 2), (16, 32, 1), (32, 32, 2), (32, 64, 1), (64, 64, 2))
GAN_TYPES = ("STGAN",)


def _block(ci, co, stride):
    return nn.Sequential(nn.Conv2d(ci, co, 3, stride=stride, padding=1, bias=False), nn.BatchNorm2d(co, eps=BN_EPS, momentum=BN_MOMENTUM),
                         nn.LeakyReLU(SLOPE, inplace=True))


def _branch(c):
    return nn.Sequential(*[_block(c if ci is None else ci, co, s) for ci, co, s in BRANCH])


def check_patch(P):
    if int(P) != P or P < 16 or P % 16:
        raise ValueError("ST_Discriminator: PatchSize must be a positive multiple of 16 (four stride-2 stages and a "
                         "Linear(128 (P/16)^2, 1024)), got %r" % (P,))
    return int(P)


class ST_Discriminator(nn.Module):
    """D(f0, f1, f2) -> [B, 1] logits; always in training mode (batch statistics), as the reference uses it."""

    def __init__(self, PatchSize):
        super().__init__()
        self.patch = check_patch(PatchSize)
        self.s_features = _branch(3)
        self.t_features = _branch(6)
        q = self.patch // 16
        self.classifier = nn.Sequential(nn.Linear(128 * q * q, 1024), nn.LeakyReLU(SLOPE, inplace=True), nn.Linear(1024, 1))
        self._ws = None
        self._views = {}
        self._flatten()

    # ------------------------------------------------------------------------------------------------ storage
    def _flatten(self):
        """Re-points every parameter at a view of ONE flat buffer (values, names and shapes unchanged), in parameters()
        order -- torch.optim.Adamax's: the update is one launch, the gradients are written into buffers of the same layout.
        Every offset is a multiple of four elements (all parameter sizes are, but the last bias)."""
        params = list(self.parameters())
        with torch.no_grad():
            flat = torch.cat([p.data.reshape(-1) for p in params])
        self._offsets, off = [], 0
        for p in params:
            self._offsets.append(off)
            p.data = flat[off:off + p.numel()].view_as(p)
            off += p.numel()
        self.__dict__["flat"] = flat
        self._index = {id(p): i for i, p in enumerate(params)}
        self._views = {}
        self._ws = None

    def _apply(self, fn, *args, **kwargs):
        out = super()._apply(fn, *args, **kwargs)
        self._flatten()                             # (a device or dtype move gave every parameter a tensor of its own)
        return out

    def views_intact(self):
        base = self.flat.untyped_storage().data_ptr()
        return all(p.untyped_storage().data_ptr() == base for p in self.parameters())

    def train(self, mode=True):
        if not mode:
            raise RuntimeError("ST_Discriminator has no evaluation mode: the reference never normalises by the running statistics "
                               "(they are kept, and saved, as a by-product of the training passes)")
        return super().train(True)

    def grad_views(self, flat_grad):
        """Per-parameter views of a flat gradient buffer of this layout (cached per buffer)."""
        key = flat_grad.data_ptr()
        v = self._views.get(key)
        if v is None:
            if flat_grad.numel() != self.flat.numel():
                raise ValueError("gradient buffer has %d elements, the discriminator %d" % (flat_grad.numel(), self.flat.numel()))
            v = self._views[key] = [flat_grad[o:o + p.numel()].view_as(p) for o, p in zip(self._offsets, self.parameters())]
        return v

    def _workspace(self, nbytes):
        if self._ws is None or self._ws.numel() * 8 < nbytes or self._ws.device != self.flat.device:
            self._ws = torch.empty(max(int(nbytes) + 7, 16) // 8, dtype=torch.float64, device=self.flat.device)
        return self._ws

    # ------------------------------------------------------------------------------------------------ checks (host only)
    def check_inputs(self, f0, f1, f2):
        P = self.patch
        for name, t in (("f0", f0), ("f1", f1), ("f2", f2)):
            if t.dim() != 4 or t.shape[1] != 3 or t.shape[2] != P or t.shape[3] != P or t.shape[0] != f1.shape[0]:
                raise ValueError("ST_Discriminator(PatchSize=%d): %s must be [B, 3, %d, %d], got %r (H == W == PatchSize: the "
                                 "classifier is a Linear on the flattened features)" % (P, name, P, P, tuple(t.shape)))
        if f1.shape[0] * (P // 16) ** 2 < 2:
            raise ValueError("ST_Discriminator: batch statistics need more than 1 value per channel; the last stage has B * (P/16)^2 "
                             "= 1 (torch refuses it too)")
        N.require_gpu(f0, f1, f2, self.flat)
        for t in (f0, f1, f2):
            if t.dtype != torch.float32:
                raise N.EbfiNativeError("ST_Discriminator takes float32 tensors, got %s" % t.dtype)

    # ------------------------------------------------------------------------------------------------ native pieces
    def _conv_forward(self, x, w, stride, st):
        B, Cin, H, W = (int(v) for v in x.shape)
        Ho, Wo = (H - 1) // stride + 1, (W - 1) // stride + 1
        out = torch.empty((B, int(w.shape[0]), Ho, Wo), dtype=torch.float32, device=x.device)
        rc = N.lib().ebfi_conv2d_forward(N.ptr(x), N.ptr(w), N.ptr(None), N.ptr(out), B, Cin, H, W, int(w.shape[0]), 3, stride, 1, 0, 0.0,
                                         N.EBFI_F32, st)
        N.check(rc, "ebfi_conv2d_forward (discriminator)")
        return out

    def _conv_weight_grad(self, x, gz, gw, stride, st):
        B, Cin, H, W = (int(v) for v in x.shape)
        geo = (B, Cin, H, W, int(gz.shape[1]), 3, stride, 1)
        lib = N.lib()
        need = int(lib.ebfi_conv2d_backward_weight_workspace(*geo, N.EBFI_F32))
        ws = self._workspace(need)
        rc = lib.ebfi_conv2d_backward_weight(N.ptr(x), N.ptr(gz), N.ptr(None), N.ptr(gw), N.ptr(None), *geo, 0, 0.0, N.ptr(ws), need,
                                             N.EBFI_F32, st)
        N.check(rc, "ebfi_conv2d_backward_weight (discriminator)")

    def _conv_data_grad(self, gz, w, x_shape, stride, st):
        B, Cin, H, W = (int(v) for v in x_shape)
        Cout = int(w.shape[0])
        if stride == 2:
            # zero insertion, as ebfi_amd.conv.ConvBiasAct: the stride-1 data gradient of the gradient spread over the even pixels
            up = gz.new_zeros((B, Cout, H, W))
            up[:, :, ::2, ::2] = gz
            gz = up
        gx = torch.empty((B, Cin, H, W), dtype=torch.float32, device=gz.device)
        rc = N.lib().ebfi_conv2d_backward_data(N.ptr(gz), N.ptr(None), N.ptr(w), N.ptr(gx), B, Cin, H, W, Cout, 3, 1, 1, 0, 0.0,
                                               N.EBFI_F32, st)
        N.check(rc, "ebfi_conv2d_backward_data (discriminator)")
        return gx

    def _bn_forward(self, z, bn, st):
        B, C, H, W = (int(v) for v in z.shape)
        lib = N.lib()
        y = torch.empty_like(z)
        stats = torch.empty((C, 2), dtype=torch.float64, device=z.device)
        need = int(lib.ebfi_bn_lrelu_workspace(B, C, H * W))
        ws = self._workspace(need)
        rc = lib.ebfi_bn_lrelu_forward(N.ptr(z), N.ptr(bn.weight), N.ptr(bn.bias), N.ptr(y), N.ptr(stats), N.ptr(bn.running_mean),
                                       N.ptr(bn.running_var), N.ptr(bn.num_batches_tracked), B, C, H * W, BN_EPS, BN_MOMENTUM, SLOPE,
                                       N.ptr(ws), need, st)
        N.check(rc, "ebfi_bn_lrelu_forward")
        return y, stats

    def _bn_backward(self, gy, z, y, bn, stats, ggamma, gbeta, st):
        B, C, H, W = (int(v) for v in z.shape)
        lib = N.lib()
        gz = torch.empty_like(z)
        need = int(lib.ebfi_bn_lrelu_workspace(B, C, H * W))
        ws = self._workspace(need)
        rc = lib.ebfi_bn_lrelu_backward(N.ptr(gy), N.ptr(z), N.ptr(y), N.ptr(bn.weight), N.ptr(stats), N.ptr(gz), N.ptr(ggamma),
                                        N.ptr(gbeta), B, C, H * W, SLOPE, N.ptr(ws), need, st)
        N.check(rc, "ebfi_bn_lrelu_backward")
        return gz

    def _linear_forward(self, x, lin, act, st):
        B, K = (int(v) for v in x.shape)
        y = torch.empty((B, int(lin.weight.shape[0])), dtype=torch.float32, device=x.device)
        rc = N.lib().ebfi_linear_forward(N.ptr(x), N.ptr(lin.weight), N.ptr(lin.bias), N.ptr(y), B, K, int(lin.weight.shape[0]),
                                         1 if act else 0, SLOPE, st)
        N.check(rc, "ebfi_linear_forward")
        return y

    def _linear_backward_data(self, gy, lin, mask, st):
        B, n_out = (int(v) for v in gy.shape)
        K = int(lin.weight.shape[1])
        gx = torch.empty((B, K), dtype=torch.float32, device=gy.device)
        rc = N.lib().ebfi_linear_backward_data(N.ptr(gy), N.ptr(lin.weight), N.ptr(mask), SLOPE, N.ptr(gx), B, K, n_out, st)
        N.check(rc, "ebfi_linear_backward_data")
        return gx

    def _linear_backward_weight(self, gy, x, gw, gb, st):
        B, n_out = (int(v) for v in gy.shape)
        rc = N.lib().ebfi_linear_backward_weight(N.ptr(gy), N.ptr(x), N.ptr(gw), N.ptr(gb), B, int(x.shape[1]), n_out, st)
        N.check(rc, "ebfi_linear_backward_weight")

    def _branch_forward(self, seq, x, st):
        saved = []
        for blk in seq:
            z = self._conv_forward(x, blk[0].weight, int(blk[0].stride[0]), st)
            y, stats = self._bn_forward(z, blk[1], st)
            saved.append((x, z, y, stats))
            x = y
        return saved, x

    def _branch_backward(self, seq, saved, gy, views, need_x, st):
        for k in range(len(seq) - 1, -1, -1):
            conv, bn = seq[k][0], seq[k][1]
            x, z, y, stats = saved[k]
            gg = gb = None
            if views is not None:
                gg, gb = views[self._index[id(bn.weight)]], views[self._index[id(bn.bias)]]
            gz = self._bn_backward(gy, z, y, bn, stats, gg, gb, st)
            if views is not None:
                self._conv_weight_grad(x, gz, views[self._index[id(conv.weight)]], int(conv.stride[0]), st)
            if k == 0 and not need_x:
                return None
            gy = self._conv_data_grad(gz, conv.weight, x.shape, int(conv.stride[0]), st)
        return gy

    # ------------------------------------------------------------------------------------------------ passes
    @torch.no_grad()
    def forward_saved(self, f0, f1, f2):
        """-> (logits [B, 1], what `backward` needs).  Updates the running statistics of all sixteen BatchNorm layers."""
        self.check_inputs(f0, f1, f2)
        B, P = int(f1.shape[0]), self.patch
        chw = 3 * P * P
        per_sample = lambda t: t if t.stride()[1:] == (P * P, P, 1) and t.stride(0) >= chw else t.contiguous()
        f0, f1, f2 = per_sample(f0), f1.contiguous(), per_sample(f2)
        with torch.cuda.device_of(f1):
            st = N.stream_ptr(f1.device)
            t_in = torch.empty((B, 6, P, P), dtype=torch.float32, device=f1.device)
            rc = N.lib().ebfi_stgan_temporal_forward(N.ptr(f0), int(f0.stride(0)), N.ptr(f1), int(f1.stride(0)), N.ptr(f2),
                                                     int(f2.stride(0)), N.ptr(t_in), B, chw, st)
            N.check(rc, "ebfi_stgan_temporal_forward")
            s_saved, s_out = self._branch_forward(self.s_features, f1, st)
            t_saved, t_out = self._branch_forward(self.t_features, t_in, st)
            feat = torch.cat([s_out.reshape(B, -1), t_out.reshape(B, -1)], 1)
            l1, l2 = self.classifier[0], self.classifier[2]
            h = self._linear_forward(feat, l1, True, st)
            d = self._linear_forward(h, l2, False, st)
        return d, (s_saved, t_saved, feat, h)

    def forward(self, f0, f1, f2):
        return self.forward_saved(f0, f1, f2)[0]

    @torch.no_grad()
    def backward(self, saved, gd, flat_grad=None):
        """gd [B, 1]: the gradient of the logits.  flat_grad given: every parameter's gradient is WRITTEN into that flat buffer
        (the discriminator's step; nothing flows into the images) -> None.  flat_grad None: the data gradient alone (the
        generator's pass: no parameter gradient is computed) -> the gradient of f1 [B, 3, P, P]."""
        s_saved, t_saved, feat, h = saved
        B, P = int(feat.shape[0]), self.patch
        q = P // 16
        l1, l2 = self.classifier[0], self.classifier[2]
        views = None if flat_grad is None else self.grad_views(flat_grad)
        with torch.cuda.device_of(feat):
            st = N.stream_ptr(feat.device)
            gd = gd.contiguous()
            ghp = self._linear_backward_data(gd, l2, h, st)            # (times LeakyReLU'(h): the hidden layer's pre-activation gradient)
            if views is not None:
                ix = self._index
                self._linear_backward_weight(gd, h, views[ix[id(l2.weight)]], views[ix[id(l2.bias)]], st)
                self._linear_backward_weight(ghp, feat, views[ix[id(l1.weight)]], views[ix[id(l1.bias)]], st)
            gfeat = self._linear_backward_data(ghp, l1, None, st)
            half = 64 * q * q
            gs = gfeat[:, :half].reshape(B, 64, q, q).contiguous()
            gt = gfeat[:, half:].reshape(B, 64, q, q).contiguous()
            need_x = views is None
            gs_in = self._branch_backward(self.s_features, s_saved, gs, views, need_x, st)
            gt_in = self._branch_backward(self.t_features, t_saved, gt, views, need_x, st)
            if not need_x:
                return None
            gf1 = torch.empty((B, 3, P, P), dtype=torch.float32, device=feat.device)
            rc = N.lib().ebfi_stgan_temporal_backward(N.ptr(gt_in), N.ptr(gs_in), N.ptr(gf1), B, 3 * P * P, st)
            N.check(rc, "ebfi_stgan_temporal_backward")
        return gf1


def bce_logits_pair(fake, real, want_grad=True, out=None):
    """mean softplus(fake) + mean softplus(-real) of two [B, 1] logit tensors (either may be None) as a 0-dim device tensor, and
    the gradients (None where not asked / not there): ebfi_bce_logits_pair."""
    ref = fake if fake is not None else real
    N.require_gpu(ref)
    n = int(ref.numel())
    loss = out if out is not None else torch.empty((), dtype=torch.float32, device=ref.device)
    gf = torch.empty_like(fake) if (fake is not None and want_grad) else None
    gr = torch.empty_like(real) if (real is not None and want_grad) else None
    with torch.cuda.device_of(ref):
        rc = N.lib().ebfi_bce_logits_pair(N.ptr(fake), N.ptr(real), n, N.ptr(loss), N.ptr(gf), N.ptr(gr), N.stream_ptr(ref.device))
    N.check(rc, "ebfi_bce_logits_pair")
    return loss, gf, gr


class FlatAdamax:
    """torch.optim.Adamax over the discriminator's flat parameter buffer: ONE native launch (csrc/stgan.hip, ebfi_adamax_step),
    the step count a device word, hyper-parameters by value -- read from `inner.param_groups` at every step, so what an LR
    scheduler wrote reaches the next eager launch (inside a captured step the value is part of the graph: the engine keys its
    graphs by it).  `inner` is torch.optim.Adamax([flat]): it owns hyper-parameters and state and is what a scheduler wraps.
    state_dict() / load_state_dict() speak torch's per-parameter layout (step, exp_avg, exp_inf per parameter), so the states
    interchange with a torch.optim.Adamax over the reference's discriminator.  CPU tensors take torch's own step."""

    def __init__(self, disc, lr=1e-3, betas=(0.9, 0.999), eps=1e-8, weight_decay=0.0):
        self.disc = disc
        self.flat = nn.Parameter(disc.flat)
        self.inner = torch.optim.Adamax([self.flat], lr=lr, betas=tuple(betas), eps=eps, weight_decay=weight_decay, foreach=False)

    @property
    def param_groups(self):
        return self.inner.param_groups

    def rebind(self):
        """After the discriminator moved (its flat buffer is a new tensor): the state follows."""
        old, new = self.flat, nn.Parameter(self.disc.flat)
        st = self.inner.state.pop(old, None)
        self.inner.param_groups[0]["params"] = [new]
        if st:
            self.inner.state[new] = {k: (v.to(new.device) if torch.is_tensor(v) else v) for k, v in st.items()}
        self.flat = new

    def _state(self):
        st = self.inner.state[self.flat]
        if "step" not in st:
            st["step"] = torch.zeros((), dtype=torch.float32, device=self.flat.device)
            st["exp_avg"] = torch.zeros_like(self.flat.data)
            st["exp_inf"] = torch.zeros_like(self.flat.data)
        return st

    def zero_grad(self, set_to_none=True):
        """The gradients are written from zero by every call of Adversarial; nothing is kept between calls."""

    def step(self, grad, grad2=None):
        """grad (+ grad2): flat gradient buffer(s) of the discriminator's layout; their sum is the gradient."""
        grp = self.inner.param_groups[0]
        if grp.get("maximize"):
            raise NotImplementedError("FlatAdamax: maximize is not implemented")
        if not self.flat.is_cuda:
            self.flat.grad = grad if grad2 is None else grad + grad2
            self.inner.step()
            self.flat.grad = None
            return
        st = self._state()
        st["step"] += 1
        b1, b2 = grp["betas"]
        with torch.cuda.device_of(self.flat):
            rc = N.lib().ebfi_adamax_step(N.ptr(self.flat.data), N.ptr(grad), N.ptr(grad2), N.ptr(st["exp_avg"]), N.ptr(st["exp_inf"]),
                                          N.ptr(st["step"]), self.flat.numel(), float(grp["lr"]), float(b1), float(b2), float(grp["eps"]),
                                          float(grp["weight_decay"]), N.stream_ptr(self.flat.device))
        N.check(rc, "ebfi_adamax_step")
        self.inner._opt_called = True                       # (what the LR schedulers look at, as ebfi_amd.dp.FlatOptimizer)
        if hasattr(self.inner, "_step_count"):
            self.inner._step_count += 1

    def _slices(self):
        return [(i, p, slice(o, o + p.numel())) for i, (p, o) in enumerate(zip(self.disc.parameters(), self.disc._offsets))]

    _LOCAL_KEYS = ("params", "foreach", "capturable", "differentiable", "maximize")

    def state_dict(self):
        st = self.inner.state.get(self.flat, {})
        state = {}
        if st:
            for i, p, sl in self._slices():
                state[i] = {"step": st["step"].clone(), "exp_avg": st["exp_avg"][sl].view_as(p).clone(),
                            "exp_inf": st["exp_inf"][sl].view_as(p).clone()}
        group = {k: v for k, v in self.inner.param_groups[0].items() if k != "params"}
        group["params"] = list(range(len(self.disc._offsets)))
        return {"state": state, "param_groups": [group]}

    def load_state_dict(self, sd):
        groups = sd["param_groups"]
        if len(groups) != 1 or len(groups[0]["params"]) != len(self.disc._offsets):
            raise ValueError("Adamax state has %d parameters in %d group(s), the discriminator %d"
                             % (sum(len(g["params"]) for g in groups), len(groups), len(self.disc._offsets)))
        grp = self.inner.param_groups[0]
        for k, v in groups[0].items():
            if k not in self._LOCAL_KEYS and k in grp:
                grp[k] = v
        if not sd["state"]:
            self.inner.state.pop(self.flat, None)
            return
        bufs = {k: torch.zeros_like(self.flat.data) for k in ("exp_avg", "exp_inf")}
        step = None
        for pid, (_, p, sl) in zip(groups[0]["params"], self._slices()):
            e = sd["state"].get(pid)
            if e is None:
                continue
            for k in bufs:
                bufs[k][sl] = e[k].reshape(-1).to(bufs[k])
            if step is not None and float(e["step"]) != step:
                raise ValueError("Adamax state holds different step counts per parameter (%g and %g): the flat update keeps one "
                                 "counter" % (step, float(e["step"])))
            step = float(e["step"])
        self.inner.state[self.flat] = dict(bufs, step=torch.tensor(step or 0.0, dtype=torch.float32, device=self.flat.device))


class _GeneratorPass(Function):
    """loss_g = mean softplus(-D(f0, fake, f2)) as ONE node with a gradient into `fake` only."""

    @staticmethod
    def forward(ctx, fake, adv, f0, f2):
        d_g, saved = adv.discriminator.forward_saved(f0, fake, f2)
        loss_g, _, g_unit = bce_logits_pair(None, d_g)
        ctx.adv, ctx.saved, ctx.g_unit = adv, saved, g_unit
        return loss_g

    @staticmethod
    def backward(ctx, g):
        saved, ctx.saved = ctx.saved, None
        return ctx.adv.discriminator.backward(saved, ctx.g_unit * g), None, None, None


class Adversarial(nn.Module):
    """Adversarial(PatchSize, gan_type='STGAN'): forward(fake, real, input_frames) takes the discriminator's Adamax step on
    (fake.detach(), real) and returns the generator's loss under the updated weights, with a graph into `fake`.
    `loss_d` is the discriminator's loss of the last call as a 0-dim DEVICE tensor; `loss` reads it on demand (the reference
    keeps a Python float, a host read per call)."""

    def __init__(self, PatchSize, gan_type="STGAN"):
        if gan_type not in GAN_TYPES:
            raise NotImplementedError("Adversarial: gan_type %r is not implemented here (only 'STGAN', what the reference's "
                                      "trainer builds)" % (gan_type,))
        super().__init__()
        self.gan_type, self.gan_k = gan_type, 1
        self.discriminator = ST_Discriminator(PatchSize)
        self.optimizer = FlatAdamax(self.discriminator, lr=1e-3, betas=(0.9, 0.999), eps=1e-8, weight_decay=0.0)
        # (built as the reference builds it; nobody steps it there either)
        self.scheduler = torch.optim.lr_scheduler.ReduceLROnPlateau(self.optimizer.inner, mode="max", factor=0.5, patience=5,
                                                                    threshold=0.01, threshold_mode="abs")
        self.register_buffer("loss_d", torch.zeros(()), persistent=False)
        self._grads = None

    def _apply(self, fn, *args, **kwargs):
        out = super()._apply(fn, *args, **kwargs)
        self.optimizer.rebind()
        self._grads = None
        return out

    @property
    def loss(self):
        return float(self.loss_d)

    @property
    def lr(self):
        return float(self.optimizer.param_groups[0]["lr"])

    def forward(self, fake, real, input_frames=None):
        D = self.discriminator
        if input_frames is None or input_frames.dim() != 5 or input_frames.shape[1] != 2:
            raise ValueError("Adversarial(STGAN): input_frames must be the neighbours [B, 2, 3, H, W], got %r"
                             % (None if input_frames is None else tuple(input_frames.shape),))
        f0, f2 = input_frames[:, 0], input_frames[:, 1]
        D.check_inputs(f0, fake, f2)
        D.check_inputs(f0, real, f2)
        if self._grads is None or self._grads[0].device != D.flat.device:
            self._grads = (torch.empty_like(D.flat), torch.empty_like(D.flat))
        with torch.no_grad():
            self.optimizer.zero_grad()
            d_fake, sv_fake = D.forward_saved(f0, fake.detach(), f2)
            d_real, sv_real = D.forward_saved(f0, real.detach(), f2)
            _, g_fake, g_real = bce_logits_pair(d_fake, d_real, out=self.loss_d)
            D.backward(sv_fake, g_fake, self._grads[0])
            D.backward(sv_real, g_real, self._grads[1])
            del sv_fake, sv_real
            self.optimizer.step(self._grads[0], self._grads[1])
        return _GeneratorPass.apply(fake, self, f0.detach(), f2.detach())

    # ------------------------------------------------------------------------------------------------ state around a capture
    def _state_tensors(self):
        st = self.optimizer._state()
        return [self.discriminator.flat, st["step"], st["exp_avg"], st["exp_inf"], self.loss_d] + list(self.discriminator.buffers())

    def snapshot(self):
        """Copies of everything a call changes (weights, Adamax state, running statistics): a hipGraph capture runs warm-up
        passes, each a discriminator step, that must not count."""
        return [t.clone() for t in self._state_tensors()]

    @torch.no_grad()
    def restore(self, snap):
        for t, s in zip(self._state_tensors(), snap):
            t.copy_(s)

    # ------------------------------------------------------------------------------------------------ checkpoint entry
    def checkpoint_state(self):
        """The `gan` entry of a checkpoint: the discriminator's states plus the Adamax states in torch's per-parameter layout."""
        return {"type": self.gan_type, "patch": self.discriminator.patch,
                "discriminator": {k: v.detach().clone() for k, v in self.discriminator.state_dict().items()},
                "optimizer": self.optimizer.state_dict()}

    def load_checkpoint_state(self, state):
        if state.get("patch") != self.discriminator.patch:
            raise ValueError("checkpoint gan.patch = %r, this run's crop is %d (the classifier's input depends on it)"
                             % (state.get("patch"), self.discriminator.patch))
        self.discriminator.load_state_dict(state["discriminator"])
        self.optimizer.load_state_dict(state["optimizer"])


class AdversarialTerm:
    """weight * loss_g as a term of the training loss, beside Lap, census and LPIPS (train_ours.py:757-767); mirrors
    ebfi_amd.loss.PerceptualTerm.  term(fake, real, neighbours [B, 2, 3, H, W]) -> 0-dim tensor with a graph into fake; the call
    also takes the discriminator's step.  The discriminator is no part of the trained model: it has its own optimiser and its
    own checkpoint entry."""

    def __init__(self, adversarial, weight):
        if not isinstance(adversarial, Adversarial):
            raise TypeError("AdversarialTerm needs an ebfi_amd.gan.Adversarial, got %s" % type(adversarial).__name__)
        if not float(weight) > 0:
            raise ValueError("AdversarialTerm: the weight must be positive, got %r (leave the term out instead)" % (weight,))
        self.adversarial, self.weight = adversarial, float(weight)

    def __call__(self, fake, real, neighbours):
        return self.weight * self.adversarial(fake, real.detach(), neighbours)
