"""Float64 restatement of the STGAN adversarial loss, written from the law in include/ebfi_hip.h (section "STGAN adversarial
loss"), not from the reference's file: plain tensors under their state-dict names, torch's conv2d / matmul and autograd for the
derivatives, BatchNorm, LeakyReLU, BCE with logits and Adamax spelled out.  `dtype=torch.float32` runs the same operations in
float32: the yardstick the GPU tests measure the native path against.

  names_and_shapes(P)            the 100 state-dict entries of Adversarial(P, 'STGAN'), in order
  fill_state(seed, P)            every parameter from numpy.random.RandomState(seed); buffers at their defaults
  RefAdversarial(P, state)       .call(fake, real, frames) -> (loss_d, loss_g, grad_fake); updates weights, Adamax state and
                                 running statistics in place, as Adversarial.forward does
"""
import numpy as np
import torch
import torch.nn.functional as F

SLOPE, EPS, MOMENTUM = 0.2, 1e-5, 0.1
LR, BETA1, BETA2, ADAMAX_EPS = 1e-3, 0.9, 0.999, 1e-8
BRANCH = ((None, 8, 1), (8, 8, 2), (8, 16, 1), (16, 16, 2), (16, 32, 1), (32, 32, 2), (32, 64, 1), (64, 64, 2))
PREFIX = "discriminator."


def names_and_shapes(P):
    out = []
    for branch, c in (("s_features", 3), ("t_features", 6)):
        for k, (ci, co, _) in enumerate(BRANCH):
            ci = c if ci is None else ci
            base = "%s%s.%d." % (PREFIX, branch, k)
            out += [(base + "0.weight", (co, ci, 3, 3)), (base + "1.weight", (co,)), (base + "1.bias", (co,)),
                    (base + "1.running_mean", (co,)), (base + "1.running_var", (co,)), (base + "1.num_batches_tracked", ())]
    q = P // 16
    out += [(PREFIX + "classifier.0.weight", (1024, 128 * q * q)), (PREFIX + "classifier.0.bias", (1024,)),
            (PREFIX + "classifier.2.weight", (1, 1024)), (PREFIX + "classifier.2.bias", (1,))]
    return out


def is_parameter(name):
    return not name.endswith(("running_mean", "running_var", "num_batches_tracked"))


def fill_state(seed, P):
    """{name: float64 tensor (int64 for num_batches_tracked)}.  Convolution and linear weights are normal with standard deviation
    1 / sqrt(fan-in), BatchNorm scales 1 + 0.2 normal, every bias 0.1 normal; running statistics 0 / 1 / 0 (a fresh module's)."""
    rs = np.random.RandomState(seed)
    state = {}
    for name, shape in names_and_shapes(P):
        if name.endswith("num_batches_tracked"):
            state[name] = torch.zeros((), dtype=torch.int64)
        elif name.endswith("running_mean"):
            state[name] = torch.zeros(shape, dtype=torch.float64)
        elif name.endswith("running_var"):
            state[name] = torch.ones(shape, dtype=torch.float64)
        elif name.endswith("bias"):
            state[name] = torch.from_numpy(0.1 * rs.standard_normal(shape))
        elif len(shape) == 1:
            state[name] = torch.from_numpy(1.0 + 0.2 * rs.standard_normal(shape))
        else:
            fan_in = int(np.prod(shape[1:]))
            state[name] = torch.from_numpy(rs.standard_normal(shape) / np.sqrt(fan_in))
    return state


def softplus(x):
    """log(1 + exp(x)) in the stable form of BCE with logits at target 0: max(x, 0) + log1p(exp(-|x|))."""
    return torch.clamp(x, min=0) + torch.log1p(torch.exp(-x.abs()))


class RefAdversarial:
    def __init__(self, P, state, dtype=torch.float64):
        if P % 16:
            raise ValueError("P % 16")
        self.P, self.dtype = P, dtype
        self.state = {k: (v.clone() if v.dtype == torch.int64 else v.to(dtype).clone()) for k, v in state.items()}
        self.param_names = [n for n, _ in names_and_shapes(P) if is_parameter(n)]
        self.exp_avg = {n: torch.zeros_like(self.state[n]) for n in self.param_names}
        self.exp_inf = {n: torch.zeros_like(self.state[n]) for n in self.param_names}
        self.t = 0
        self.preacts = None            # a list: every LeakyReLU's pre-activation of the passes that follow is appended

    def discriminator(self, w, f0, f1, f2):
        """One pass with the weights `w` (name -> tensor); updates the running statistics in self.state."""
        feats = []
        for branch, x in (("s_features", f1), ("t_features", torch.cat([f1 - f0, f1 - f2], 1))):
            for k, (_, co, stride) in enumerate(BRANCH):
                base = "%s%s.%d." % (PREFIX, branch, k)
                z = F.conv2d(x, w[base + "0.weight"], None, stride, 1)
                n = z.numel() // co
                if n < 2:
                    raise ValueError("batch statistics over one value")
                mean = z.mean((0, 2, 3))
                var = ((z - mean[None, :, None, None]) ** 2).mean((0, 2, 3))
                with torch.no_grad():
                    rm, rv = self.state[base + "1.running_mean"], self.state[base + "1.running_var"]
                    rm.mul_(1 - MOMENTUM).add_(MOMENTUM * mean.detach())
                    rv.mul_(1 - MOMENTUM).add_(MOMENTUM * var.detach() * n / (n - 1))
                    self.state[base + "1.num_batches_tracked"] += 1
                xh = (z - mean[None, :, None, None]) / torch.sqrt(var + EPS)[None, :, None, None]
                y = xh * w[base + "1.weight"][None, :, None, None] + w[base + "1.bias"][None, :, None, None]
                if self.preacts is not None:
                    self.preacts.append(y.detach())
                x = torch.where(y > 0, y, SLOPE * y)
            feats.append(x.reshape(x.shape[0], -1))
        h = torch.cat(feats, 1) @ w[PREFIX + "classifier.0.weight"].t() + w[PREFIX + "classifier.0.bias"]
        if self.preacts is not None:
            self.preacts.append(h.detach())
        h = torch.where(h > 0, h, SLOPE * h)
        return h @ w[PREFIX + "classifier.2.weight"].t() + w[PREFIX + "classifier.2.bias"]

    def call(self, fake, real, frames):
        dt = self.dtype
        fake, real, frames = fake.to(dt), real.to(dt), frames.to(dt)
        f0, f2 = frames[:, 0], frames[:, 1]
        w = {n: self.state[n].detach().requires_grad_(True) for n in self.param_names}
        d_fake = self.discriminator(w, f0, fake.detach(), f2)
        d_real = self.discriminator(w, f0, real, f2)
        loss_d = softplus(d_fake).mean() + softplus(-d_real).mean()
        grads = torch.autograd.grad(loss_d, [w[n] for n in self.param_names])
        self.t += 1
        with torch.no_grad():
            for n, g in zip(self.param_names, grads):
                m, u, p = self.exp_avg[n], self.exp_inf[n], self.state[n]
                m.add_((1 - BETA1) * (g - m))
                torch.maximum(BETA2 * u, g.abs() + ADAMAX_EPS, out=u)
                p.sub_(LR / (1 - BETA1 ** self.t) * m / u)
        fake = fake.detach().requires_grad_(True)
        w = {n: self.state[n] for n in self.param_names}
        loss_g = softplus(-self.discriminator(w, f0, fake, f2)).mean()
        (grad_fake,) = torch.autograd.grad(loss_g, fake)
        return loss_d.detach(), loss_g.detach(), grad_fake


def inputs_from_bytes(u8):
    """The fixture keeps its images as bytes: value / 255 in float32, exactly representable in every precision compared."""
    return torch.from_numpy(np.asarray(u8)).to(torch.float32) / 255.0


def make_inputs(seed, B, P, calls=2):
    """Per call (fake, real, frames [B, 2, 3, P, P]) as uint8 arrays: smooth random images (a few low-frequency cosines plus
    noise), the neighbours shifted copies of `real` and `fake` a noisy copy -- what the term sees in training, not white noise."""
    rs = np.random.RandomState(seed)
    yy, xx = np.meshgrid(np.arange(P), np.arange(P), indexing="ij")
    out = []

    def image():
        img = np.zeros((B, 3, P, P))
        for _ in range(4):
            fy, fx, ph = rs.uniform(0, 3, (B, 3, 1, 1)), rs.uniform(0, 3, (B, 3, 1, 1)), rs.uniform(0, 6.28, (B, 3, 1, 1))
            img += rs.uniform(0.05, 0.25, (B, 3, 1, 1)) * np.cos(2 * np.pi * (fy * yy + fx * xx) / P + ph)
        return img + 0.5

    to_u8 = lambda a: np.clip(np.rint(a * 255), 0, 255).astype(np.uint8)
    for _ in range(calls):
        real = image() + 0.03 * rs.standard_normal((B, 3, P, P))
        fake = real + 0.08 * rs.standard_normal((B, 3, P, P)) + 0.05 * (image() - 0.5)
        n0 = np.roll(real, 1, 3) + 0.03 * rs.standard_normal((B, 3, P, P))
        n2 = np.roll(real, -1, 2) + 0.03 * rs.standard_normal((B, 3, P, P))
        out.append((to_u8(fake), to_u8(real), to_u8(np.stack([n0, n2], 1))))
    return out
