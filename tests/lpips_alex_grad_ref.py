"""The gradient yardstick of the LPIPS AlexNet training loss: torch-CPU autograd through a restatement of the definition
(include/ebfi_hip.h, ebfi_lpips_alex: F.conv2d / F.max_pool2d / F.relu) with a `dtype` argument -- test_lpips_host.ref_features is
fixed to float64 -- in float64 by default, with the seeded random_trunk and the fixture heads of test_lpips_host; the cases of
test_gpu_lpips_alex_grad and the error measure they are held to.  Shared by test_lpips_alex_grad_host and
test_gpu_lpips_alex_grad."""
import torch
import torch.nn.functional as F

from test_lpips_host import SCALE, SHIFT, fixture_heads, random_trunk

GRAD_OUT = (1.5, 0.0, -0.5)        # per pair: a scale, a zero weight and a sign

# N, C, H, W, kind; the bar of a kind comes from the float32 evaluation of the kind's cases ("dead" and "flat" are held to the
# random bar and do not set it)
CASES = [
    (1, 3, 31, 31, "random"),          # the smallest size: f1 7x7, pooled 3x3, f3..f5 one pixel, every 5x5 tap partly in padding
    (2, 1, 34, 38, "unclamped"),       # the channel fold; input row 33 is in no conv1 window (exactly 0); f1 7x8: an unpooled column
    (2, 3, 35, 47, "near"),            # pred = target + 1e-3 noise: cancellation; f1 8x11
    (1, 3, 64, 80, "random"),          # f1 15x19: several overlapping windows
    (2, 3, 41, 52, "unclamped-pm1"),   # normalize=False on [-1, 1]: the other mul_c
    (3, 3, 71, 93, "random"),          # f1 17x22 (the device test also passes pred as a strided view)
    (1, 3, 143, 150, "random"),        # pooled f1 17x17: more than one 16 x 16 tile in the 5x5 gradient
    (1, 3, 47, 51, "dead"),            # flat left half under a conv1 bias lowered by 1.0: all-zero f1 pixels
    (1, 3, 47, 51, "flat"),            # pred = 0.5 everywhere: positive tied maxima in f1's windows, the first-maximum rule decides
]
DEAD_BIAS_DROP = 1.0


def kind_of_bar(kind):
    return {"unclamped-pm1": "unclamped", "dead": "random", "flat": "random"}.get(kind, kind)


def case_id(case):
    return "%dx%dx%dx%d-%s" % case


def grad_out_of(n):
    return torch.tensor(GRAD_OUT[:n], dtype=torch.float32)


def make_pair(case, seed=None):
    """(pred, target, normalize) of a case, drawn on the CPU."""
    n, c, h, w, kind = case
    g = torch.Generator().manual_seed(n * 1000 + h * 7 + w if seed is None else seed)
    target = torch.rand(n, c, h, w, generator=g)
    if kind == "near":
        pred = target + 1e-3 * torch.randn(n, c, h, w, generator=g)
    elif kind.startswith("unclamped"):
        pred = target + 0.4 * torch.randn(n, c, h, w, generator=g)
    else:
        pred = torch.rand(n, c, h, w, generator=g)
    if kind == "dead":
        pred[..., : w // 2] = 0.5
        target[..., : w // 2] = 0.3
    if kind == "flat":
        pred[:] = 0.5
    if kind == "unclamped-pm1":
        return pred * 2 - 1, target * 2 - 1, False
    return pred, target, True


def trunk_of(case, seed=0):
    """(ws, bs, heads): the seeded trunk; for the dead case with conv1's bias lowered, so that flat regions give all-zero f1."""
    ws, bs = random_trunk(seed)
    if case[4] == "dead":
        bs = [b.clone() for b in bs]
        bs[0] -= DEAD_BIAS_DROP
    return ws, bs, fixture_heads()


def ref_features(x, ws, bs, normalize=True, dtype=torch.float64):
    """The five ReLU maps of the AlexNet trunk for [N, 3, H, W] images, computed in `dtype`."""
    x = x.to(dtype)
    if normalize:
        x = 2 * x - 1
    shift = torch.tensor(SHIFT, dtype=dtype).view(1, 3, 1, 1)
    scale = torch.tensor(SCALE, dtype=dtype).view(1, 3, 1, 1)
    x = (x - shift) / scale
    w = [t.to(dtype) for t in ws]
    b = [t.to(dtype) for t in bs]
    f1 = F.relu(F.conv2d(x, w[0], b[0], stride=4, padding=2))
    f2 = F.relu(F.conv2d(F.max_pool2d(f1, 3, 2), w[1], b[1], padding=2))
    f3 = F.relu(F.conv2d(F.max_pool2d(f2, 3, 2), w[2], b[2], padding=1))
    f4 = F.relu(F.conv2d(f3, w[3], b[3], padding=1))
    f5 = F.relu(F.conv2d(f4, w[4], b[4], padding=1))
    return [f1, f2, f3, f4, f5]


def ref_distances(feats0, feats1, heads, dtype=torch.float64):
    """[N, L] layer terms: mean over the pixels of sum_c w_c (u0_c - u1_c)^2, u = f / (||f||_c + 1e-10)."""
    out = []
    for f0, f1, h in zip(feats0, feats1, heads):
        u0 = f0 / (torch.sqrt((f0 ** 2).sum(1, keepdim=True)) + 1e-10)
        u1 = f1 / (torch.sqrt((f1 ** 2).sum(1, keepdim=True)) + 1e-10)
        out.append((h.to(dtype).view(1, -1, 1, 1) * (u0 - u1) ** 2).sum(1).mean((1, 2)))
    return torch.stack(out, 1)


def ref_grad(pred, target, ws, bs, heads, grad_out, normalize=True, dtype=torch.float64):
    """(d/dpred of sum_n grad_out[n] * lpips[n], lpips [N]) by CPU autograd in `dtype`; pred [N, C, H, W], C in {1, 3}."""
    pred = torch.as_tensor(pred).detach().cpu().to(dtype).clone().requires_grad_(True)
    target = torch.as_tensor(target).detach().cpu().to(dtype)
    p3, t3 = pred, target
    if pred.shape[1] == 1:
        p3, t3 = pred.expand(-1, 3, -1, -1), target.expand(-1, 3, -1, -1)
    layers = ref_distances(ref_features(p3, ws, bs, normalize, dtype), ref_features(t3, ws, bs, normalize, dtype), heads, dtype)
    lpips = layers.sum(1)
    (lpips * torch.as_tensor(grad_out).to(dtype)).sum().backward()
    return pred.grad.detach(), lpips.detach()


def _f1_of_image0(pred, ws, bs, normalize):
    return ref_features(pred[:1].expand(-1, 3, -1, -1) if pred.shape[1] == 1 else pred[:1], ws, bs, normalize)[0]


def dead_pixels(pred, ws, bs, normalize=True):
    """(all-zero pixels, pixels) of the first tap map of pred (image 0)."""
    f1 = _f1_of_image0(pred, ws, bs, normalize)
    return int(((f1 ** 2).sum(1) == 0).sum()), f1.shape[2] * f1.shape[3]


def tied_windows(pred, ws, bs, normalize=True):
    """How many (3x3/s2 window, channel) pairs of the first tap map of pred (image 0) have a positive maximum held by two or more
    of the window's pixels."""
    f1 = _f1_of_image0(pred, ws, bs, normalize)
    win = f1.unfold(2, 3, 2).unfold(3, 3, 2).reshape(f1.shape[0], f1.shape[1], -1, 9)
    top = win.amax(-1, keepdim=True)
    return int(((top[..., 0] > 0) & ((win == top).sum(-1) >= 2)).sum())


def pair_errors(got, want):
    """Per pair max|got - want| / max|want| (want in float64); None where max|want| == 0."""
    got, want = got.detach().cpu().double(), want.double()
    out = []
    for g, w in zip(got, want):
        top = w.abs().max().item()
        out.append((g - w).abs().max().item() / top if top > 0 else None)
    return out
