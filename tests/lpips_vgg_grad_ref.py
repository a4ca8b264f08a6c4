"""The gradient yardstick of the LPIPS VGG-16 training loss: torch-CPU autograd through the restatement of lpips_vgg_ref
(ref_features / ref_distances, F.conv2d / F.max_pool2d / F.relu), in float64 by default, with the seeded random_trunk and the
fixture heads; the cases of test_gpu_lpips_vgg_grad and the error measure they are held to.  Shared by
test_lpips_vgg_grad_host and test_gpu_lpips_vgg_grad."""
import torch

from lpips_vgg_ref import fixture_heads, random_trunk, ref_distances, ref_features

GRAD_OUT = (1.5, 0.0, -0.5)        # per pair: a scale, a zero weight and a sign

# N, C, H, W, kind; the bar of a kind comes from the float32 evaluation of the kind's cases ("dead" is held to the random bar)
CASES = [
    (1, 3, 16, 16, "random"),        # f5 is one pixel
    (2, 1, 17, 19, "unclamped"),     # odd maps, an unrouted border, the scalar path, the channel fold
    (2, 3, 31, 45, "near"),          # target = pred + 1e-3 noise
    (1, 3, 32, 48, "random"),        # even widths
    (2, 3, 20, 27, "unclamped-pm1"), # normalize=False on [-1, 1]
    (3, 3, 33, 39, "random"),        # (the device test passes pred as a strided view)
    (1, 3, 16, 16, "dead"),          # flat left half under a conv1_2 bias lowered by 2.0: all-zero feature pixels
]
DEAD_BIAS_DROP = 2.0


def kind_of_bar(kind):
    return {"unclamped-pm1": "unclamped", "dead": "random"}.get(kind, kind)


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
    if kind == "unclamped-pm1":
        return pred * 2 - 1, target * 2 - 1, False
    return pred, target, True


def trunk_of(case, seed=0):
    """(ws, bs, heads): the seeded trunk; for the dead case with conv1_2's bias lowered, so that flat regions give all-zero f1."""
    ws, bs = random_trunk(seed)
    if case[4] == "dead":
        bs = [b.clone() for b in bs]
        bs[1] -= DEAD_BIAS_DROP
    return ws, bs, fixture_heads()


def ref_grad(pred, target, ws, bs, heads, grad_out, normalize=True, dtype=torch.float64):
    """(d/dpred of sum_n grad_out[n] * lpips[n], lpips [N]) by CPU autograd in `dtype`; pred [N, C, H, W], C in {1, 3}."""
    pred = torch.as_tensor(pred).detach().cpu().to(dtype).clone().requires_grad_(True)
    target = torch.as_tensor(target).detach().cpu().to(dtype)
    p3, t3 = pred, target
    if pred.shape[1] == 1:
        p3, t3 = pred.expand(-1, 3, -1, -1), target.expand(-1, 3, -1, -1)
    layers = ref_distances(ref_features(p3, ws, bs, normalize, dtype), ref_features(t3, ws, bs, normalize, dtype), heads)
    lpips = layers.sum(1)
    (lpips * torch.as_tensor(grad_out).to(dtype)).sum().backward()
    return pred.grad.detach(), lpips.detach()


def dead_pixels(pred, ws, bs, normalize=True):
    """How many pixels of the first tap map of pred (image 0) have every channel zero."""
    f1 = ref_features(pred[:1].expand(-1, 3, -1, -1) if pred.shape[1] == 1 else pred[:1], ws, bs, normalize)[0]
    return int(((f1 ** 2).sum(1) == 0).sum())


def pair_errors(got, want):
    """Per pair max|got - want| / max|want| (want in float64); None where max|want| == 0."""
    got, want = got.detach().cpu().double(), want.double()
    out = []
    for g, w in zip(got, want):
        top = w.abs().max().item()
        out.append((g - w).abs().max().item() / top if top > 0 else None)
    return out
