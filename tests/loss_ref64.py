"""Float64 restatement of the Laplacian loss of the training step (csrc/laploss.hip), shared by test_loss_f64_host.py and
test_gpu_loss_f64.py: the pyramid of the DIFFERENCE planes [a - t ; b - t], its adjoint, the margins inside which a float32
computation of either must lie, and the table of cases (each rebuilt from its seed).

The L1 gradient is a sign, so a comparison of gradients has a kink wherever a Laplacian element is ~0.  The tests avoid it by
splitting the work the way the kernels do: the forward leaves the sign field s_l = coef * 2^l * sign(lap_l) in the workspace
(checked element by element, with the margin tau_l deciding which elements have a determined sign), and the backward is a LINEAR
map of whatever the workspace holds (checked on every element against the float64 adjoint of the field the device produced).

Margins, u = 2^-24 (unit roundoff of float32), per plane:
    tau_l = 32 (l + 1) u max|d|        level element l of a plane whose difference is d
    bound = 32 levels u G_abs          gradient element; G_abs = adjoint of abs_pyramid64 applied to |s|, times |grad_loss|
Every pyramid operator is a convex combination (the blur's taps sum to 1, the pool is a mean, the expand's taps of one output
pixel sum to 1), so an error made at one level is not amplified at the next and every intermediate is bounded by max|d|.
Operator count of csrc/laploss.hip, in units of u max|d|:
    d = a - t in float32                                   1   (exact when a, t are within a factor 2: Sterbenz)
    reduce: 5 + 5 fused multiply-adds per blurred value (the first of each chain adds to 0: exact), 3 additions, * 0.25 exact
                                                           13 per level below l
    expand: horizontal fma sums (3), rounded row products and their sums (<= 6), times 4 exact      ~10
    lap = fma(-4, e, cur)                                  the result is bounded by 2 max|d|: 2
so level l carries at most (13 l + 25 + 1) u max|d| <= 32 (l + 1) u max|d|.  The adjoint walks the same operators transposed
(lap_bwd_reduce: two chains of 5 fma and fma(-4, adj, g), 11; lap_bwd_expand: * 0.25 exact, two chains of 5 fma, one addition,
11; the final scaling 1), each term relative to the sum of magnitudes that reaches the element, once per level: 32 levels.
The float32 CPU formulation (ebfi_amd.loss.LaplacianPyramid on CPU tensors) stays below 0.25 of both (test_loss_f64_host.py).

Planes are kept as [n * B, C, H, W] (n = 2 with a second prediction), plane index (image * C + channel) as in the workspace."""
import os
import sys

import torch
import torch.nn.functional as F

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from oracle import loss_ref  # noqa: E402

U = 2.0 ** -24
G_IN = 0.37

# name -> B, C, H, W, levels, two predictions, (coef_a, coef_b), input kind, seed
CASES = {
    "min5":   dict(B=2, C=3, H=32, W=32, levels=5, two=True, coefs=(0.1, 1.0), kind="rand", seed=0),
    "ragged": dict(B=2, C=3, H=48, W=80, levels=5, two=True, coefs=(1.0, 0.1), kind="rand", seed=1),
    "one":    dict(B=1, C=1, H=80, W=112, levels=5, two=False, coefs=(0.1, 1.0), kind="rand", seed=2),
    "min2":   dict(B=1, C=3, H=4, W=6, levels=2, two=True, coefs=(0.1, 1.0), kind="rand", seed=3),
    "min3":   dict(B=2, C=1, H=8, W=12, levels=3, two=True, coefs=(1.0, 0.1), kind="rand", seed=4),
    "near3":  dict(B=2, C=3, H=48, W=80, levels=5, two=True, coefs=(0.1, 1.0), kind="near3", seed=5),
    "near6":  dict(B=1, C=3, H=32, W=48, levels=5, two=True, coefs=(1.0, 0.1), kind="near6", seed=0),
    "patch":  dict(B=2, C=3, H=64, W=64, levels=5, two=True, coefs=(0.1, 1.0), kind="patch", seed=1),
}
NEAR = {"near3": (1e-3, 1e-2), "near6": (1e-6, 1e-4)}


def make_inputs(kind, shape, seed):
    """(a, b, t) float32 CPU images of `shape` = (B, C, H, W) from a generator seeded with `seed`."""
    g = torch.Generator().manual_seed(seed)
    t = torch.rand(shape, generator=g)
    if kind in NEAR:
        sa, sb = NEAR[kind]
        a = t + sa * torch.randn(shape, generator=g)
        b = t + sb * torch.randn(shape, generator=g)
        return a, b, t
    a, b = torch.rand(shape, generator=g), torch.rand(shape, generator=g)
    if kind == "patch":
        a[:, :, 16:48, 0:40] = t[:, :, 16:48, 0:40]
        b[1, 2] = t[1, 2]
    return a, b, t


def make_case(name):
    c = CASES[name]
    a, b, t = make_inputs(c["kind"], (c["B"], c["C"], c["H"], c["W"]), c["seed"])
    return a, (b if c["two"] else None), t


def difference64(a, b, t):
    """[a - t ; b - t] in float64 (b may be None)."""
    preds = [a] if b is None else [a, b]
    return torch.cat([p.double() - t.double() for p in preds])


# ------------------------------------------------------------------------------------------------ the pyramid and its kin
_K1 = torch.tensor([1., 4., 6., 4., 1.], dtype=torch.float64) / 16


def _blur(x, factor, pad):
    c = x.shape[1]
    k = (factor * torch.outer(_K1, _K1)).repeat(c, 1, 1, 1)
    return F.conv2d(F.pad(x, (2, 2, 2, 2), mode=pad), k, groups=c)


def general_pyramid(x, levels, sign=-1.0, pad="reflect", pool="avg", pad_expand=None):
    """The pyramid of oracle.loss_ref.laplacian_pyramid with its choices opened up: level = cur + sign * expand(reduce(cur)),
    `pad` the border rule of the blur (of the expand's blur: pad_expand, default the same), `pool` the subsampling.  The defaults
    restate the oracle (held equal to it by test_loss_f64_host.py); everything else is a deliberately wrong reference."""
    pad_expand = pad_expand or pad
    pyr, cur = [], x
    for _ in range(levels - 1):
        g = _blur(cur, 1.0, pad)
        red = F.avg_pool2d(g, 2) if pool == "avg" else g[:, :, ::2, ::2]
        up = torch.zeros(red.shape[0], red.shape[1], 2 * red.shape[2], 2 * red.shape[3], dtype=x.dtype)
        up[:, :, ::2, ::2] = red
        pyr.append(cur + sign * _blur(up, 4.0, pad_expand))
        cur = red
    pyr.append(cur)
    return pyr


def pyramid64(d, levels):
    """The oracle's Laplacian pyramid of a float64 difference d [planes / C, C, H, W]."""
    assert d.dtype == torch.float64
    return loss_ref.laplacian_pyramid(d, levels)


def abs_pyramid64(x, levels):
    """The same pyramid with cur + expand(reduce(cur)): all weights positive.  Of |d| it is zero exactly where the whole footprint
    of an element is zero; its adjoint of |s| is the sum of magnitudes G_abs the gradient bound is relative to."""
    assert x.dtype == torch.float64
    return general_pyramid(x, levels, sign=1.0)


def adjoint64(s_levels, pyr=pyramid64):
    """Float64 gradient with respect to d of sum_l <s_l, pyr(d)_l>.  The map is linear, so autograd at d = 0 is the adjoint."""
    d = torch.zeros(s_levels[0].shape, dtype=torch.float64, requires_grad=True)
    out = pyr(d, len(s_levels))
    value = sum((o * s.double()).sum() for o, s in zip(out, s_levels))
    return torch.autograd.grad(value, d)[0]


# ------------------------------------------------------------------------------------------------ margins
def plane_max(d):
    return d.abs().amax(dim=(2, 3), keepdim=True)


def taus(d, levels):
    """tau_l per plane, [planes / C, C, 1, 1] each."""
    m = plane_max(d)
    return [32.0 * (l + 1) * U * m for l in range(levels)]


def grad_bound(s_levels, grad_loss=1.0):
    """Elementwise bound of a float32 adjoint of the field s, scaled by grad_loss."""
    g_abs = adjoint64([s.double().abs() for s in s_levels], abs_pyramid64)
    return 32.0 * len(s_levels) * U * abs(grad_loss) * g_abs


def plane_coefs(coefs, n_images, B):
    """float32(coef) per image of the stacked planes, as float64 [n_images, 1, 1, 1]."""
    ca, cb = (float(torch.tensor(c, dtype=torch.float32)) for c in coefs)
    return torch.tensor([ca if i < B else cb for i in range(n_images)], dtype=torch.float64).view(-1, 1, 1, 1)


# ------------------------------------------------------------------------------------------------ the workspace
def workspace_floats(planes, H, W, levels):
    return sum(planes * (H >> l) * (W >> l) for l in range(levels))


def level_offsets(planes, H, W, levels):
    """Offset (floats) of level l in the workspace; entry `levels` is the total."""
    off = [0]
    for l in range(levels):
        off.append(off[-1] + planes * (H >> l) * (W >> l))
    return off


def split_levels(ws, n_images, C, H, W, levels):
    """The flat workspace as level images [n_images, C, H >> l, W >> l] (views)."""
    off = level_offsets(n_images * C, H, W, levels)
    return [ws[off[l]:off[l + 1]].view(n_images, C, H >> l, W >> l) for l in range(levels)]


def join_levels(s_levels):
    return torch.cat([s.reshape(-1) for s in s_levels])


# ------------------------------------------------------------------------------------------------ a case's yardstick
class Yardstick:
    """Everything float64 the tests need of one set of inputs, computed once."""

    def __init__(self, a, b, t, coefs, levels):
        self.levels, self.coefs = levels, coefs
        self.B, self.C, self.H, self.W = a.shape
        self.n_images = self.B * (1 if b is None else 2)
        self.d = difference64(a, b, t)
        self.lap = pyramid64(self.d, levels)
        self.foot = abs_pyramid64(self.d.abs(), levels)
        self.tau = taus(self.d, levels)
        self.coef = plane_coefs(coefs, self.n_images, self.B)
        # clear: the sign is determined; zero: the whole footprint is zero; ambiguous: neither
        self.zero = [f == 0 for f in self.foot]
        self.clear = [lp.abs() > tau for lp, tau in zip(self.lap, self.tau)]
        self.ambiguous = [~c & ~z for c, z in zip(self.clear, self.zero)]

    def v(self, l, coef=None, weight=None):
        """float32(coef(plane)) * 2^l (exact in float32), as float64 [n_images, 1, 1, 1]."""
        return (self.coef if coef is None else coef) * float(2 ** l if weight is None else weight)

    def sign_field(self, lap=None, coef=None, weights=None):
        """v * sign(lap) per level in float32: what the forward must leave where the sign is determined."""
        lap = self.lap if lap is None else lap
        return [(self.v(l, coef, None if weights is None else weights[l]) * torch.sign(lp)).float() for l, lp in enumerate(lap)]

    def value(self):
        return sum((self.v(l) * lp.abs()).sum().item() for l, lp in enumerate(self.lap))

    def value_margin(self):
        return sum((self.v(l) * tau).sum().item() * lp.shape[2] * lp.shape[3] for l, (lp, tau) in enumerate(zip(self.lap, self.tau)))

    def cap(self, l):
        return max(4, int(0.005 * self.lap[l].numel()))


_yardsticks = {}


def yardstick(name):
    if name not in _yardsticks:
        a, b, t = make_case(name)
        _yardsticks[name] = (a, b, t, Yardstick(a, b, t, CASES[name]["coefs"], CASES[name]["levels"]))
    return _yardsticks[name]


def spread_field(shape_levels, seed, spread):
    """A workspace of arbitrary contents: randn, or randn * 2^k with k uniform in -20 .. 20 per element (float32, exact)."""
    g = torch.Generator().manual_seed(seed)
    out = []
    for shp in shape_levels:
        s = torch.randn(shp, generator=g)
        if spread:
            s = s * torch.exp2(torch.randint(-20, 21, shp, generator=g).float())
        out.append(s)
    return out
