"""The ExposureDecision head on the MI355X -- csrc/edhead.hip (fused.ed_head) and its fallback pair norm.group_norm ->
fused.product_mean -> sigmoid -> fused.scale_cat -- against a float64 restatement of the reference formulation
(models/Ours/model_singleframe.py:66-72: nn.GroupNorm on both maps, product, AdaptiveAvgPool2d(1), sigmoid, cat; gradients by
autograd), with the same formulation in fp32 on the CPU as the comparison point.

The bound, for each of out, grad_ev, grad_bl, grad_gamma, grad_beta:
    e32 = max|ref32 - ref64|,  eK = max|device - ref64|,  eK <= FACTOR * e32 + 4 * 2^-24 * max|ref64|
FACTOR = 8 covers another summation order plus the few fp32 operations per element of the closed-form apply; the floor of
4 ulp of the result's scale keeps a case where torch happens to be exact from failing on one rounding.  The maps are
ill-conditioned on purpose (|mean| >> std, near-constant and constant groups): E[x^2] - mu^2 formed from fp32 sums is 100x to
1000x outside this bound there."""
import functools

import pytest
import torch
import torch.nn as nn
import torch.nn.functional as F

pytestmark = pytest.mark.gpu

FACTOR = 8.0
NAMES = ("out", "grad_ev", "grad_bl", "grad_gamma", "grad_beta")

# (mean, std) of ev and of bl; "const": ev ~ (0.4, 1.5) with group 0 of sample 0 exactly 0.75
SWEEP = {
    "m0.4_s1.5": ((0.4, 1.5), (0.4, 1.5)),
    "m16_s1": ((16.0, 1.0), (16.0, 1.0)),
    "m64_s1": ((64.0, 1.0), (64.0, 1.0)),
    "m-64_s1": ((-64.0, 1.0), (-64.0, 1.0)),
    "m1_s1e-2": ((1.0, 1e-2), (1.0, 1e-2)),
    "m1_s1e-3": ((1.0, 1e-3), (1.0, 1e-3)),
    "mixed": ((0.4, 1.5), (64.0, 1.0)),
    "const": ((0.4, 1.5), (0.4, 1.5)),
}
SWEEP_SHAPE = (2, 8, 2, 64, 64)          # one slice of 4096 elements: four float4 iterations per lane, wave tree, four-wave sum
REGIME_SHAPES = [
    (1, 4, 2, 91, 92),                   # 2 slices of chunk 4188, the last one holds 4184
    (1, 4, 2, 106, 116),                 # 3 slices
    (3, 6, 3, 2, 2),                     # HW = 4: one lane does all the work
    (1, 72, 3, 4, 4),                    # C no multiple of 64: 128 finaliser threads
    (1, 1024, 4, 2, 2),                  # the channel cap, 41 KB of dynamic LDS
    (9, 8, 4, 4, 8),                     # the coefficient kernel's serial loop over samples
]


@functools.lru_cache(maxsize=None)
def _inputs(case, shape, affine=True):
    """(ev, bl, gamma, beta, grad_out) on the CPU in fp32; never modified afterwards (shared between the tests)."""
    B, C, G, H, W = shape
    (me, se), (mb, sb) = SWEEP[case]
    g = torch.Generator().manual_seed(1000 + sum(ord(ch) for ch in case) + B * 7 + C * 3 + H + W)
    u = torch.randn(B, C, H, W, generator=g, dtype=torch.float64)
    n = torch.randn(B, C, H, W, generator=g, dtype=torch.float64)
    ev = (me + se * u).float()
    bl = (mb + sb * (0.5 * u + 0.75 ** 0.5 * n)).float()        # bl = 0.5 ev + noise + offset: the pooled product is not ~0
    if case == "const":
        ev[0, : C // G] = 0.75                                     # variance exactly 0: rstd = 1 / sqrt(eps)
    gamma = (1.0 + 0.5 * torch.randn(C, generator=g)) if affine else None
    beta = (0.3 * torch.randn(C, generator=g)) if affine else None
    gout = torch.randn(B, 2 * C, H, W, generator=g)
    return ev, bl, gamma, beta, gout


def _gn(G, C, gamma, beta, dtype=torch.float32, device="cpu"):
    gn = nn.GroupNorm(G, C, affine=gamma is not None)
    if gamma is not None:
        with torch.no_grad():
            gn.weight.copy_(gamma)
            gn.bias.copy_(beta)
    return gn.to(device=device, dtype=dtype)


def _formulation(ev, bl, gn):
    atten = torch.sigmoid(F.adaptive_avg_pool2d(gn(ev) * gn(bl), 1))
    return torch.cat([ev * atten, bl], dim=1)


def _results(head, ev, bl, gn, gout):
    """The five results of `head(ev, bl, gn)` as float64 CPU tensors (None for a parameter the GroupNorm does not have)."""
    ev, bl = ev.detach().clone().requires_grad_(), bl.detach().clone().requires_grad_()
    out = head(ev, bl, gn)
    assert out is not None
    out.backward(gout)
    grads = [ev.grad, bl.grad, gn.weight.grad if gn.weight is not None else None, gn.bias.grad if gn.bias is not None else None]
    return [None if t is None else t.detach().double().cpu() for t in [out] + grads]


@functools.lru_cache(maxsize=None)
def _references(case, shape, affine=True):
    """(ref64, ref32) of the reference formulation on the CPU."""
    ev, bl, gamma, beta, gout = _inputs(case, shape, affine)
    G, C = shape[2], shape[1]
    r64 = _results(_formulation, ev.double(), bl.double(), _gn(G, C, gamma, beta, torch.float64), gout.double())
    r32 = _results(_formulation, ev, bl, _gn(G, C, gamma, beta), gout)
    return r64, r32


def _assert_bound(tag, got, r64, r32, names=NAMES):
    bad = []
    for name, k, a, b in zip(names, got, r64, r32):
        if a is None:
            assert k is None, name
            continue
        e32, ek, scale = (b - a).abs().max().item(), (k - a).abs().max().item(), a.abs().max().item()
        bound = FACTOR * e32 + 4.0 * 2.0 ** -24 * scale
        print("%-34s %-10s e32 %.3e  eK %.3e  eK/e32 %8.2f  bound %.3e  max|ref| %.3e"
              % (tag, name, e32, ek, ek / e32 if e32 > 0 else float("inf") if ek > 0 else 0.0, bound, scale))
        if not ek <= bound:                                         # (a NaN error fails too)
            bad.append((name, e32, ek, bound))
    assert not bad, (tag, bad)


def _ed_head(ev, bl, gn):
    from ebfi_amd import fused
    return fused.ed_head(ev, bl, gn)


def _fallback(ev, bl, gn):
    """What ExposureDecision.ex_map composes when fused.ed_head declines."""
    from ebfi_amd import fused, norm
    atten = torch.sigmoid(fused.product_mean(norm.group_norm(ev, gn), norm.group_norm(bl, gn)))
    return fused.scale_cat(ev, atten, bl)


def _device_results(head, case, shape, affine=True):
    ev, bl, gamma, beta, gout = _inputs(case, shape, affine)
    return _results(head, ev.cuda(), bl.cuda(), _gn(shape[2], shape[1], gamma, beta, device="cuda"), gout.cuda())


@pytest.mark.parametrize("case", list(SWEEP))
def test_ed_head_conditioning_sweep(case):
    _assert_bound("ed_head %s" % case, _device_results(_ed_head, case, SWEEP_SHAPE), *_references(case, SWEEP_SHAPE))


@pytest.mark.parametrize("case", ["m0.4_s1.5", "m16_s1"])
@pytest.mark.parametrize("shape", REGIME_SHAPES, ids=lambda s: "x".join(map(str, s)))
def test_ed_head_regime_shapes(shape, case):
    _assert_bound("ed_head %s %s" % (shape, case), _device_results(_ed_head, case, shape), *_references(case, shape))


@pytest.mark.parametrize("case", list(SWEEP))
def test_fallback_pair_conditioning_sweep(case):
    _assert_bound("fallback %s" % case, _device_results(_fallback, case, SWEEP_SHAPE), *_references(case, SWEEP_SHAPE))


# ---- fused.ed_head declines; the model path then runs the fallback composition ----

def _model_results(ed, event, blur, gout):
    event, blur = event.detach().clone().requires_grad_(), blur.detach().clone().requires_grad_()
    ed.zero_grad(set_to_none=True)
    out = ed(event, blur)
    out.backward(gout)
    gn = ed.GroupNorm
    grads = [event.grad, blur.grad, gn.weight.grad if gn.weight is not None else None, gn.bias.grad if gn.bias is not None else None]
    return [None if t is None else t.detach().double().cpu() for t in [out] + grads]


class _PlainExposureDecision(nn.Module):
    """ExposureDecision of the reference (model_singleframe.py:23-76) in plain torch ops, any dtype, for the CPU."""

    def __init__(self, src, dtype):
        super().__init__()
        import copy
        self.ev, self.bl = copy.deepcopy(src.EventFeatExtract.conv2d), copy.deepcopy(src.BLFeatExtract.conv2d)
        self.c1, self.c2 = copy.deepcopy(src.Conv1[0].conv2d), copy.deepcopy(src.Conv1[1].conv2d)
        self.GroupNorm = copy.deepcopy(src.GroupNorm)
        self.slope = src.EventFeatExtract.activation.negative_slope
        self.to(dtype)

    def forward(self, event, blur):
        ev, bl = F.leaky_relu(self.ev(event), self.slope), F.leaky_relu(self.bl(blur), self.slope)
        cat = _formulation(ev, bl, self.GroupNorm)
        x = self.c2(F.leaky_relu(self.c1(cat), self.slope))
        return torch.sigmoid(F.adaptive_avg_pool2d(x, 1).view(-1, 1))


@pytest.mark.parametrize("why", ["hw_not_multiple_of_4", "no_affine"])
def test_declined_head_model_path(why):
    """ExposureDecision.forward through the fallback composition: 5x5 maps (H*W % 4 != 0: torch's own GroupNorm on the device)
    and a GroupNorm without affine parameters (the native kernels' NULL gamma / beta branches)."""
    from ebfi_amd import fused
    from ebfi_amd.model import ExposureDecision
    torch.manual_seed(31)
    B, Cin, C, G = 2, 4, 8, 2
    H, W = (5, 5) if why == "hw_not_multiple_of_4" else (8, 12)
    ed = ExposureDecision(EventInch=Cin, BLInch=1, InterCH=C, Group=G)
    with torch.no_grad():                                          # the x0.1 initialisation leaves hardly any signal
        for p in ed.parameters():
            if p.dim() > 1:
                p.copy_(torch.randn_like(p) * (1.2 / p[0].numel() ** 0.5))
        ed.GroupNorm.weight.copy_(1.0 + 0.5 * torch.randn(C))
        ed.GroupNorm.bias.copy_(0.3 * torch.randn(C))
    if why == "no_affine":
        ed.GroupNorm = nn.GroupNorm(G, C, affine=False)
    event, blur, gout = torch.randn(B, Cin, H, W) + 0.5, torch.rand(B, 1, H, W), torch.randn(B, 1)
    r64 = _model_results(_PlainExposureDecision(ed, torch.float64), event.double(), blur.double(), gout.double())
    r32 = _model_results(_PlainExposureDecision(ed, torch.float32), event, blur, gout)
    dev = ed.cuda()
    x = torch.randn(B, C, H, W, device="cuda")
    assert fused.ed_head(x, x.clone(), dev.GroupNorm) is None
    got = _model_results(dev, event.cuda(), blur.cuda(), gout.cuda())
    _assert_bound("model path %s" % why, got, r64, r32, names=("duty", "grad_event", "grad_blur", "grad_gamma", "grad_beta"))


def test_head_declines_what_it_cannot_run():
    from ebfi_amd import fused
    x, z = torch.randn(2, 8, 5, 5, device="cuda"), torch.randn(2, 8, 5, 5, device="cuda")
    assert fused.ed_head(x, z, nn.GroupNorm(2, 8).cuda()) is None                       # H*W % 4 != 0
    x, z = torch.randn(2, 8, 4, 4, device="cuda"), torch.randn(2, 8, 4, 4, device="cuda")
    assert fused.ed_head(x, z, nn.GroupNorm(2, 16).cuda()) is None                      # C != gn.num_channels
    assert fused.ed_head(x, z, nn.GroupNorm(2, 8, affine=False).cuda()) is None         # no gamma / beta
    assert fused.ed_head(x, z, nn.GroupNorm(2, 8).cuda()) is not None


# ---- non-finite inputs ----

NF_SHAPE = (3, 8, 2, 8, 8)


def _nf_forward(ev, bl, gamma, beta):
    with torch.no_grad():
        out = _ed_head(ev.cuda(), bl.cuda(), _gn(NF_SHAPE[2], NF_SHAPE[1], gamma, beta, device="cuda"))
    assert out is not None
    return out.cpu()


@pytest.mark.parametrize("which", ["ev", "bl"])
@pytest.mark.parametrize("where", ["first", "last"])
def test_nan_stays_in_its_sample_and_group(which, where):
    B, C, G, H, W = NF_SHAPE
    ev, bl, gamma, beta, _ = _inputs("m0.4_s1.5", NF_SHAPE)
    clean = _nf_forward(ev, bl, gamma, beta)
    ev, bl = ev.clone(), bl.clone()
    c = 5                                                          # a plane of group 1 (channels 4..7)
    (ev if which == "ev" else bl)[1, c].view(-1)[0 if where == "first" else -1] = float("nan")
    out = _nf_forward(ev, bl, gamma, beta)
    cpg = C // G
    grp = slice((c // cpg) * cpg, (c // cpg + 1) * cpg)
    assert torch.isnan(out[1, grp]).all()                          # ev * atten: every channel of the plane's group
    other = slice(0, cpg)
    assert torch.equal(out[1, other], clean[1, other])             # the sample's other group does not see it
    want_bl = torch.isnan(bl[1])
    assert torch.equal(torch.isnan(out[1, C:]), want_bl) and torch.equal(out[1, C:][~want_bl], bl[1][~want_bl])
    for b in (0, 2):
        assert torch.equal(out[b], clean[b]), b


@pytest.mark.parametrize("variant", ["plain", "negative_plane"])
def test_inf_gives_the_nan_mask_of_the_fp32_formulation(variant):
    """negative_plane: a bl plane of the inf's group whose mean has the other sign than the group's mean, with gamma * beta < 0.
    The pooled product's closed form is then +inf - (-inf), not inf - inf, unless the group's variance (NaN) is kept NaN:
    a finaliser that clamps it with fmax gives that plane an attention of exactly 1 where nn.GroupNorm gives NaN."""
    B, C, G, H, W = NF_SHAPE
    ev, bl, gamma, beta, _ = _inputs("m0.4_s1.5", NF_SHAPE)
    if variant == "negative_plane":
        c = 1                                                      # a plane of the inf's group, not the inf's own (2)
        gamma, beta, bl = gamma.clone(), beta.clone(), bl.clone()
        gamma[c], beta[c] = 1.25, -0.4                             # gamma * beta < 0
        bl[1, c] -= 1.0
        assert bl[1, c].mean() < 0 < bl[1, : C // G].mean()
    clean = _nf_forward(ev, bl, gamma, beta)
    ev = ev.clone()
    ev[1, 2, 3, 4] = float("inf")
    out = _nf_forward(ev, bl, gamma, beta)
    for b in (0, 2):
        assert torch.equal(out[b], clean[b]), b
    with torch.no_grad():
        ref = _formulation(ev, bl, _gn(G, C, gamma, beta))
    assert torch.equal(torch.isnan(out[1]), torch.isnan(ref[1]))
    assert torch.isnan(ref[1, : C // G]).all()                     # (the whole group of the plane with the inf)


# ---- reproducibility ----

@pytest.mark.parametrize("shape", [(1, 4, 2, 91, 92), SWEEP_SHAPE], ids=["2_slices", "sweep_shape"])
def test_forward_backward_twice_gives_identical_bits(shape):
    a = _device_results(_ed_head, "m16_s1", shape)
    b = _device_results(_ed_head, "m16_s1", shape)
    for name, x, y in zip(NAMES, a, b):
        assert torch.equal(x, y), name


# ---- norm.group_norm alone ----

def _gn_results(fn, x, gn, gy):
    x = x.detach().clone().requires_grad_()
    y = fn(x, gn)
    y.backward(gy)
    grads = [x.grad, gn.weight.grad if gn.weight is not None else None, gn.bias.grad if gn.bias is not None else None]
    return [None if t is None else t.detach().double().cpu() for t in [y] + grads]


@pytest.mark.parametrize("name,shape,affine,case", [
    ("no_affine", (2, 8, 2, 8, 12), False, "m16_s1"),              # NULL gamma / beta in all three kernels
    ("no_affine_sweep_shape", SWEEP_SHAPE, False, "m64_s1"),
    ("more_groups_than_channels", (5, 4, 2, 2, 4), True, "m16_s1"),   # B * G = 10 > C = 4: the backward finaliser's sizing
    ("hw_4", (3, 6, 3, 2, 2), True, "m16_s1"),
    ("constant_group", SWEEP_SHAPE, True, "const"),
])
def test_group_norm_alone(name, shape, affine, case):
    from ebfi_amd import norm
    B, C, G, H, W = shape
    x, _, gamma, beta, gout = _inputs(case, shape, affine)
    gy = gout[:, :C].contiguous()
    plain = lambda t, m: m(t)
    r64 = _gn_results(plain, x.double(), _gn(G, C, gamma, beta, torch.float64), gy.double())
    r32 = _gn_results(plain, x, _gn(G, C, gamma, beta), gy)
    got = _gn_results(norm.group_norm, x.cuda(), _gn(G, C, gamma, beta, device="cuda"), gy.cuda())
    _assert_bound("group_norm %s" % name, got, r64, r32, names=("y", "grad_x", "grad_gamma", "grad_beta"))
