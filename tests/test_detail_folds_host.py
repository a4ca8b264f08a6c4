"""The depth-2 folds of the detail branch (ebfi_amd/fold3d.py) against torch's own Conv3d / ConvTranspose3d in float64 on the CPU,
outputs and -- through autograd -- the gradients of weight, bias and input; and the case table of
tests/test_gpu_detail_stages.py: every case's recorded seed gives a float64 reference without an activation near its kink."""
import pytest
import torch
import torch.nn as nn
import torch.nn.functional as F

import test_gpu_detail_stages as stages

TOL = 1e-12          # float64, sums of at most 3*7*7*4 products: measured 0 .. 9e-16


def _rel(got, ref):
    return ((got - ref).abs().max() / ref.abs().max()).item()


def _compare(ref_out, ref_leaves, out, leaves, g):
    """Outputs and the gradients of matching leaves under the same upstream gradient."""
    assert out.shape == ref_out.shape
    assert _rel(out.detach(), ref_out.detach()) < TOL
    ref_grads = torch.autograd.grad(ref_out, ref_leaves, g)
    grads = torch.autograd.grad(out, leaves, g)
    for a, b in zip(grads, ref_grads):
        assert a.shape == b.shape and _rel(a, b) < TOL


# every kernel form the branch has: the stem, the blocks' 3x3x3 (plain and strided), the shortcuts' 1x1x1 (strided and plain)
FORMS = [((3, 7, 7), (1, 2, 2), (1, 3, 3)), ((3, 3, 3), (1, 1, 1), (1, 1, 1)), ((3, 3, 3), (1, 2, 2), (1, 1, 1)),
         ((1, 1, 1), (1, 2, 2), (0, 0, 0)), ((1, 1, 1), (1, 1, 1), (0, 0, 0))]


@pytest.mark.parametrize("bias", [True, False])
@pytest.mark.parametrize("B,Ci,Co,H,W", [(2, 3, 5, 9, 7), (1, 4, 6, 8, 12), (1, 2, 3, 5, 6)])
@pytest.mark.parametrize("k,s,p", FORMS)
def test_folded_conv2d_is_conv3d_on_depth_2(k, s, p, B, Ci, Co, H, W, bias):
    from ebfi_amd import fold3d
    torch.manual_seed(11 + Ci + H)
    m = nn.Conv3d(Ci, Co, kernel_size=k, stride=s, padding=p, bias=bias).double()
    x = torch.randn(B, Ci, 2, H, W, dtype=torch.float64, requires_grad=True)
    ref = m(x)
    g = torch.randn_like(ref)
    w = m.weight.detach().clone().requires_grad_()
    b = m.bias.detach().clone().requires_grad_() if bias else None
    x1 = x.detach().clone().requires_grad_()
    x2, s2 = x1.reshape(B, 2 * Ci, H, W), s[1]
    if k[1] == 1 and s2 != 1:                            # as fold3d.conv3d_d2: subsample first, then 1x1
        x2, s2 = x2[:, :, ::s2, ::s2], 1
    y2 = F.conv2d(x2, fold3d.fold_conv3d_weight(w), fold3d._rep2(b) if bias else None, s2, p[1])
    out = y2.view(B, Co, 2, y2.shape[-2], y2.shape[-1])
    _compare(ref, [m.weight, x] + ([m.bias] if bias else []), out, [w, x1] + ([b] if bias else []), g)


@pytest.mark.parametrize("bias", [True, False])
@pytest.mark.parametrize("B,Ci,Co,H,W", [(2, 3, 5, 5, 7), (1, 4, 2, 4, 6), (1, 2, 3, 1, 3)])
def test_folded_conv2d_and_pixel_shuffle_is_conv_transpose3d_on_depth_2(B, Ci, Co, H, W, bias):
    from ebfi_amd import fold3d
    torch.manual_seed(5 + Ci + W)
    m = nn.ConvTranspose3d(Ci, Co, kernel_size=(3, 4, 4), stride=(1, 2, 2), padding=(1, 1, 1), bias=bias).double()
    x = torch.randn(B, Ci, 2, H, W, dtype=torch.float64, requires_grad=True)
    ref = m(x)
    g = torch.randn_like(ref)
    w = m.weight.detach().clone().requires_grad_()
    b = m.bias.detach().clone().requires_grad_() if bias else None
    x1 = x.detach().clone().requires_grad_()
    y2 = F.conv2d(x1.reshape(B, 2 * Ci, H, W), fold3d.fold_conv_transpose3d_weight(w), fold3d._rep8(b) if bias else None, 1, 1)
    out = F.pixel_shuffle(y2, 2).view(B, Co, 2, 2 * H, 2 * W)
    _compare(ref, [m.weight, x] + ([m.bias] if bias else []), out, [w, x1] + ([b] if bias else []), g)


@pytest.mark.parametrize("B,c0,H,W", [(2, 3, 5, 7), (1, 8, 4, 6)])
def test_fuse_weight_on_depth_minor_channels_is_the_fuse_on_cat_unbind(B, c0, H, W):
    from ebfi_amd.model import UNet3d_18
    torch.manual_seed(3 + c0)
    w = torch.randn(c0, 2 * c0, 1, 1, dtype=torch.float64, requires_grad=True)
    y = torch.randn(B, c0, 2, H, W, dtype=torch.float64, requires_grad=True)
    ref = F.conv2d(torch.cat(torch.unbind(y, 2), 1), w)
    g = torch.randn_like(ref)
    w1, y1 = w.detach().clone().requires_grad_(), y.detach().clone().requires_grad_()
    out = F.conv2d(y1.reshape(B, 2 * c0, H, W), UNet3d_18._fuse_weight_on_depth_minor_channels(w1))
    _compare(ref, [w, y], out, [w1, y1], g)


# ------------------------------------------------------------------------------------------------ the GPU test's case table
def test_case_table_covers_the_dispatch_classes():
    assert len({c.id for c in stages.CASES}) == len(stages.CASES)
    assert all(0 <= c.seed <= 255 and c.B in (1, 2) for c in stages.CASES)
    kinds = [c.kind for c in stages.CASES]
    assert set(kinds) == {"stem", "block", "conv3d", "up", "tail", "unet"}
    blocks = [c.args for c in stages.CASES if c.kind == "block"]
    assert any(a[0] == a[1] and a[2] == 1 for a in blocks) and any(a[2] == 2 for a in blocks) and \
        any(a[0] != a[1] and a[2] == 1 for a in blocks)
    # folded input channels of the blocks' and decoder stages' 3x3 layers: 32, 48 (data-gradient threshold), 64, 96, and 2 * 96
    folded = {2 * a for c in stages.CASES if c.kind == "block" for a in c.args[:2]} | \
        {2 * c.args[0] for c in stages.CASES if c.kind in ("conv3d", "up")}
    assert {32, 48, 64, 96, 192} <= folded
    sizes = {(c.H, c.W) for c in stages.CASES}
    assert {(4, 8), (8, 12), (5, 6), (9, 7), (2, 2), (16, 16), (16, 24)} <= sizes
    ups = [c for c in stages.CASES if c.kind == "up"]
    assert any(c.W % 2 == 0 for c in ups) and any(c.W % 2 == 1 for c in ups)


@pytest.mark.parametrize("case", stages.CASES, ids=[c.id for c in stages.CASES])
def test_recorded_seed_keeps_every_activation_off_its_kink(case):
    """What the GPU test relies on, checked on the reference alone: with the recorded seed every ReLU / LeakyReLU pre-activation
    of the float64 reference has |z| >= KINK * max|z|, so no device rounding can pick another subgradient."""
    ref = stages.build_reference(case, backward=False)
    want = {"stem": 1, "block": 2, "conv3d": 1, "up": 1, "tail": 2}.get(case.kind)
    assert ref.n_act >= 1 and (want is None or ref.n_act == want)        # every activation of the stage was seen
    assert ref.kink >= stages.KINK, (case.id, case.seed, ref.kink)
    assert torch.isfinite(ref.out).all() and ref.out.abs().max() > 1e-2
