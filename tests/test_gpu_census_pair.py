"""ebfi_census_pair_* (csrc/imgops.hip): the two census terms of the training loss -- two predictions against one target -- in one
launch each way.  Per prediction the per-tile partial sums and the gradient are BIT-equal to the single-pair entry points
ebfi_census_forward / ebfi_census_backward (given the gradient scaled by the term's weight); the weighted loss, summed by the
node's own one-workgroup launch, is held to the CPU oracle at the bound of
tests/test_gpu_model.py::test_census_kernel_pair_vs_slice_formulation.  Shapes: (7, 9) has a 1 x 3 interior, (16, 16) is one
tile, (20, 37) and (37, 41) are ragged and put an image edge inside a halo."""
import os
import sys

import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from oracle import loss_ref  # noqa: E402

pytestmark = pytest.mark.gpu

SHAPES = [(7, 9), (16, 16), (20, 37), (37, 41)]
WEIGHTS = [(0.1, 1.0), (1.0, 0.1)]
B, C, G_IN = 2, 3, 0.37


def _rel(a, b):
    a, b = torch.as_tensor(a).float().cpu(), torch.as_tensor(b).float().cpu()
    return ((a - b).abs().max() / b.abs().max().clamp_min(1e-30)).item()


def _bits(t):
    return t.contiguous().view(torch.int32)


@pytest.fixture(scope="module")
def images():
    """Per shape: two predictions, the target, and the oracle's two census terms with their gradients (CPU, computed once)."""
    torch.manual_seed(21)
    out = {}
    for (H, W) in SHAPES:
        xa, xb, y = torch.rand(B, C, H, W), torch.rand(B, C, H, W), torch.rand(B, C, H, W)
        refs = []
        for x in (xa, xb):
            xr = x.clone().requires_grad_()
            l = loss_ref.census_loss(xr, y)
            l.backward()
            refs.append((l.item(), xr.grad))
        out[(H, W)] = (xa, xb, y, refs)
    return out


def _single(x, y, g_scaled):
    """(partials, gradient) of the single-pair entry points for one prediction; g_scaled: 1-element device gradient."""
    from ebfi_amd import _native as N
    lib = N.lib()
    Bn, Cn, H, W = x.shape
    partial = torch.empty(int(lib.ebfi_census_partials(Bn, H, W)), dtype=torch.float32, device=x.device)
    gx = torch.empty_like(x)
    st = N.stream_ptr(x.device)
    N.check(lib.ebfi_census_forward(N.ptr(x), N.ptr(y), N.ptr(partial), Bn, Cn, H, W, st), "ebfi_census_forward")
    N.check(lib.ebfi_census_backward(N.ptr(x), N.ptr(y), N.ptr(g_scaled), N.ptr(gx), Bn, Cn, H, W, st), "ebfi_census_backward")
    return partial, gx


def _pair(xa, xb, y, wa, wb, g):
    """(partials, loss, grad_a, grad_b) of the two-prediction entry points; xb may be None."""
    from ebfi_amd import _native as N
    lib = N.lib()
    Bn, Cn, H, W = xa.shape
    P = int(lib.ebfi_census_partials(Bn, H, W))
    partial = torch.full((2 * P,), -7.0, dtype=torch.float32, device=xa.device)
    loss = torch.empty((), dtype=torch.float32, device=xa.device)
    ga = torch.empty_like(xa)
    gb = torch.empty_like(xb) if xb is not None else None
    st = N.stream_ptr(xa.device)
    xbp, gbp = (N.ptr(xb), N.ptr(gb)) if xb is not None else (None, None)
    N.check(lib.ebfi_census_pair_forward(N.ptr(xa), xbp, N.ptr(y), wa, wb, N.ptr(partial), N.ptr(loss), Bn, Cn, H, W, st),
            "ebfi_census_pair_forward")
    N.check(lib.ebfi_census_pair_backward(N.ptr(xa), xbp, N.ptr(y), wa, wb, N.ptr(g), N.ptr(ga), gbp, Bn, Cn, H, W, st),
            "ebfi_census_pair_backward")
    return partial, loss, ga, gb


@pytest.mark.parametrize("two", [True, False], ids=["two", "one"])
@pytest.mark.parametrize("wa,wb", WEIGHTS)
@pytest.mark.parametrize("H,W", SHAPES)
def test_pair_is_bit_equal_to_the_single_pair_entry_points(images, H, W, wa, wb, two):
    xa, xb, y, _ = images[(H, W)]
    xa, xb, y = xa.cuda(), (xb.cuda() if two else None), y.cuda()
    g = torch.tensor([G_IN], dtype=torch.float32, device="cuda")
    partial, loss, ga, gb = _pair(xa, xb, y, wa, wb, g)
    P = partial.numel() // 2
    pa, sa = _single(xa, y, g * wa)                      # (fp32 product, as autograd forms the gradient of w * term)
    assert torch.equal(_bits(partial[:P]), _bits(pa))
    assert torch.equal(_bits(ga), _bits(sa))
    if two:
        pb, sb = _single(xb, y, g * wb)
        assert torch.equal(_bits(partial[P:]), _bits(pb))
        assert torch.equal(_bits(gb), _bits(sb))
    else:
        assert (partial[P:] == -7.0).all()               # one prediction: the second half is not touched
    again = _pair(xa, xb, y, wa, wb, g)
    for t, u in zip((partial, loss.reshape(1), ga, gb), (again[0], again[1].reshape(1), again[2], again[3])):
        assert (t is None and u is None) or torch.equal(_bits(t), _bits(u))


@pytest.mark.parametrize("two", [True, False], ids=["two", "one"])
@pytest.mark.parametrize("wa,wb", WEIGHTS)
@pytest.mark.parametrize("H,W", SHAPES)
def test_weighted_loss_and_gradients_against_the_oracle(images, H, W, wa, wb, two):
    from ebfi_amd.loss import census_pair
    xa, xb, y, refs = images[(H, W)]
    da = xa.cuda().requires_grad_()
    db = xb.cuda().requires_grad_() if two else None
    out = census_pair(da, db, y.cuda(), wa, wb)
    (out * 3.0).backward()
    ref = wa * refs[0][0] + (wb * refs[1][0] if two else 0.0)
    print("H=%d W=%d w=(%g, %g) two=%d: loss %.9g oracle %.9g" % (H, W, wa, wb, two, out.item(), ref))
    assert abs(out.item() - ref) <= 2e-6 + 1e-5 * abs(ref)
    assert _rel(da.grad, 3.0 * wa * refs[0][1]) < 5e-5
    if two:
        assert _rel(db.grad, 3.0 * wb * refs[1][1]) < 5e-5


def test_a_nan_in_one_prediction_stays_out_of_the_others_gradient(images):
    from ebfi_amd.loss import census_pair
    xa, xb, y, refs = images[(20, 37)]
    for bad in (0, 1):
        preds = [xa.clone(), xb.clone()]
        preds[bad][1, 2, 9, 17] = float("nan")
        da, db = preds[0].cuda().requires_grad_(), preds[1].cuda().requires_grad_()
        out = census_pair(da, db, y.cuda(), 0.1, 1.0)
        out.backward()
        assert torch.isnan(out).item()
        good, w = ((db, 1.0), (da, 0.1))[bad]
        assert torch.isfinite(good.grad).all()
        assert _rel(good.grad, w * refs[1 - bad][1]) < 5e-5
        assert torch.isnan((da, db)[bad].grad).any()

