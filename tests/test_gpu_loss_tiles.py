"""csrc/laploss.hip, the LDS-tiled difference pyramid, at sizes where a tiling can go wrong: the pyramid through
ebfi_laploss_forward / ebfi_laploss_backward against the operator-by-operator LaplacianLoss on the GPU (gauss5_fwd /
gauss5_bwd of csrc/imgops.hip through autograd), fed the same difference planes a - t against a zero target.

The gradient is compared bit for bit (it is 2^l * coef * sign(lap_l) carried through the adjoints, and the adjoints of
both paths add the same terms in the same order); the value at the tolerance of
test_laplacian_difference_pyramid_vs_operator_formulation (2e-5 relative: the partial sums are added in another order)."""
import pytest
import torch

pytestmark = pytest.mark.gpu

# (H, W, levels): 32x32 is the smallest legal size at 5 levels (coarsest blurred level 4x4: every pixel is a border
# pixel); 80x112 is several tiles with ragged last tiles in both directions; at 4x6 / 2 levels the reflection reaches
# the opposite border.
SHAPES = [(32, 32, 5), (32, 48, 5), (80, 112, 5), (4, 6, 2)]


def _pyramid(a, b, t, ca, cb, levels):
    from ebfi_amd import _native as N
    lib = N.lib()
    B, C, H, W = a.shape
    ppt = B * C
    n = 2 if b is not None else 1
    ws = torch.empty(int(lib.ebfi_laploss_workspace_floats(n * ppt, H, W, levels)), dtype=torch.float32, device=a.device)
    partial = torch.empty(int(lib.ebfi_laploss_partials(n * ppt, H, W, levels)), dtype=torch.float32, device=a.device)
    st = N.stream_ptr(a.device)
    N.check(lib.ebfi_laploss_forward(N.ptr(a), N.ptr(b) if b is not None else None, N.ptr(t), ca, cb, N.ptr(ws), N.ptr(partial),
                                     ppt, H, W, levels, st), "ebfi_laploss_forward")
    value = partial.sum()
    g = torch.ones(1, dtype=torch.float32, device=a.device)
    out = torch.empty((n * B, C, H, W), dtype=torch.float32, device=a.device)
    N.check(lib.ebfi_laploss_backward(N.ptr(g), N.ptr(ws), N.ptr(out), n * ppt, H, W, levels, st), "ebfi_laploss_backward")
    return value, out


def _operators(diffs, coefs, levels):
    from ebfi_amd.loss import LaplacianLoss
    lap = LaplacianLoss().cuda()
    lap.lap.max_level = levels
    leaves = [d.clone().requires_grad_() for d in diffs]
    value = sum(c * lap(d, torch.zeros_like(d)) for c, d in zip(coefs, leaves))
    value.backward()
    return value.detach(), torch.cat([d.grad for d in leaves])


@pytest.mark.parametrize("C", [3, 1])
@pytest.mark.parametrize("two", [False, True])
@pytest.mark.parametrize("H,W,levels", SHAPES)
def test_tiled_pyramid_vs_gpu_operator_formulation(H, W, levels, two, C):
    torch.manual_seed(100 * H + W + 7 * C + two)
    a, b, t = (torch.rand(1, C, H, W, device="cuda") for _ in range(3))
    a[:, :, :2, :3] = t[:, :, :2, :3]                        # exactly matching patch: zero differences
    ca, cb = 0.1, 1.0
    value, grad = _pyramid(a, b if two else None, t, ca, cb, levels)
    diffs = [a - t, b - t] if two else [a - t]
    ref_value, ref_grad = _operators(diffs, (ca, cb), levels)
    bad = int((grad.view(torch.int32) != ref_grad.view(torch.int32)).sum().item())
    rel = abs(value.item() - ref_value.item()) / abs(ref_value.item())
    print("laploss %dx%d L=%d two=%d C=%d: %d of %d gradient elements differ, value rel %.2e"
          % (H, W, levels, two, C, bad, grad.numel(), rel))
    assert torch.isfinite(grad).all()
    assert bad == 0
    assert rel <= 2e-5


def test_tiled_pyramid_carries_a_nan_to_the_loss():
    torch.manual_seed(3)
    a, b, t = (torch.rand(1, 3, 32, 48, device="cuda") for _ in range(3))
    b[0, 1, 17, 40] = float("nan")
    value, _ = _pyramid(a, b, t, 1.0, 0.1, 5)
    assert not torch.isfinite(value).item()
    value, _ = _pyramid(a, None, t, 1.0, 0.1, 5)           # the first prediction alone is clean
    assert torch.isfinite(value).item()

