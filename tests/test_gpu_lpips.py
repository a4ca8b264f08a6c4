"""ebfi_amd.lpips (ebfi_lpips_alex: the AlexNet trunk on fp32 MFMA, the distance and finalize kernels) against the float64
restatement of test_lpips_host, per pair and per layer, over sizes from the smallest AlexNet accepts to one 720 x 1280 pair, one
and three channels, near-identical pairs, unclamped predictions and strided views; plus NaN / Inf isolation per pair,
bit-reproducibility, no torch convolution or pooling on the path, and the perceptual_loss shim."""
import pytest
import torch

from test_lpips_host import ref_lpips, write_weights

ATOL, RTOL = 1e-5, 1e-4


@pytest.fixture(scope="module")
def alex(tmp_path_factory):
    from ebfi_amd.lpips import load_alex_lpips
    lin_path, backbone_path, (ws, bs, heads) = write_weights(tmp_path_factory.mktemp("lpips"), seed=0)
    return load_alex_lpips(lin_path, backbone_path, device="cuda"), (ws, bs, heads), (lin_path, backbone_path)


def _check(model_and_weights, pred, target, normalize=True):
    model, (ws, bs, heads), _ = model_and_weights
    got, got_layers = model(pred, target, normalize=normalize, per_layer=True)
    torch.cuda.synchronize()
    want, want_layers = ref_lpips(pred.cpu(), target.cpu(), ws, bs, heads, normalize=normalize)
    got, got_layers = got.cpu().double(), got_layers.cpu().double()
    assert got.shape == want.shape and got_layers.shape == want_layers.shape
    assert torch.all(want > 0)
    err = (got - want).abs()
    assert torch.all(err <= ATOL + RTOL * want.abs()), (got, want)
    err = (got_layers - want_layers).abs()
    assert torch.all(err <= ATOL + RTOL * want_layers.abs()), (got_layers, want_layers)
    return got


def _pair(n, c, h, w, seed, kind="random"):
    g = torch.Generator(device="cuda").manual_seed(seed)
    target = torch.rand(n, c, h, w, device="cuda", generator=g)
    if kind == "near":                                   # the squared difference cancels most of the features
        pred = target + 1e-3 * torch.randn(n, c, h, w, device="cuda", generator=g)
    elif kind == "unclamped":                            # a model output, not clipped to [0, 1]
        pred = target + 0.4 * torch.randn(n, c, h, w, device="cuda", generator=g)
    else:
        pred = torch.rand(n, c, h, w, device="cuda", generator=g)
    return pred, target


@pytest.mark.gpu
@pytest.mark.parametrize("n,c,h,w,kind", [
    (1, 3, 31, 31, "random"),
    (16, 1, 31, 31, "unclamped"),
    (5, 1, 64, 64, "random"),
    (5, 3, 64, 64, "near"),
    (5, 3, 97, 131, "unclamped"),
    (16, 1, 97, 131, "near"),
    (16, 3, 64, 64, "random"),
    (2, 3, 256, 256, "unclamped"),
    (1, 3, 720, 1280, "near"),
])
def test_lpips_matches_the_restatement(alex, n, c, h, w, kind):
    pred, target = _pair(n, c, h, w, seed=n * 1000 + h, kind=kind)
    _check(alex, pred, target)


@pytest.mark.gpu
def test_without_normalize_the_images_are_taken_as_minus_one_to_one(alex):
    pred, target = _pair(3, 3, 40, 52, seed=7, kind="unclamped")
    _check(alex, pred * 2 - 1, target * 2 - 1, normalize=False)


@pytest.mark.gpu
def test_strided_views_are_read_in_place(alex):
    g = torch.Generator(device="cuda").manual_seed(11)
    big_p = torch.rand(4, 5, 75, 90, device="cuda", generator=g)
    big_t = torch.rand(3, 4, 70, 83, device="cuda", generator=g)
    pred = big_p[1:4, 1:4, 3:68, 5:78]                   # channel, row and image strides of a larger tensor
    target = big_t[:, 0:3, 2:67, 4:77]
    assert not pred.is_contiguous() and not target.is_contiguous() and pred.stride(3) == 1
    got = _check(alex, pred, target)
    model = alex[0]
    assert torch.equal(model(pred, target).cpu().double(), got)
    # one channel picked out of a three-channel tensor (channel stride of the parent, no copy)
    _check(alex, big_p[:2, 2:3, :64, :80], big_t[:2, 1:2, :64, :80])


@pytest.mark.gpu
def test_non_finite_values_stay_in_their_pair(alex):
    model = alex[0]
    pred, target = _pair(4, 3, 66, 67, seed=5)
    clean = model(pred, target)
    pred, target = pred.clone(), target.clone()
    pred[1, 2, 10, 20] = float("nan")
    target[2, 0, 65, 30] = float("inf")                 # (row 65 lies outside every conv1 window: only the input check sees it)
    got = model(pred, target)
    torch.cuda.synchronize()
    assert torch.isnan(got[1]) and torch.isnan(got[2])
    assert torch.equal(got[[0, 3]], clean[[0, 3]])
    _, layers = model(pred, target, per_layer=True)
    assert torch.isnan(layers[1]).all() and torch.isnan(layers[2]).all() and torch.isfinite(layers[[0, 3]]).all()


@pytest.mark.gpu
def test_two_calls_are_bit_identical(alex):
    model = alex[0]
    pred, target = _pair(5, 3, 97, 131, seed=3, kind="near")
    a, la = model(pred, target, per_layer=True)
    b, lb = model(pred, target, per_layer=True)
    torch.cuda.synchronize()
    assert torch.equal(a, b) and torch.equal(la, lb)


@pytest.mark.gpu
def test_no_torch_convolution_or_pooling_on_the_path(alex, monkeypatch):
    import torch.nn.functional as F
    model = alex[0]
    pred, target = _pair(2, 3, 64, 64, seed=9)
    want = model(pred, target).cpu()

    def refuse(*a, **k):
        raise AssertionError("torch convolution / pooling called on the LPIPS path")

    for name in ("conv2d", "max_pool2d", "relu"):
        monkeypatch.setattr(F, name, refuse)
    monkeypatch.setattr(torch, "conv2d", refuse)
    monkeypatch.setattr(torch, "max_pool2d", refuse)
    got = model(pred, target).cpu()
    assert torch.equal(got, want)


@pytest.mark.gpu
def test_perceptual_loss_shim(alex):
    from loss import perceptual_loss
    model, (ws, bs, heads), (lin_path, backbone_path) = alex
    loss = perceptual_loss(net="alex", lin_path=lin_path, backbone_path=backbone_path)
    pred, target = _pair(3, 3, 48, 56, seed=21)
    v = loss(pred, target)
    assert v.dim() == 0 and isinstance(v.item(), float)
    assert v.item() == pytest.approx(float(model(pred, target).mean()), rel=1e-6)
    # two channels: the mean of the per-channel calls, each channel read as three
    pred2, target2 = _pair(1, 2, 40, 40, seed=22)
    want = sum(float(ref_lpips(pred2[:, i:i + 1].cpu(), target2[:, i:i + 1].cpu(), ws, bs, heads)[0][0]) for i in range(2)) / 2
    got = perceptual_loss(weight=2.0, lin_path=lin_path, backbone_path=backbone_path)(pred2, target2).item()
    assert abs(got - 2.0 * want) <= 2.0 * (ATOL + RTOL * want)
