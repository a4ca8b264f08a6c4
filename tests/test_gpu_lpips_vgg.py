"""ebfi_amd.lpips.VggLPIPS (ebfi_lpips_vgg: prologue, 13 exact-fp32 convolutions, tap kernels, finalize) against the float64
restatement of lpips_vgg_ref, per pair and per layer.

The bar is relative only -- |got - want| <= bar * want with want > 0 -- and is measured, not chosen: a module fixture evaluates
every case of the table in float32 and in float64 on the CPU, takes per kind the worst relative layer error of the float32
evaluation and multiplies it by 10 (the kernels sum K = 576 .. 4608 products in another order than the CPU does).  The totals
are held to the same bar.  The measured device errors are printed before they are asserted (profiles/lpips_vgg.md records them).

Plus: normalize=False, strided views, NaN / Inf isolation per pair, bit-reproducibility, chunking, no torch convolution or
pooling on the path, the perceptual_loss shim and an infer_ours.py --lpips_net vgg run."""
import importlib.util
import os

import numpy as np
import pytest
import torch
import yaml

from lpips_vgg_ref import ref_lpips, write_weights

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
PKG = os.path.join(ROOT, "ebfi-be_amd")

CASES = [
    (1, 3, 16, 16, "random"),        # the smallest size, 1 x 1 at the last tap
    (2, 1, 17, 19, "unclamped"),     # floor pooling drops a row and a column at the first pool
    (2, 3, 31, 45, "near"),          # odd at every level: 31-15-7-3-1
    (3, 3, 33, 47, "unclamped"),
    (5, 1, 48, 80, "random"),
    (1, 3, 64, 96, "near"),
    (1, 3, 128, 272, "random"),      # more than one tile in both directions
]
FACTOR = 10.0


def _pair(n, c, h, w, seed, kind="random"):
    """The kinds of test_gpu_lpips (drawn on the CPU, so that the yardstick needs no device)."""
    g = torch.Generator().manual_seed(seed)
    target = torch.rand(n, c, h, w, generator=g)
    if kind == "near":                                   # the squared difference cancels most of the features
        pred = target + 1e-3 * torch.randn(n, c, h, w, generator=g)
    elif kind == "unclamped":                            # a model output, not clipped to [0, 1]
        pred = target + 0.4 * torch.randn(n, c, h, w, generator=g)
    else:
        pred = torch.rand(n, c, h, w, generator=g)
    return pred, target


@pytest.fixture(scope="module")
def weights(tmp_path_factory):
    return write_weights(tmp_path_factory.mktemp("lpips_vgg"), seed=0)


@pytest.fixture(scope="module")
def vgg(weights):
    from ebfi_amd.lpips import load_vgg_lpips
    lin_path, backbone_path, _ = weights
    return load_vgg_lpips(lin_path, backbone_path, device="cuda")


@pytest.fixture(scope="module")
def yardstick(weights):
    """Per case the inputs and the float64 layer terms, and per kind the bar: 10 x the worst relative layer error of the float32
    evaluation of the same restatement.  Computed once; nothing below changes it."""
    _, _, (ws, bs, heads) = weights
    cases, worst = {}, {}
    for case in CASES:
        n, c, h, w, kind = case
        pred, target = _pair(n, c, h, w, seed=n * 1000 + h, kind=kind)
        want, want_layers = ref_lpips(pred, target, ws, bs, heads)
        _, f32_layers = ref_lpips(pred, target, ws, bs, heads, dtype=torch.float32)
        assert torch.all(want_layers > 0)
        rel = ((f32_layers.double() - want_layers).abs() / want_layers).max().item()
        worst[kind] = max(worst.get(kind, 0.0), rel)
        cases[case] = (pred, target, want, want_layers)
    bars = {kind: FACTOR * v for kind, v in worst.items()}
    for kind in sorted(bars):
        print("lpips_vgg yardstick: kind %-9s float32-CPU worst relative layer error %.3e -> bar %.3e" % (kind, worst[kind], bars[kind]))
    assert all(0 < b < 1e-2 for b in bars.values()), bars       # (a float32 evaluation that were this far off would bar nothing)
    return cases, bars


def _compare(got, got_layers, want, want_layers, bar, label):
    got, got_layers = got.cpu().double(), got_layers.cpu().double()
    assert got.shape == want.shape and got_layers.shape == want_layers.shape
    assert torch.all(want > 0) and torch.all(want_layers > 0)
    rel_layers = ((got_layers - want_layers).abs() / want_layers).max().item()
    rel_total = ((got - want).abs() / want).max().item()
    print("lpips_vgg device error: %s worst relative error layers %.3e total %.3e (bar %.3e)" % (label, rel_layers, rel_total, bar))
    assert torch.all((got_layers - want_layers).abs() <= bar * want_layers), (got_layers, want_layers, bar)
    assert torch.all((got - want).abs() <= bar * want), (got, want, bar)


@pytest.mark.gpu
@pytest.mark.parametrize("case", CASES, ids=lambda c: "%dx%dx%dx%d-%s" % c)
def test_lpips_vgg_matches_the_restatement(vgg, yardstick, case):
    cases, bars = yardstick
    pred, target, want, want_layers = cases[case]
    got, got_layers = vgg(pred.cuda(), target.cuda(), per_layer=True)
    torch.cuda.synchronize()
    _compare(got, got_layers, want, want_layers, bars[case[4]], "%dx%dx%dx%d %s" % case)
    assert torch.equal(vgg(pred.cuda(), target.cuda()), got)            # (without per_layer: the same totals)


@pytest.mark.gpu
def test_without_normalize_the_images_are_taken_as_minus_one_to_one(vgg, weights, yardstick):
    _, _, (ws, bs, heads) = weights
    pred, target = _pair(2, 3, 20, 27, seed=7, kind="unclamped")
    pred, target = pred * 2 - 1, target * 2 - 1
    want, want_layers = ref_lpips(pred, target, ws, bs, heads, normalize=False)
    got, got_layers = vgg(pred.cuda(), target.cuda(), normalize=False, per_layer=True)
    _compare(got, got_layers, want, want_layers, yardstick[1]["unclamped"], "normalize=False")
    other = vgg(pred.cuda(), target.cuda(), normalize=True)
    assert not torch.equal(other, got)


@pytest.mark.gpu
def test_strided_views_equal_their_contiguous_copies(vgg, weights, yardstick):
    _, _, (ws, bs, heads) = weights
    g = torch.Generator().manual_seed(11)
    big_p = torch.rand(4, 5, 40, 50, generator=g).cuda()
    big_t = torch.rand(3, 4, 37, 45, generator=g).cuda()
    pred = big_p[1:4, 1:4, 3:36, 5:44]                   # channel, row and image strides of a larger tensor
    target = big_t[:, 0:3, 2:35, 4:43]
    assert not pred.is_contiguous() and not target.is_contiguous() and pred.stride(3) == 1
    got, got_layers = vgg(pred, target, per_layer=True)
    flat, flat_layers = vgg(pred.contiguous(), target.contiguous(), per_layer=True)
    assert torch.equal(got, flat) and torch.equal(got_layers, flat_layers)
    want, want_layers = ref_lpips(pred.cpu(), target.cpu(), ws, bs, heads)
    _compare(got, got_layers, want, want_layers, yardstick[1]["random"], "strided")
    # one channel picked out of a three-channel tensor (channel stride of the parent, no copy)
    p1, t1 = big_p[:2, 2:3, :32, :40], big_t[:2, 1:2, :32, :40]
    assert not p1.is_contiguous() and p1.shape == t1.shape
    a, la = vgg(p1, t1, per_layer=True)
    b, lb = vgg(p1.contiguous(), t1.contiguous(), per_layer=True)
    assert torch.equal(a, b) and torch.equal(la, lb) and torch.all(a > 0)


@pytest.mark.gpu
def test_non_finite_values_stay_in_their_pair(vgg):
    pred, target = _pair(4, 3, 17, 21, seed=5)
    pred, target = pred.cuda(), target.cuda()
    clean, clean_layers = vgg(pred, target, per_layer=True)
    pred, target = pred.clone(), target.clone()
    pred[1, 2, 10, 20] = float("nan")
    target[2, 0, 16, 5] = float("inf")                  # the last row: the first pool drops it
    got, layers = vgg(pred, target, per_layer=True)
    torch.cuda.synchronize()
    assert torch.isnan(got[1]) and torch.isnan(got[2])
    assert torch.equal(got[[0, 3]], clean[[0, 3]]) and torch.all(clean > 0)
    assert torch.isnan(layers[1]).all() and torch.isnan(layers[2]).all()
    assert torch.equal(layers[[0, 3]], clean_layers[[0, 3]])


@pytest.mark.gpu
def test_two_calls_are_bit_identical(vgg):
    pred, target = _pair(3, 3, 33, 47, seed=3, kind="near")
    pred, target = pred.cuda(), target.cuda()
    a, la = vgg(pred, target, per_layer=True)
    b, lb = vgg(pred, target, per_layer=True)
    torch.cuda.synchronize()
    assert torch.equal(a, b) and torch.equal(la, lb) and torch.all(a > 0)


@pytest.mark.gpu
def test_chunking_changes_no_bit(vgg):
    pred, target = _pair(5, 3, 20, 24, seed=13, kind="unclamped")
    pred, target = pred.cuda(), target.cuda()
    whole, whole_layers = vgg(pred, target, per_layer=True)
    assert vgg._chunk(5, 3, 20, 24) == 5
    vgg.chunk = 2
    try:
        assert vgg._chunk(5, 3, 20, 24) == 2
        parts, parts_layers = vgg(pred, target, per_layer=True)
    finally:
        vgg.chunk = None
    assert torch.equal(whole, parts) and torch.equal(whole_layers, parts_layers) and torch.all(whole > 0)
    # the budget: one workspace stays under it, and a 720 x 1280 load is split
    from ebfi_amd import _native as N
    from ebfi_amd.lpips import VGG_WORKSPACE_BUDGET
    k = vgg._chunk(16, 3, 720, 1280)
    assert 1 <= k < 16 and N.lib().ebfi_lpips_vgg_workspace(k, 3, 720, 1280) <= VGG_WORKSPACE_BUDGET


@pytest.mark.gpu
def test_no_torch_convolution_or_pooling_on_the_path(vgg, monkeypatch):
    import torch.nn.functional as F
    pred, target = _pair(2, 3, 32, 32, seed=9)
    pred, target = pred.cuda(), target.cuda()
    want = vgg(pred, target).cpu()

    def refuse(*a, **k):
        raise AssertionError("torch convolution / pooling called on the LPIPS path")

    for name in ("conv2d", "max_pool2d", "relu"):
        monkeypatch.setattr(F, name, refuse)
    monkeypatch.setattr(torch, "conv2d", refuse)
    monkeypatch.setattr(torch, "max_pool2d", refuse)
    got = vgg(pred, target).cpu()
    assert torch.equal(got, want) and torch.all(want > 0)


@pytest.mark.gpu
def test_perceptual_loss_shim(vgg, weights, yardstick):
    from loss import perceptual_loss
    lin_path, backbone_path, (ws, bs, heads) = weights
    loss = perceptual_loss(weight=2.0, net="vgg", lin_path=lin_path, backbone_path=backbone_path)
    pred, target = _pair(3, 3, 24, 28, seed=21)
    v = loss(pred.cuda(), target.cuda())
    assert v.dim() == 0 and isinstance(v.item(), float)
    assert v.item() == pytest.approx(2.0 * float(vgg(pred.cuda(), target.cuda()).mean()), rel=1e-6)
    want = 2.0 * float(ref_lpips(pred, target, ws, bs, heads)[0].mean())
    assert want > 0 and abs(v.item() - want) <= yardstick[1]["random"] * want + 1e-6 * want     # (+ the float32 mean and product)


# ------------------------------------------------------------------ infer_ours.py --lpips_net vgg
@pytest.fixture(scope="module")
def cli():
    spec = importlib.util.spec_from_file_location("ebfi_infer_ours_gpu_lpips_vgg", os.path.join(PKG, "infer_ours.py"))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod


@pytest.mark.gpu
def test_infer_ours_scores_lpips_vgg(cli, golden_dir, tmp_path, capsys, weights, yardstick):
    from ebfi_amd import clipdata
    from test_gpu_infer_lpips import _setup
    from test_lpips_host import ref_lpips as alex_ref_lpips
    from test_lpips_host import write_weights as write_alex_weights
    clip, args = _setup(tmp_path, golden_dir)
    lin_path, backbone_path, (ws, bs, heads) = weights
    out = str(tmp_path / "out")
    cli.main(args + ["--output_path", out, "--lpips_net", "vgg", "--lpips_lin", lin_path, "--lpips_backbone", backbone_path])
    err = capsys.readouterr().err
    assert "LPIPS is not computed" not in err and "lpips (vgg)" in err

    res = np.load(os.path.join(out, "clip0.npz", "restored.npz"))
    assert res["restored"].shape == (2, 8, 3, 48, 64) and res["lpips"].shape == (2, 8)
    assert str(res["lpips_net"]) == "vgg"
    data = clipdata.ClipDataset(clip, time_bins=4, frames_per_period=8, frames_per_blurry=3, exposure_method="Fixed", crop=None,
                                crop_mode="center", device="cuda", seed=123, noise=None)
    want = np.concatenate([ref_lpips(torch.from_numpy(res["restored"][load]),
                                     data.__getitem__(period, seed=123 + period)["SeqLatentF"][0, 0].cpu(), ws, bs, heads)[0].numpy()
                           for load, period in enumerate((0, 1))])
    got = res["lpips"].ravel().astype(np.float64)
    bar = yardstick[1]["random"]
    assert np.all(want > 0) and want.std() > 0
    print("lpips_vgg device error: infer_ours worst relative error %.3e (bar %.3e)" % (np.max(np.abs(got - want) / want), bar))
    assert np.all(np.abs(got - want) <= bar * want), (got, want)

    # the three yml files: the reference's key, whatever the net (a yml value is the float64 mean of float32 scores)
    doc = yaml.safe_load(open(os.path.join(out, "clip0.npz", "inference.yml")))
    assert set(doc["evaluation results"]) == {"mse", "psnr", "ssim", "lpips"}
    assert abs(doc["evaluation results"]["lpips"] - want.mean()) <= bar * want.mean()
    all_ = yaml.safe_load(open(os.path.join(out, "inference_all.yml")))
    assert all_["breakdown results for each data"]["lpips"] == {"clip0.npz": doc["evaluation results"]["lpips"]}
    assert abs(all_["mean results for the whole data"]["lpips"] - want.mean()) <= bar * want.mean()
    all_step = yaml.safe_load(open(os.path.join(out, "inference_all_step.yml")))
    assert all_step["breakdown results for each data"] == {"psnr": {"clip0.npz": doc["evaluation step results"]["psnr"]}}

    # the same run with the default net: AlexNet's outputs, with no trace of the new flag
    alex_lin, alex_backbone, alex_weights = write_alex_weights(tmp_path)
    plain = str(tmp_path / "plain")
    cli.main(args + ["--output_path", plain, "--lpips_lin", alex_lin, "--lpips_backbone", alex_backbone])
    err = capsys.readouterr().err
    assert "lpips (" not in err and "LPIPS is not computed" not in err
    ref = np.load(os.path.join(plain, "clip0.npz", "restored.npz"))
    assert sorted(ref.files) == sorted(["restored", "blurry", "exposure_duty", "timestamps", "period", "psnr", "ssim", "mse", "lpips"])
    for k in ("restored", "blurry", "psnr", "ssim", "mse"):
        assert np.array_equal(res[k], ref[k]), k
    want0 = np.concatenate([alex_ref_lpips(torch.from_numpy(ref["restored"][load]),
                                           data.__getitem__(period, seed=123 + period)["SeqLatentF"][0, 0].cpu(), *alex_weights)[0].numpy()
                            for load, period in enumerate((0, 1))])
    got0 = ref["lpips"].ravel().astype(np.float64)
    assert np.all(np.abs(got0 - want0) <= 1e-5 + 1e-4 * np.abs(want0)), (got0, want0)       # (the bar of test_gpu_infer_lpips)
    doc0 = yaml.safe_load(open(os.path.join(plain, "clip0.npz", "inference.yml")))
    assert set(doc0["evaluation results"]) == {"mse", "psnr", "ssim", "lpips"}
    for k in ("mse", "psnr", "ssim"):
        assert doc["evaluation results"][k] == doc0["evaluation results"][k]
    assert doc0["evaluation results"]["lpips"] != doc["evaluation results"]["lpips"]
