"""LPIPS (AlexNet, v0.1) without a GPU: a float64 torch-CPU restatement of the definition (include/ebfi_hip.h, ebfi_lpips_alex)
checked on hand-built cases, the weight loader's refusals, the C entry points' argument errors, the perceptual_loss shim and
the infer_ours.py flags.  The restatement and the random-trunk writer are shared with the GPU tests."""
import ctypes
import importlib.util
import os

import numpy as np
import pytest
import torch
import torch.nn.functional as F

from ebfi_amd import _native as N

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
PKG = os.path.join(ROOT, "ebfi-be_amd")
LIN_FIXTURE = os.path.join(ROOT, "tests", "golden", "lpips_alex_v01_lin.npz")

CONV_SHAPES = ((64, 3, 11, 11), (192, 64, 5, 5), (384, 192, 3, 3), (256, 384, 3, 3), (256, 256, 3, 3))
TRUNK_KEYS = ("features.0", "features.3", "features.6", "features.8", "features.10")
SHIFT = (-0.030, -0.088, -0.188)
SCALE = (0.458, 0.448, 0.450)


# ------------------------------------------------------------------ weights
def random_trunk(seed=0):
    """A seeded AlexNet trunk: He-scaled weights and small positive biases, so that every ReLU layer stays active."""
    g = torch.Generator().manual_seed(seed)
    ws, bs = [], []
    for shape in CONV_SHAPES:
        fan_in = shape[1] * shape[2] * shape[3]
        ws.append(torch.randn(shape, generator=g) * (2.0 / fan_in) ** 0.5)
        bs.append(0.01 + 0.05 * torch.rand(shape[0], generator=g))
    return ws, bs


def fixture_heads():
    z = np.load(LIN_FIXTURE)
    return [torch.from_numpy(z["lin%d" % l].astype(np.float32)) for l in range(5)]


def write_weights(tmp_path, seed=0):
    """(lin_path, backbone_path, (ws, bs, heads)): the fixture's heads in the reference's alex.pth layout and a random trunk in
    torchvision's AlexNet layout (with a classifier entry, which the loader ignores)."""
    ws, bs = random_trunk(seed)
    heads = fixture_heads()
    trunk = {}
    for key, w, b in zip(TRUNK_KEYS, ws, bs):
        trunk[key + ".weight"], trunk[key + ".bias"] = w, b
    trunk["classifier.1.weight"] = torch.zeros(4, 9216)
    lin = {"lin%d.model.1.weight" % l: h.reshape(1, -1, 1, 1) for l, h in enumerate(heads)}
    lin_path, backbone_path = str(tmp_path / "alex.pth"), str(tmp_path / "alexnet-owt.pth")
    torch.save(lin, lin_path)
    torch.save(trunk, backbone_path)
    return lin_path, backbone_path, (ws, bs, heads)


# ------------------------------------------------------------------ the float64 restatement
def ref_features(x, ws, bs, normalize=True):
    """The five ReLU maps of the AlexNet trunk for [N, 3, H, W] float64 images."""
    x = x.double()
    if normalize:
        x = 2 * x - 1
    shift = torch.tensor(SHIFT, dtype=torch.float64).view(1, 3, 1, 1)
    scale = torch.tensor(SCALE, dtype=torch.float64).view(1, 3, 1, 1)
    x = (x - shift) / scale
    w = [t.double() for t in ws]
    b = [t.double() for t in bs]
    f1 = F.relu(F.conv2d(x, w[0], b[0], stride=4, padding=2))
    f2 = F.relu(F.conv2d(F.max_pool2d(f1, 3, 2), w[1], b[1], padding=2))
    f3 = F.relu(F.conv2d(F.max_pool2d(f2, 3, 2), w[2], b[2], padding=1))
    f4 = F.relu(F.conv2d(f3, w[3], b[3], padding=1))
    f5 = F.relu(F.conv2d(f4, w[4], b[4], padding=1))
    return [f1, f2, f3, f4, f5]


def ref_distances(feats0, feats1, heads):
    """[N, L] layer terms: mean over the pixels of sum_c w_c (u0_c - u1_c)^2, u = f / (||f||_c + 1e-10)."""
    out = []
    for f0, f1, h in zip(feats0, feats1, heads):
        u0 = f0 / (torch.sqrt((f0 ** 2).sum(1, keepdim=True)) + 1e-10)
        u1 = f1 / (torch.sqrt((f1 ** 2).sum(1, keepdim=True)) + 1e-10)
        d = (h.double().view(1, -1, 1, 1) * (u0 - u1) ** 2).sum(1)
        out.append(d.mean((1, 2)))
    return torch.stack(out, 1)


def ref_lpips(pred, target, ws, bs, heads, normalize=True):
    """(lpips [N], layers [N, 5]) in float64 of an [N, C, H, W] pair, C in {1, 3} (one channel read as three)."""
    pred, target = torch.as_tensor(pred).cpu(), torch.as_tensor(target).cpu()
    if pred.shape[1] == 1:
        pred, target = pred.expand(-1, 3, -1, -1), target.expand(-1, 3, -1, -1)
    layers = ref_distances(ref_features(pred, ws, bs, normalize), ref_features(target, ws, bs, normalize), heads)
    return layers.sum(1), layers


# ------------------------------------------------------------------ the restatement on hand-built cases
def test_identical_images_score_zero():
    ws, bs = random_trunk(1)
    x = torch.rand(2, 3, 40, 48, generator=torch.Generator().manual_seed(3))
    total, layers = ref_lpips(x, x.clone(), ws, bs, fixture_heads())
    assert total.shape == (2,) and layers.shape == (2, 5)
    assert torch.all(total == 0) and torch.all(layers == 0)


def test_single_pixel_difference_of_one_layer():
    # one layer of 2 channels on 2 x 2 pixels; only pixel (0, 0) differs: u0 = (0.6, 0.8), u1 = (0.8, 0.6)
    f0 = torch.ones(1, 2, 2, 2, dtype=torch.float64)
    f1 = f0.clone()
    f0[0, :, 0, 0] = torch.tensor([3.0, 4.0])
    f1[0, :, 0, 0] = torch.tensor([4.0, 3.0])
    w = torch.tensor([0.5, 2.0])
    d = ref_distances([f0], [f1], [w])
    want = (0.5 + 2.0) * (1.0 / (5.0 + 1e-10)) ** 2 / 4      # (|u0_c - u1_c| = 1 / (5 + eps) in both channels)
    assert d.shape == (1, 1) and abs(float(d[0, 0]) - want) < 1e-15
    # scaling a feature vector does not change its unit vector
    assert float(ref_distances([f0 * 7.0], [f0], [w])[0, 0]) < 1e-12


def test_restatement_shapes_at_the_smallest_size():
    ws, bs = random_trunk(0)
    feats = ref_features(torch.rand(1, 3, 31, 31), ws, bs)
    assert [tuple(f.shape[1:]) for f in feats] == [(64, 7, 7), (192, 3, 3), (384, 1, 1), (256, 1, 1), (256, 1, 1)]
    assert all(float(f.amax()) > 0 for f in feats)      # (the random trunk keeps every layer active)
    with pytest.raises(RuntimeError):
        ref_features(torch.rand(1, 3, 30, 30), ws, bs)


def test_one_channel_is_read_as_three():
    ws, bs = random_trunk(2)
    g = torch.Generator().manual_seed(4)
    a, b = torch.rand(1, 1, 33, 35, generator=g), torch.rand(1, 1, 33, 35, generator=g)
    one, _ = ref_lpips(a, b, ws, bs, fixture_heads())
    three, _ = ref_lpips(a.repeat(1, 3, 1, 1), b.repeat(1, 3, 1, 1), ws, bs, fixture_heads())
    assert float(one[0]) > 0 and float(one[0]) == float(three[0])


# ------------------------------------------------------------------ the weight loader
def test_loader_reads_both_files(tmp_path):
    from ebfi_amd.lpips import read_alex_weights
    lin_path, backbone_path, (ws, bs, heads) = write_weights(tmp_path)
    rw, rb, rh = read_alex_weights(lin_path, backbone_path)
    for got, want in zip(rw + rb + rh, ws + bs + heads):
        assert got.dtype == torch.float32 and torch.equal(got, want.reshape(got.shape))
    assert [tuple(h.shape) for h in rh] == [(64,), (192,), (384,), (256,), (256,)]


def test_loader_names_a_missing_key(tmp_path):
    from ebfi_amd.lpips import read_alex_weights
    lin_path, backbone_path, _ = write_weights(tmp_path)
    sd = torch.load(backbone_path, weights_only=True)
    sd["features.9.weight"] = sd.pop("features.8.weight")
    torch.save(sd, backbone_path)
    with pytest.raises(KeyError, match="features.8.weight"):
        read_alex_weights(lin_path, backbone_path)
    lin_path, backbone_path, _ = write_weights(tmp_path)
    lin = torch.load(lin_path, weights_only=True)
    del lin["lin3.model.1.weight"]
    torch.save(lin, lin_path)
    with pytest.raises(KeyError, match="lin3.model.1.weight"):
        read_alex_weights(lin_path, backbone_path)


def test_loader_names_a_wrong_shape(tmp_path):
    from ebfi_amd.lpips import read_alex_weights
    lin_path, backbone_path, _ = write_weights(tmp_path)
    sd = torch.load(backbone_path, weights_only=True)
    sd["features.3.bias"] = torch.zeros(191)
    torch.save(sd, backbone_path)
    with pytest.raises(ValueError, match=r"features\.3\.bias.*\(191,\).*\(192,\)"):
        read_alex_weights(lin_path, backbone_path)
    lin_path, backbone_path, _ = write_weights(tmp_path)
    lin = torch.load(lin_path, weights_only=True)
    lin["lin0.model.1.weight"] = torch.zeros(1, 63, 1, 1)
    torch.save(lin, lin_path)
    with pytest.raises(ValueError, match="lin0.model.1.weight"):
        read_alex_weights(lin_path, backbone_path)


def test_other_nets_are_refused():
    from ebfi_amd.lpips import load_alex_lpips
    with pytest.raises(NotImplementedError, match="vgg"):
        load_alex_lpips("unused", "unused", net="vgg")


# ------------------------------------------------------------------ the C entry points' argument errors (no GPU touched)
@pytest.fixture(scope="module")
def lib():
    if not os.path.exists(N.LIB_PATH):
        N.build()
    return N.lib()


def test_sizes_are_host_arithmetic(lib):
    kpad = [368, 1600, 1728, 3456, 2304]
    cout = [64, 192, 384, 256, 256]
    assert lib.ebfi_lpips_params_bytes() == 4 * sum(k * c + 2 * c for k, c in zip(kpad, cout))
    assert lib.ebfi_lpips_workspace(16, 3, 720, 1280) >= 4 * 2 * 16 * (64 * 179 * 319 + 192 * 89 * 159 + (384 + 256 + 256) * 44 * 79)
    assert lib.ebfi_lpips_workspace(1, 3, 31, 31) > 0
    for bad in ((1, 2, 64, 64), (1, 3, 30, 64), (1, 1, 64, 30), (-1, 3, 64, 64)):
        assert lib.ebfi_lpips_workspace(*bad) == 0, bad


def test_alex_argument_errors(lib):
    p = ctypes.c_void_p(256)          # never dereferenced: every case below fails before a launch
    s = N.i64x4((3 * 64 * 64, 64 * 64, 64, 1))
    ws = lib.ebfi_lpips_workspace(2, 3, 64, 64)

    def call(pred=p, ps=s, target=p, ts=s, n=2, c=3, h=64, w=64, params=p, work=p, nbytes=ws, out=p):
        return lib.ebfi_lpips_alex(pred, ps, target, ts, n, c, h, w, 1, params, work, nbytes, out, None, None)

    assert call(pred=None) == -1 and b"null" in lib.ebfi_last_error()
    assert call(params=None) == -1
    assert call(out=None) == -1
    assert call(c=2) == -1 and b"C in {1, 3}" in lib.ebfi_last_error()
    assert call(h=30) == -1 and call(w=30) == -1
    assert call(ts=N.i64x4((3 * 64 * 128, 64 * 128, 128, 2))) == -1 and b"column stride" in lib.ebfi_last_error()
    assert call(nbytes=ws - 1) == -4 and b"workspace" in lib.ebfi_last_error()


def test_pack_argument_errors(lib):
    ptrs = (ctypes.c_void_p * 5)(*([256] * 5))
    holes = (ctypes.c_void_p * 5)(256, 256, None, 256, 256)
    nbytes = lib.ebfi_lpips_params_bytes()
    assert lib.ebfi_lpips_pack_params(ptrs, ptrs, ptrs, None, nbytes, None) == -1
    assert lib.ebfi_lpips_pack_params(ptrs, holes, ptrs, ctypes.c_void_p(256), nbytes, None) == -1
    assert b"layer 3" in lib.ebfi_last_error()
    assert lib.ebfi_lpips_pack_params(ptrs, ptrs, ptrs, ctypes.c_void_p(256), nbytes - 4, None) == -4


# ------------------------------------------------------------------ the shim and the command line
def test_shim_without_paths_still_raises():
    from loss import perceptual_loss
    with pytest.raises(NotImplementedError, match="LPIPS"):
        perceptual_loss(net="alex", lin_path="alex.pth")
    with pytest.raises(NotImplementedError, match="LPIPS"):
        perceptual_loss(net="alex", backbone_path="alexnet-owt-7be5be79.pth")


@pytest.fixture(scope="module")
def cli():
    spec = importlib.util.spec_from_file_location("ebfi_infer_ours_lpips_host", os.path.join(PKG, "infer_ours.py"))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod


@pytest.mark.parametrize("flag", ["--lpips_lin", "--lpips_backbone"])
def test_cli_refuses_a_single_lpips_flag(cli, flag):
    with pytest.raises(SystemExit, match="both weight files"):
        cli.main([flag, "some.pth", "--data_list", "list.txt", "--output_path", "out"])


def test_cli_flags_parse(cli):
    a = cli.get_flags(["--lpips_lin", "a.pth", "--lpips_backbone", "b.pth"])
    assert (a.lpips_lin, a.lpips_backbone) == ("a.pth", "b.pth")
    a = cli.get_flags([])
    assert a.lpips_lin is None and a.lpips_backbone is None
