"""The yardstick of the LPIPS VGG-16 tests: a torch-CPU restatement of the definition (include/ebfi_hip.h, ebfi_lpips_vgg;
PNetLin(pnet_type='vgg', version='0.1', spatial=False) in eval mode) with F.conv2d / F.max_pool2d(x, 2, 2), in float64 by default,
and a seeded trunk writer.  Shared by test_lpips_vgg_host and test_gpu_lpips_vgg."""
import os

import numpy as np
import torch
import torch.nn.functional as F

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
LIN_FIXTURE = os.path.join(ROOT, "tests", "golden", "lpips_vgg_v01_lin.npz")

TRUNK_KEYS = tuple("features.%d" % i for i in (0, 2, 5, 7, 10, 12, 14, 17, 19, 21, 24, 26, 28))
BLOCKS = ((64, 64), (128, 128), (256, 256, 256), (512, 512, 512), (512, 512, 512))     # a 2x2 / stride 2 pool between blocks
HEAD_CHANNELS = tuple(b[-1] for b in BLOCKS)
SHIFT = (-0.030, -0.088, -0.188)
SCALE = (0.458, 0.448, 0.450)


def conv_shapes():
    shapes, cin = [], 3
    for block in BLOCKS:
        for cout in block:
            shapes.append((cout, cin, 3, 3))
            cin = cout
    return tuple(shapes)


CONV_SHAPES = conv_shapes()


# ------------------------------------------------------------------ weights
def random_trunk(seed=0):
    """A seeded VGG-16 trunk: He-scaled weights and biases in [0.01, 0.06], so that every ReLU layer stays about half active."""
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
    """(lin_path, backbone_path, (ws, bs, heads)): the fixture's heads in the reference's vgg.pth layout and a random trunk in
    torchvision's VGG-16 layout (with a classifier entry, which the loader ignores)."""
    ws, bs = random_trunk(seed)
    heads = fixture_heads()
    trunk = {}
    for key, w, b in zip(TRUNK_KEYS, ws, bs):
        trunk[key + ".weight"], trunk[key + ".bias"] = w, b
    trunk["classifier.0.weight"] = torch.zeros(4, 25088)
    lin = {"lin%d.model.1.weight" % l: h.reshape(1, -1, 1, 1) for l, h in enumerate(heads)}
    lin_path, backbone_path = str(tmp_path / "vgg.pth"), str(tmp_path / "vgg16.pth")
    torch.save(lin, lin_path)
    torch.save(trunk, backbone_path)
    return lin_path, backbone_path, (ws, bs, heads)


# ------------------------------------------------------------------ the restatement
def ref_features(x, ws, bs, normalize=True, dtype=torch.float64):
    """The five tap maps (ReLU outputs of conv1_2, conv2_2, conv3_3, conv4_3, conv5_3) for [N, 3, H, W] images."""
    x = x.to(dtype)
    if normalize:
        x = 2 * x - 1
    shift = torch.tensor(SHIFT, dtype=dtype).view(1, 3, 1, 1)
    scale = torch.tensor(SCALE, dtype=dtype).view(1, 3, 1, 1)
    x = (x - shift) / scale
    taps, i = [], 0
    for k, block in enumerate(BLOCKS):
        if k:
            if x.shape[2] < 2 or x.shape[3] < 2:
                raise RuntimeError("the VGG-16 trunk needs H, W >= 16: the pool before block %d has no window" % (k + 1))
            x = F.max_pool2d(x, 2, 2)
        for _ in block:
            x = F.relu(F.conv2d(x, ws[i].to(dtype), bs[i].to(dtype), stride=1, padding=1))
            i += 1
        taps.append(x)
    return taps


def ref_distances(feats0, feats1, heads):
    """[N, L] layer terms: mean over the pixels of sum_c w_c (u0_c - u1_c)^2, u = f / (||f||_c + 1e-10)."""
    out = []
    for f0, f1, h in zip(feats0, feats1, heads):
        u0 = f0 / (torch.sqrt((f0 ** 2).sum(1, keepdim=True)) + 1e-10)
        u1 = f1 / (torch.sqrt((f1 ** 2).sum(1, keepdim=True)) + 1e-10)
        d = (h.to(f0.dtype).view(1, -1, 1, 1) * (u0 - u1) ** 2).sum(1)
        out.append(d.mean((1, 2)))
    return torch.stack(out, 1)


def ref_lpips(pred, target, ws, bs, heads, normalize=True, dtype=torch.float64):
    """(lpips [N], layers [N, 5]) of an [N, C, H, W] pair, C in {1, 3} (one channel read as three), evaluated in `dtype`."""
    pred, target = torch.as_tensor(pred).cpu(), torch.as_tensor(target).cpu()
    if pred.shape[1] == 1:
        pred, target = pred.expand(-1, 3, -1, -1), target.expand(-1, 3, -1, -1)
    layers = ref_distances(ref_features(pred, ws, bs, normalize, dtype), ref_features(target, ws, bs, normalize, dtype), heads)
    return layers.sum(1), layers
