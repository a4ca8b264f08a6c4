"""Restatement of the frame-upsampling law (the Vid2E adaptive upsampler around two Super-SloMo U-Nets) in plain torch on the
CPU, in the dtype the caller asks for (float64 by default): what ebfi_amd.upsample and csrc/upsample.hip are held to.  It is
itself held to the reference's own code by tests/golden/upsample_small.npz (tests/golden/make_golden_upsample.py runs the
reference's UNet, backWarp and _upsample_adaptive; tests/test_upsample_host.py compares).

The law, layer by layer, is in ebfi_amd/upsample.py's and include/ebfi_hip.h's comments; nothing here is device code.

The weights of the tests are not stored (about 40 M parameters): `seeded_state_dict` is the recipe, and the fixture carries a
few checksums of what it gave when the fixture was made.
"""
import math

import numpy as np
import torch
import torch.nn.functional as F

MEAN = (0.429, 0.431, 0.397)
GRAY15 = (3735, 19235, 9798)          # channel 0, 1, 2 under cvtColor(BGR2GRAY)'s 15-bit law (unverified against cv2)
SLOPE = 0.1

FC_SEED, AT_SEED = 20250301, 20250302
# conv3 of the flow network is scaled so that the seeded flows of the fixture's pair reach a few pixels: the generator asserts
# 3 <= N <= 8 and a fractional part of the maximum in [0.2, 0.8] on the reference's float64 numbers.  LeakyReLU is positively
# homogeneous, so the scale multiplies the flows exactly.
FC_LAST_SCALE = 3.7
CHECKSUM_KEYS = ("conv1.weight", "down1.conv1.weight", "up1.conv2.weight", "conv3.weight", "conv3.bias")


def unet_layers(in_channels, out_channels):
    layers = [("conv1", in_channels, 32, 7), ("conv2", 32, 32, 7)]
    for i, (ci, co, k) in enumerate([(32, 64, 5), (64, 128, 3), (128, 256, 3), (256, 512, 3), (512, 512, 3)], 1):
        layers += [("down%d.conv1" % i, ci, co, k), ("down%d.conv2" % i, co, co, k)]
    for i, (ci, co) in enumerate([(512, 512), (512, 256), (256, 128), (128, 64), (64, 32)], 1):
        layers += [("up%d.conv1" % i, ci, co, 3), ("up%d.conv2" % i, 2 * co, co, 3)]
    return layers + [("conv3", 32, out_channels, 3)]


_sd_cache = {}


def seeded_state_dict(in_channels, out_channels, seed, last_scale=1.0):
    """float32 state dict with the reference's key names: weight ~ N(0, 2 / fan_in), bias ~ N(0, 0.05^2), one torch.Generator
    walked in layer order; conv3 times `last_scale`.  Cached: callers must not modify the tensors."""
    key = (in_channels, out_channels, seed, last_scale)
    if key not in _sd_cache:
        g = torch.Generator().manual_seed(seed)
        sd = {}
        for name, ci, co, k in unet_layers(in_channels, out_channels):
            sd[name + ".weight"] = torch.randn((co, ci, k, k), generator=g, dtype=torch.float32) * math.sqrt(2.0 / (ci * k * k))
            sd[name + ".bias"] = torch.randn((co,), generator=g, dtype=torch.float32) * 0.05
        sd["conv3.weight"] = sd["conv3.weight"] * last_scale
        sd["conv3.bias"] = sd["conv3.bias"] * last_scale
        _sd_cache[key] = sd
    return _sd_cache[key]


def flow_state_dict():
    return seeded_state_dict(6, 4, FC_SEED, FC_LAST_SCALE)


def interp_state_dict():
    return seeded_state_dict(20, 5, AT_SEED)


def checksums(sd):
    """float64 [len(CHECKSUM_KEYS), 2]: sum and sum of absolute values of a few tensors."""
    return np.array([[sd[k].double().sum().item(), sd[k].double().abs().sum().item()] for k in CHECKSUM_KEYS])


# ------------------------------------------------------------------------------------------------------------ the network
def conv_act(x, sd, name, dtype):
    w, b = sd[name + ".weight"].to(dtype), sd[name + ".bias"].to(dtype)
    return F.leaky_relu(F.conv2d(x, w, b, stride=1, padding=w.shape[-1] // 2), SLOPE)


def unet_forward(sd, x, dtype=torch.float64):
    """x [B, Cin, H, W] -> [B, Cout, H, W]"""
    x = x.to(dtype)
    x = conv_act(x, sd, "conv1", dtype)
    skips = [conv_act(x, sd, "conv2", dtype)]
    x = skips[0]
    for i in range(1, 6):
        x = F.avg_pool2d(x, 2)
        x = conv_act(conv_act(x, sd, "down%d.conv1" % i, dtype), sd, "down%d.conv2" % i, dtype)
        if i < 5:
            skips.append(x)
    for i in range(1, 6):
        x = F.interpolate(x, scale_factor=2, mode="bilinear", align_corners=True)
        x = conv_act(x, sd, "up%d.conv1" % i, dtype)
        x = conv_act(torch.cat((x, skips[5 - i]), 1), sd, "up%d.conv2" % i, dtype)
    return conv_act(x, sd, "conv3", dtype)


def back_warp(img, flow):
    """img [B, C, H, W], flow [B, 2, H, W] (u, v): the reference's coordinate law into grid_sample."""
    B, _, H, W = img.shape
    gy, gx = torch.meshgrid(torch.arange(H, device=img.device), torch.arange(W, device=img.device), indexing="ij")
    x = gx.to(img.dtype)[None] + flow[:, 0]
    y = gy.to(img.dtype)[None] + flow[:, 1]
    grid = torch.stack((2 * (x / W - 0.5), 2 * (y / H - 0.5)), dim=3)
    return F.grid_sample(img, grid, mode="bilinear", padding_mode="zeros", align_corners=True)


def time_flows(flow_out, t):
    temp = -t * (1 - t)
    F01, F10 = flow_out[:, :2], flow_out[:, 2:]
    return temp * F01 + (t * t) * F10, ((1 - t) * (1 - t)) * F01 + temp * F10        # F_t_0, F_t_1


def assemble(I0, I1, flow_out, t):
    """-> the 20-channel input of the interpolation network"""
    Ft0, Ft1 = time_flows(flow_out, t)
    return torch.cat((I0, I1, flow_out[:, :2], flow_out[:, 2:], Ft1, Ft0, back_warp(I1, Ft1), back_warp(I0, Ft0)), dim=1)


def blend(intrp, x20, t):
    """-> Ft_p + mean, [B, 3, H, W]"""
    I0, I1, Ft1, Ft0 = x20[:, 0:3], x20[:, 3:6], x20[:, 10:12], x20[:, 12:14]
    V0 = torch.sigmoid(intrp[:, 4:5])
    V1 = 1 - V0
    g0, g1 = back_warp(I0, intrp[:, :2] + Ft0), back_warp(I1, intrp[:, 2:4] + Ft1)
    p = ((1 - t) * V0 * g0 + t * V1 * g1) / ((1 - t) * V0 + t * V1)
    return p + torch.tensor(MEAN, dtype=p.dtype, device=p.device).view(1, 3, 1, 1)


def flow_max(flow_out):
    """max over both flows of the magnitude, in flow_out's dtype"""
    m01 = flow_out[:, :2].pow(2).sum(1).pow(0.5).max()
    m10 = flow_out[:, 2:].pow(2).sum(1).pow(0.5).max()
    return torch.max(m01, m10).item()


def upsample_pair(sd_fc, sd_at, I0, I1, t0, t1, dtype=torch.float64):
    """I0, I1: normalised [3, H, W].  -> dict: flow_out [4, H, W], flow_max, N, timestamps, frames [max(N, 1), 3, H, W] (+ mean:
    I0, then the intermediates), intrp {k: [5, H, W]}, x20 {k: [20, H, W]}"""
    I0, I1 = I0.to(dtype)[None], I1.to(dtype)[None]
    mean = torch.tensor(MEAN, dtype=dtype).view(1, 3, 1, 1)
    flow_out = unet_forward(sd_fc, torch.cat((I0, I1), 1), dtype)
    fmax = flow_max(flow_out)
    n = int(math.ceil(fmax))
    frames, stamps, intrps, x20s = [I0 + mean], [t0], {}, {}
    for k in range(1, n):
        t = float(k) / n
        x20 = assemble(I0, I1, flow_out, t)
        intrp = unet_forward(sd_at, x20, dtype)
        frames.append(blend(intrp, x20, t))
        stamps.append(t0 + t * (t1 - t0))
        intrps[k], x20s[k] = intrp[0], x20[0]
    return dict(flow_out=flow_out[0], flow_max=fmax, N=n, timestamps=stamps, frames=torch.cat(frames), intrp=intrps, x20=x20s)


# ------------------------------------------------------------------------------------------------------------ bytes
def normalise(rgb_u8):
    """uint8 [H, W, 3] -> float32 [3, H, W]: / 255 then - mean, each rounded in float32"""
    v = rgb_u8.astype(np.float32) / np.float32(255)
    return np.ascontiguousarray(np.stack([v[..., c] - np.float32(MEAN[c]) for c in range(3)]))


def levels_f32(normalised):
    """float32 [..., 3, H, W] normalised frames -> uint8 levels: + mean, * 255, clip, truncate -- every step in float32"""
    v = np.asarray(normalised, dtype=np.float32)
    mean = np.array(MEAN, dtype=np.float32).reshape(3, 1, 1)
    return frames_to_levels(v + mean)


def frames_to_levels(frames_plus_mean):
    return np.clip(255 * np.asarray(frames_plus_mean, dtype=np.float32), 0, 255).astype(np.uint8)


def gray15(levels):
    """uint8 [..., 3, H, W] -> uint8 [..., H, W]"""
    l = levels.astype(np.int64)
    return ((GRAY15[0] * l[..., 0, :, :] + GRAY15[1] * l[..., 1, :, :] + GRAY15[2] * l[..., 2, :, :] + (1 << 14)) >> 15).astype(np.uint8)


def frame_u8(normalised):
    return gray15(levels_f32(normalised))


def crop_box(w_orig, h_orig):
    w, h = w_orig // 32 * 32, h_orig // 32 * 32
    left, upper = (w_orig - w) // 2, (h_orig - h) // 2
    return left, upper, left + w, upper + h


def upsample_sequence(sd_fc, sd_at, rgb_frames, fps, dtype=torch.float64):
    """rgb_frames: uint8 [H, W, 3] each, uncropped.  -> (gray frames uint8 [H', W'] in file order, timestamps)"""
    cropped = []
    for f in rgb_frames:
        l, u, r, d = crop_box(f.shape[1], f.shape[0])
        cropped.append(torch.from_numpy(normalise(f[u:d, l:r])))
    grays, stamps = [], []
    for idx in range(len(cropped) - 1):
        res = upsample_pair(sd_fc, sd_at, cropped[idx], cropped[idx + 1], idx / fps, (idx + 1) / fps, dtype)
        # I0 takes the float32 round trip (normalised float32 + mean); the intermediates come from the restatement's dtype
        g = [frame_u8(cropped[idx].numpy())] + [gray15(frames_to_levels(fr.to(torch.float32).numpy())) for fr in res["frames"][1:]]
        grays += g
        stamps += res["timestamps"]
    return grays, stamps


def pair_images(H=64, W=96, seed=7):
    """Two uint8 [H, W, 3] frames: smooth seeded colour texture, the second shifted and brightened a little."""
    g = np.random.RandomState(seed)
    base = g.rand(3, H // 8 + 3, W // 8 + 3)
    big = F.interpolate(torch.from_numpy(base)[None], scale_factor=8, mode="bicubic", align_corners=False)[0].numpy()
    a = big[:, 8:8 + H, 8:8 + W]
    b = big[:, 10:10 + H, 5:5 + W] * 1.05
    to_u8 = lambda v: np.clip(np.round(255 * v), 0, 255).astype(np.uint8).transpose(1, 2, 0).copy()
    return to_u8(a), to_u8(b)
