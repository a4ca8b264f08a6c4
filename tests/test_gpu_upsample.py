"""The frame-upsampling step on the device (ebfi_amd.upsample, csrc/upsample.hip, the 5x5 instantiation of csrc/conv2d.hip)
against the float64 restatement of its law (tests/upsample_ref.py, itself held to the reference's own outputs by
test_upsample_host.py).

Bars.  Kernels: max |err| <= 1e-4 * max |reference| (the project's kernel bar); the flow maximum and the byte law: exact (a
selection, and a law on bytes); a whole U-Net, and the float frames of a pair: 1e-3 (the project's whole-model bar); gray bytes
of a pair: within 1 level, which 1e-3 of a frame in [0, 1] implies (0.255 of a level per channel, and the gray weights sum to 1).

Shapes are the smallest at which each path can go wrong: ragged maps without a 16-byte form (5x4x6, 2x3, 5x7, 33x70), maps with
one (8x16, 32x32, 64x96), the 1x1 bottom of a 32-pixel side, maps smaller than a convolution tile, two
output-channel blocks, more than one workgroup."""
import os
import shutil

import numpy as np
import pytest
import torch
import torch.nn.functional as F

import upsample_ref as R
from test_upsample_host import fixture, load_script, restated_pair

pytestmark = pytest.mark.gpu
KERNEL_BAR, MODEL_BAR = 1e-4, 1e-3
_cache = {}


def lib_st():
    from ebfi_amd import _native as N
    return N, N.lib(), N.stream_ptr(torch.device("cuda", 0))


def relerr(got, want):
    want = want.double()
    return ((got.detach().cpu().double() - want).abs().max() / want.abs().max()).item()


def seeded(shape, seed, lo=-1.0, hi=1.0):
    g = torch.Generator().manual_seed(seed)
    return (torch.rand(shape, generator=g, dtype=torch.float32) * (hi - lo) + lo).contiguous()


def images(H, W, seed):
    """Two normalised frames [3, H, W] in [-0.43, 0.6]: a smooth seeded texture plus a fifth of white noise."""
    g = torch.Generator().manual_seed(seed)
    coarse = torch.rand((2, 3, H // 8 + 2, W // 8 + 2), generator=g, dtype=torch.float32)
    smooth = F.interpolate(coarse, scale_factor=8, mode="bilinear", align_corners=False)[:, :, 4:4 + H, 4:4 + W]
    v = 0.8 * smooth + 0.2 * torch.rand((2, 3, H, W), generator=g, dtype=torch.float32)
    v = (v * 1.03 - 0.43).contiguous()
    return v[0].contiguous(), v[1].contiguous()


def device_upsampler():
    """One Upsampler with the seeded networks for the whole session (80 MB of weights each way)."""
    if "up" not in _cache:
        from ebfi_amd.upsample import Upsampler
        _cache["up"] = Upsampler.from_state_dicts("cuda:0", R.flow_state_dict(), R.interp_state_dict())
    return _cache["up"]


# ------------------------------------------------------------------------------------------------------------ pool, up-sampling
@pytest.mark.parametrize("shape", [(5, 4, 6), (32, 2, 2), (3, 8, 16)])
def test_avgpool2(shape):
    N, lib, st = lib_st()
    x = seeded(shape, 1)
    out = torch.empty((shape[0], shape[1] // 2, shape[2] // 2), device="cuda")
    xd = x.cuda()
    N.check(lib.ebfi_avgpool2_forward(N.ptr(xd), N.ptr(out), *shape, st), "avgpool2")
    assert relerr(out, F.avg_pool2d(x.double()[None], 2)[0]) <= KERNEL_BAR


@pytest.mark.parametrize("shape", [(7, 1, 1), (3, 2, 3), (2, 5, 7), (3, 4, 8)])
def test_bilinear_up2(shape):
    N, lib, st = lib_st()
    x = seeded(shape, 2)
    out = torch.empty((shape[0], 2 * shape[1], 2 * shape[2]), device="cuda")
    xd = x.cuda()
    N.check(lib.ebfi_bilinear_up2_forward(N.ptr(xd), N.ptr(out), *shape, st), "bilinear_up2")
    want = F.interpolate(x.double()[None], scale_factor=2, mode="bilinear", align_corners=True)[0]
    assert relerr(out, want) <= KERNEL_BAR


def test_pool_and_up_refuse_bad_sizes():
    N, lib, st = lib_st()
    x = torch.zeros(64, device="cuda")
    assert lib.ebfi_avgpool2_forward(N.ptr(x), N.ptr(x), 1, 3, 4, st) == -1
    assert lib.ebfi_avgpool2_forward(N.ptr(None), N.ptr(x), 1, 2, 4, st) == -1
    assert lib.ebfi_bilinear_up2_forward(N.ptr(x), N.ptr(x), 0, 2, 4, st) == -1


# ------------------------------------------------------------------------------------------------------------ flow maximum
@pytest.mark.parametrize("where", ["first", "last", "tail"])
@pytest.mark.parametrize("H,W", [(32, 32), (33, 70)])
def test_flow_max_magnitude_is_exact(H, W, where):
    N, lib, st = lib_st()
    flow = seeded((4, H, W), 3).numpy()
    u, v = np.float32(3.3), np.float32(-4.1)
    pair, at = {"first": (0, 0), "last": (2, H * W - 1), "tail": (0, H * W - 2)}[where]
    flat = flow.reshape(4, -1)
    flat[pair, at], flat[pair + 1, at] = u, v
    want = np.sqrt(flat[0::2].astype(np.float32) ** 2 + flat[1::2].astype(np.float32) ** 2, dtype=np.float32).max()
    assert want == np.sqrt(u * u + v * v, dtype=np.float32) and want.dtype == np.float32
    out = torch.full((1,), -7.0, device="cuda")
    fd = torch.from_numpy(flow).cuda()
    N.check(lib.ebfi_flow_max_magnitude(N.ptr(fd), H, W, N.ptr(out), st), "flow_max")
    assert out.item() == float(want)
    assert R.flow_max(torch.from_numpy(flow)[None]) == float(want)          # the restatement in float32 selects the same number


# ------------------------------------------------------------------------------------------------------------ the warps
def warp_flow_cases(H, W, t):
    """name -> flowOut [4, H, W].  Most cases steer F_t_1 = (1-t)^2 F_0_1 (with F_1_0 = 0); F_t_0 = -t(1-t) F_0_1 then moves the
    other way by a different amount, which is as good a case."""
    gy, gx = torch.meshgrid(torch.arange(H, dtype=torch.float32), torch.arange(W, dtype=torch.float32), indexing="ij")
    c = (1 - t) * (1 - t)
    z = torch.zeros(H, W)
    cases = {"zero": torch.zeros(4, H, W)}
    cases["integer"] = torch.stack([z + 2, z - 3, z - 1, z + 2])
    cases["fractional"] = seeded((4, H, W), 5, -3.0, 3.0)
    # landing positions (in gx + u) by bands of rows, and (gy + v) by bands of columns: outside by less and by more than a pixel
    # on every side, and inside
    lx = torch.tensor([-0.5, -1.7, W - 0.4, W + 1.3, 3.25, W - 1.5, -0.999, W + 0.02])[(gy.long() * 8) // H]
    ly = torch.tensor([2.5, -0.3, H - 0.6, -2.2, H + 1.1, H - 1.0, 0.0, H - 0.01])[(gx.long() * 8) // W]
    cases["outside"] = torch.stack([(lx - gx) / c, (ly - gy) / c, z, z])
    # gx + u = W and gy + v = H: the sampling position is exactly W - 1 / H - 1 where W, H are powers of two
    cases["edge"] = torch.stack([(W - gx) / c, (H - gy) / c, z, z])
    return {k: v.contiguous() for k, v in cases.items()}


@pytest.mark.parametrize("H,W", [(32, 32), (64, 96)])
@pytest.mark.parametrize("case", ["zero", "integer", "fractional", "outside", "edge"])
def test_assemble_warps(H, W, case):
    N, lib, st = lib_st()
    I0, I1 = images(H, W, 6)
    out = torch.empty((20, H, W), device="cuda")
    d0, d1 = I0.cuda(), I1.cuda()
    for t in (1 / 3, 1 / 2, 7 / 8):
        flow = warp_flow_cases(H, W, t)[case]
        fd = flow.cuda()
        N.check(lib.ebfi_slomo_assemble(N.ptr(d0), N.ptr(d1), N.ptr(fd), t, N.ptr(out), H, W, st), "assemble")
        want = R.assemble(I0.double()[None], I1.double()[None], flow.double()[None], t)[0]
        if case == "zero":          # the shrink: zero flow is not the identity
            assert (want[14:17] - I1.double()).abs().max() > 1e-3
        for lo, hi in ((0, 6), (6, 10), (10, 14), (14, 17), (17, 20)):
            if want[lo:hi].abs().max() == 0:
                assert out[lo:hi].abs().max().item() == 0
            else:
                err = relerr(out[lo:hi], want[lo:hi])
                assert err <= KERNEL_BAR, (case, t, lo, err)


def test_assemble_and_blend_refuse_bad_arguments():
    N, lib, st = lib_st()
    x = torch.zeros(20 * 32 * 32 + 4, device="cuda")
    g = torch.zeros(32 * 32, dtype=torch.uint8, device="cuda")
    ok = (N.ptr(x), N.ptr(x), N.ptr(x))
    assert lib.ebfi_slomo_assemble(*ok, 0.5, N.ptr(x), 32, 30, st) == -1            # W % 4
    assert lib.ebfi_slomo_assemble(*ok, 1.0, N.ptr(x), 32, 32, st) == -1            # t
    assert lib.ebfi_slomo_assemble(N.ptr(x[1:]), N.ptr(x), N.ptr(x), 0.5, N.ptr(x), 32, 32, st) == -1     # alignment
    assert lib.ebfi_slomo_blend(N.ptr(x), N.ptr(x), 0.0, N.ptr(None), N.ptr(g), 32, 32, st) == -1
    assert lib.ebfi_slomo_blend(N.ptr(x), N.ptr(x), 0.5, N.ptr(None), N.ptr(None), 32, 32, st) == -1


@pytest.mark.parametrize("H,W", [(32, 32), (64, 96)])
def test_blend(H, W):
    """The blend kernel against the restatement on seeded network outputs: refined warps, sigmoid, blend, + mean; and its bytes
    against the byte law applied to ITS OWN float frame (exact), so the two outputs of one launch agree."""
    N, lib, st = lib_st()
    t = 1 / 3
    I0, I1 = images(H, W, 8)
    flow, intrp = seeded((4, H, W), 10, -3.0, 3.0), seeded((5, H, W), 11, -2.0, 2.0)
    x20 = R.assemble(I0.double()[None], I1.double()[None], flow.double()[None], t)
    want = R.blend(intrp.double()[None], x20, t)[0]
    rgb = torch.empty((3, H, W), device="cuda")
    gray = torch.empty((H, W), dtype=torch.uint8, device="cuda")
    di, dx = intrp.cuda(), x20[0].float().contiguous().cuda()
    N.check(lib.ebfi_slomo_blend(N.ptr(di), N.ptr(dx), t, N.ptr(rgb), N.ptr(gray), H, W, st),
            "blend")
    assert relerr(rgb, want) <= KERNEL_BAR
    assert np.array_equal(gray.cpu().numpy(), R.gray15(R.frames_to_levels(rgb.cpu().numpy())))
    gray2 = torch.empty_like(gray)
    N.check(lib.ebfi_slomo_blend(N.ptr(di), N.ptr(dx), t, N.ptr(None), N.ptr(gray2), H, W, st),
            "blend without the float frame")
    assert torch.equal(gray, gray2)


# ------------------------------------------------------------------------------------------------------------ the byte law
def byte_law_values():
    """float32 [3, L]: per channel k / 255 - mean for every k (the I0 round trip), one float32 step either side, and values
    below 0 and above 1 after the mean is added."""
    from ebfi_amd.upsample import normalise_table
    table = normalise_table()
    special = np.array([-1.0, -0.5, -0.4290001, -0.397, -0.0, 0.0, 0.569, 0.5690001, 0.571, 0.603, 0.61, 1.0, 2.0, 1e30, -1e30,
                        1e20, -1e20, 1e-40], dtype=np.float32)
    rows = [np.concatenate([table[c], np.nextafter(table[c], np.float32(np.inf)), np.nextafter(table[c], np.float32(-np.inf)),
                            special]) for c in range(3)]
    return np.stack(rows).astype(np.float32)


@pytest.mark.parametrize("drop", [0, 1, 2])
def test_frame_u8_is_bit_exact(drop):
    """drop: 786 values (no multiple of 4: the scalar form), 785, 784 (the 16-byte form)"""
    N, lib, st = lib_st()
    vals = byte_law_values()
    vals = vals[:, :vals.shape[1] - drop]
    L = vals.shape[1]
    assert L == 786 - drop
    # every channel's list against the two other channels' lists rotated, so the gray sum sees varied triples
    frame = np.stack([vals[0], np.roll(vals[1], 7), np.roll(vals[2], 131)]).reshape(3, 1, L)
    frame = np.concatenate([frame, frame[:, :, ::-1], np.stack([vals[1], vals[2], vals[0]]).reshape(3, 1, L)], axis=1)     # [3, 3, L]
    want = R.frame_u8(frame)
    out = torch.full((3, L), 77, dtype=torch.uint8, device="cuda")
    fd = torch.from_numpy(frame.copy()).cuda()
    N.check(lib.ebfi_slomo_frame_u8(N.ptr(fd), N.ptr(out), 3, L, st), "frame_u8")
    got = out.cpu().numpy()
    assert np.array_equal(got, want), (int((got != want).sum()), np.argwhere(got != want)[:5])
    # the I0 round trip on the table itself: byte -> normalised -> byte is what the law says, for every byte and channel
    levels = R.levels_f32(vals[:, :256].reshape(3, 1, 256))
    assert levels.shape == (3, 1, 256) and (np.abs(levels.astype(int) - np.arange(256)) <= 1).all()


# ------------------------------------------------------------------------------------------------------------ 5x5 convolution
@pytest.mark.parametrize("act", [0, 1])
@pytest.mark.parametrize("shape", [(1, 32, 9, 41, 64), (1, 64, 32, 48, 64), (2, 5, 4, 5, 8)])
def test_conv5x5_forward(shape, act):
    N, lib, st = lib_st()
    B, Cin, H, W, Cout = shape
    x = seeded((B, Cin, H, W), 12)
    w = seeded((Cout, Cin, 5, 5), 13) * (1.0 / (Cin * 25) ** 0.5)
    b = seeded((Cout,), 14)
    out = torch.full((B, Cout, H, W), float("nan"), device="cuda")
    xd, wd, bd = x.cuda(), w.contiguous().cuda(), b.cuda()
    N.check(lib.ebfi_conv2d_forward(N.ptr(xd), N.ptr(wd), N.ptr(bd), N.ptr(out), B, Cin, H, W, Cout, 5, 1, 2,
                                    act, 0.1, N.EBFI_F32, st), "conv2d_forward 5x5")
    want = F.conv2d(x.double(), w.double(), b.double(), padding=2)
    if act:
        want = F.leaky_relu(want, 0.1)
    assert relerr(out, want) <= KERNEL_BAR


def test_conv5x5_elsewhere_is_still_refused():
    N, lib, st = lib_st()
    x = torch.zeros(1, 8, 8, 8, device="cuda")
    w = torch.zeros(8, 8, 5, 5, device="cuda")
    geo = (1, 8, 8, 8, 8, 5)
    assert lib.ebfi_conv2d_forward(N.ptr(x), N.ptr(w), N.ptr(None), N.ptr(x), *geo, 2, 2, 0, 0.0, N.EBFI_F32, st) == N.EBFI_ERR_UNSUPPORTED
    assert lib.ebfi_conv2d_backward_data(N.ptr(x), N.ptr(None), N.ptr(w), N.ptr(x), *geo, 1, 2, 0, 0.0, N.EBFI_F32, st) == N.EBFI_ERR_UNSUPPORTED
    assert lib.ebfi_conv2d_backward_weight_workspace(*geo, 1, 2, N.EBFI_F32) == 0


# ------------------------------------------------------------------------------------------------------------ whole networks
@pytest.mark.parametrize("net,cin,H,W", [("flow", 6, 64, 96), ("interp", 20, 32, 32), ("flow", 6, 32, 32)])
def test_unet_forward(net, cin, H, W):
    up = device_upsampler()
    model, sd = (up.flowComp, R.flow_state_dict()) if net == "flow" else (up.ArbTimeFlowIntrp, R.interp_state_dict())
    x = seeded((cin, H, W), 15, -0.5, 0.6)
    with torch.no_grad():
        want = R.unet_forward(sd, x[None])[0]
    got = model(x.cuda())
    err = relerr(got, want)
    print("unet %s %dx%dx%d: max abs err / max abs ref = %.3e" % (net, cin, H, W, err))
    assert err <= MODEL_BAR


def test_unet_refuses_what_it_cannot_run():
    up = device_upsampler()
    with pytest.raises(ValueError):
        up.flowComp(torch.zeros(6, 48, 64, device="cuda"))
    with pytest.raises(NotImplementedError):
        up.flowComp(torch.zeros(6, 32, 32))
    from ebfi_amd.upsample import SloMoNet
    with pytest.raises(KeyError):
        SloMoNet(6, 4, "cuda:0").load_state_dict({})


# ------------------------------------------------------------------------------------------------------------ one pair
def test_fixture_pair():
    fx, res = fixture(), restated_pair()
    up = device_upsampler()
    I0, I1 = (up.normalise(f) for f in fx["pair_u8"])
    assert np.array_equal(I0.cpu().numpy(), R.normalise(fx["pair_u8"][0]))
    n, stamps, gray, frames = up.upsample_pair(I0, I1, float(fx["times"][0]), float(fx["times"][1]), want_float=True)
    assert n == int(fx["N"]) == res["N"]
    assert stamps == list(fx["timestamps"]) == res["timestamps"]
    err = relerr(frames, res["frames"])
    print("pair: float frames max abs err / max abs ref = %.3e" % err)
    assert err <= MODEL_BAR
    want = np.stack([R.frame_u8(R.normalise(fx["pair_u8"][0]))] +
                    [R.gray15(R.frames_to_levels(f.float().numpy())) for f in res["frames"][1:]])
    got = gray.cpu().numpy()
    diff = np.abs(got.astype(int) - want.astype(int))
    print("pair: gray bytes that differ from the restatement's: %d of %d (%.4f %%), largest difference %d"
          % ((diff > 0).sum(), diff.size, 100.0 * (diff > 0).mean(), diff.max()))
    assert np.array_equal(got[0], want[0])           # I0: the byte law on the same float32 values
    assert diff.max() <= 1
    _, stamps2, gray2, none = up.upsample_pair(I0, I1, float(fx["times"][0]), float(fx["times"][1]))
    assert none is None and stamps2 == stamps and torch.equal(gray, gray2)


# ------------------------------------------------------------------------------------------------------------ the script
def e2e_frames():
    """three 70 x 100 frames: one seeded texture, rolled a little further each frame (the crop to 64 x 96 is exercised)"""
    base, _ = R.pair_images(72, 104, seed=11)
    return [np.roll(base, (k, 2 * k), (0, 1))[:70, :100].copy() for k in range(3)]


def test_script_end_to_end(tmp_path):
    from PIL import Image
    frames = e2e_frames()
    seq = tmp_path / "in" / "seq0"
    (seq / "imgs").mkdir(parents=True)
    (seq / "fps.txt").write_text("240\n")
    for k, f in enumerate(frames):
        Image.fromarray(f).save(str(seq / "imgs" / ("%04d.png" % k)))
    ckpt = tmp_path / "SuperSloMo.ckpt"
    torch.save({"state_dictFC": R.flow_state_dict(), "state_dictAT": R.interp_state_dict()}, str(ckpt))
    out = tmp_path / "out"
    assert load_script().main(["--input_dir", str(tmp_path / "in"), "--output_dir", str(out), "--checkpoint", str(ckpt),
                               "--imgs_dirname", "mono"]) == 0
    with torch.no_grad():
        want_gray, want_stamps = R.upsample_sequence(R.flow_state_dict(), R.interp_state_dict(), frames, 240.0)
    assert len(want_gray) > 4
    names = sorted(os.listdir(str(out / "seq0" / "mono")))
    assert names == ["%08d.png" % k for k in range(len(want_gray))]
    assert (out / "seq0" / "timestamps.txt").read_text() == "".join(str(t) + "\n" for t in want_stamps)
    for name, want in zip(names, want_gray):
        with Image.open(str(out / "seq0" / "mono" / name)) as im:
            assert im.mode == "L" and im.size == (96, 64)
            got = np.asarray(im).astype(int)
        assert np.abs(got - want.astype(int)).max() <= 1, name
    # the next stage reads it: rgb/ beside mono/ and timestamps.txt
    shutil.copytree(str(seq / "imgs"), str(out / "seq0" / "rgb"))
    import importlib.util
    path = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "ebfi-be_amd", "generate_dataset", "syn_gopro.py")
    spec = importlib.util.spec_from_file_location("syn_gopro_script", path)
    syn = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(syn)
    assert syn.main(["--root_data_path", str(out), "--path_to_h5", str(tmp_path / "h5")]) == 0
    clip = np.load(str(tmp_path / "h5" / "seq0.npz"))
    assert clip["images"].shape == (3, 70, 100, 3) and len(clip["ts"]) == len(clip["xs"]) > 0
