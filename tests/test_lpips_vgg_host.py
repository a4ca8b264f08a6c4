"""LPIPS (VGG-16, v0.1) without a GPU: the float64 restatement of lpips_vgg_ref on hand-built cases, the weight loader's
refusals, the C entry points' sizes and argument errors (with pointers that are never dereferenced), the perceptual_loss shim
and the infer_ours.py flag."""
import ctypes
import importlib.util
import os

import numpy as np
import pytest
import torch

from ebfi_amd import _native as N
from lpips_vgg_ref import (CONV_SHAPES, HEAD_CHANNELS, LIN_FIXTURE, fixture_heads, random_trunk, ref_distances, ref_features,
                           ref_lpips, write_weights)

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
PKG = os.path.join(ROOT, "ebfi-be_amd")
ALEX_FIXTURE = os.path.join(ROOT, "tests", "golden", "lpips_alex_v01_lin.npz")


# ------------------------------------------------------------------ the fixture and the restatement on hand-built cases
def test_fixture_holds_the_five_heads_as_plain_arrays():
    z = np.load(LIN_FIXTURE, allow_pickle=False)
    assert sorted(z.files) == ["lin%d" % l for l in range(5)]
    assert [z["lin%d" % l].shape for l in range(5)] == [(c,) for c in HEAD_CHANNELS]
    assert all(z[k].dtype == np.float32 and np.isfinite(z[k]).all() for k in z.files)
    assert sum(z[k].size for k in z.files) == 1472
    assert all((z[k] >= 0).all() and z[k].max() > 0 for k in z.files)       # (the v0.1 heads were trained non-negative)


def test_identical_images_score_zero():
    ws, bs = random_trunk(1)
    x = torch.rand(2, 3, 24, 20, generator=torch.Generator().manual_seed(3))
    total, layers = ref_lpips(x, x.clone(), ws, bs, fixture_heads())
    assert total.shape == (2,) and layers.shape == (2, 5)
    assert torch.all(total == 0) and torch.all(layers == 0)


def test_tap_shapes_at_the_smallest_size():
    ws, bs = random_trunk(0)
    feats = ref_features(torch.rand(1, 3, 16, 16, generator=torch.Generator().manual_seed(1)), ws, bs)
    assert [tuple(f.shape[1:]) for f in feats] == [(64, 16, 16), (128, 8, 8), (256, 4, 4), (512, 2, 2), (512, 1, 1)]
    active = [float((f > 0).double().mean()) for f in feats]
    assert all(0.3 < a < 0.8 for a in active), active             # (the seeded trunk keeps every tap about half active)
    with pytest.raises(RuntimeError):
        ref_features(torch.rand(1, 3, 15, 16), ws, bs)


def test_floor_pooling_drops_an_odd_row_and_column():
    ws, bs = random_trunk(0)
    g = torch.Generator().manual_seed(2)
    x = torch.rand(1, 3, 17, 19, generator=g)
    feats = ref_features(x, ws, bs)
    assert [tuple(f.shape[2:]) for f in feats] == [(17, 19), (8, 9), (4, 4), (2, 2), (1, 1)]


def test_one_channel_is_read_as_three():
    ws, bs = random_trunk(2)
    g = torch.Generator().manual_seed(4)
    a, b = torch.rand(1, 1, 17, 18, generator=g), torch.rand(1, 1, 17, 18, generator=g)
    one, _ = ref_lpips(a, b, ws, bs, fixture_heads())
    three, _ = ref_lpips(a.repeat(1, 3, 1, 1), b.repeat(1, 3, 1, 1), ws, bs, fixture_heads())
    assert float(one[0]) > 0 and float(one[0]) == float(three[0])


def test_single_pixel_difference_of_one_layer():
    f0 = torch.ones(1, 2, 2, 2, dtype=torch.float64)
    f1 = f0.clone()
    f0[0, :, 0, 0] = torch.tensor([3.0, 4.0])
    f1[0, :, 0, 0] = torch.tensor([4.0, 3.0])
    w = torch.tensor([0.5, 2.0])
    d = ref_distances([f0], [f1], [w])
    want = (0.5 + 2.0) * (1.0 / (5.0 + 1e-10)) ** 2 / 4
    assert d.shape == (1, 1) and abs(float(d[0, 0]) - want) < 1e-15


# ------------------------------------------------------------------ the weight loader
def test_loader_reads_both_files_and_ignores_the_classifier(tmp_path):
    from ebfi_amd.lpips import VGG_CONV_SHAPES, read_vgg_weights
    assert VGG_CONV_SHAPES == CONV_SHAPES
    lin_path, backbone_path, (ws, bs, heads) = write_weights(tmp_path)
    assert "classifier.0.weight" in torch.load(backbone_path, weights_only=True)
    rw, rb, rh = read_vgg_weights(lin_path, backbone_path)
    assert (len(rw), len(rb), len(rh)) == (13, 13, 5)
    for got, want in zip(rw + rb + rh, ws + bs + heads):
        assert got.dtype == torch.float32 and torch.equal(got, want.reshape(got.shape))
    assert [tuple(h.shape) for h in rh] == [(64,), (128,), (256,), (512,), (512,)]


def test_loader_names_a_missing_key(tmp_path):
    from ebfi_amd.lpips import read_vgg_weights
    lin_path, backbone_path, _ = write_weights(tmp_path)
    sd = torch.load(backbone_path, weights_only=True)
    sd["features.27.weight"] = sd.pop("features.26.weight")
    torch.save(sd, backbone_path)
    with pytest.raises(KeyError, match=r"features\.26\.weight"):
        read_vgg_weights(lin_path, backbone_path)
    lin_path, backbone_path, _ = write_weights(tmp_path)
    lin = torch.load(lin_path, weights_only=True)
    del lin["lin4.model.1.weight"]
    torch.save(lin, lin_path)
    with pytest.raises(KeyError, match=r"lin4\.model\.1\.weight"):
        read_vgg_weights(lin_path, backbone_path)


def test_loader_names_a_wrong_shape(tmp_path):
    from ebfi_amd.lpips import read_vgg_weights
    lin_path, backbone_path, _ = write_weights(tmp_path)
    sd = torch.load(backbone_path, weights_only=True)
    sd["features.10.bias"] = torch.zeros(255)
    torch.save(sd, backbone_path)
    with pytest.raises(ValueError, match=r"features\.10\.bias.*\(255,\).*\(256,\)"):
        read_vgg_weights(lin_path, backbone_path)
    lin_path, backbone_path, _ = write_weights(tmp_path)
    sd = torch.load(backbone_path, weights_only=True)
    sd["features.5.weight"] = torch.zeros(128, 64, 5, 5)
    torch.save(sd, backbone_path)
    with pytest.raises(ValueError, match=r"features\.5\.weight"):
        read_vgg_weights(lin_path, backbone_path)


def test_loader_refuses_the_alexnet_heads(tmp_path):
    from ebfi_amd.lpips import read_vgg_weights
    _, backbone_path, _ = write_weights(tmp_path)
    z = np.load(ALEX_FIXTURE)
    alex = {"lin%d.model.1.weight" % l: torch.from_numpy(z["lin%d" % l]).reshape(1, -1, 1, 1) for l in range(5)}
    alex_path = str(tmp_path / "alex.pth")
    torch.save(alex, alex_path)
    with pytest.raises(ValueError, match=r"lin1\.model\.1\.weight.*192.*128"):
        read_vgg_weights(alex_path, backbone_path)


def test_load_lpips_dispatches_and_refuses_squeeze(tmp_path, monkeypatch):
    from ebfi_amd import lpips
    calls = []
    monkeypatch.setattr(lpips, "load_alex_lpips", lambda lin, trunk, device="cuda": calls.append(("alex", lin, trunk, device)))
    monkeypatch.setattr(lpips, "load_vgg_lpips", lambda lin, trunk, device="cuda": calls.append(("vgg", lin, trunk, device)))
    lpips.load_lpips("alex", "a", "b", device="cuda:0")
    lpips.load_lpips("vgg", "c", "d")
    assert calls == [("alex", "a", "b", "cuda:0"), ("vgg", "c", "d", "cuda")]
    with pytest.raises(NotImplementedError, match="squeeze"):
        lpips.load_lpips("squeeze", "a", "b")


def test_the_model_refuses_a_cpu_device():
    from ebfi_amd.lpips import VggLPIPS
    ws, bs = random_trunk(0)
    with pytest.raises(NotImplementedError, match="MI355X"):
        VggLPIPS(ws, bs, fixture_heads(), "cpu")


# ------------------------------------------------------------------ the C entry points' sizes and argument errors (no GPU touched)
@pytest.fixture(scope="module")
def lib():
    if not os.path.exists(N.LIB_PATH):
        N.build()
    return N.lib()


def test_sizes_are_host_arithmetic(lib):
    floats = sum(co * ci * 9 + co for co, ci, _, _ in CONV_SHAPES) + sum(HEAD_CHANNELS)
    assert floats == 14714688 + 1472
    got = lib.ebfi_lpips_vgg_params_bytes()
    assert got % 16 == 0 and 4 * floats <= got <= 4 * floats + (2 * 13 + 5) * 256      # (each array padded to 64 floats at most)
    # the scaled inputs and two maps of the largest layer, for both images of every pair
    need = lambda n, h, w: 4 * 2 * n * (3 + 2 * 64) * h * w      # noqa: E731
    for n, c, h, w in ((1, 3, 16, 16), (2, 1, 17, 19), (1, 3, 720, 1280), (16, 3, 256, 256)):
        ws = lib.ebfi_lpips_vgg_workspace(n, c, h, w)
        assert need(n, h, w) <= ws <= need(n, h, w) * 1.01 + 65536, (n, c, h, w, ws)
    assert lib.ebfi_lpips_vgg_workspace(0, 3, 16, 16) >= 0
    assert lib.ebfi_lpips_vgg_workspace(2, 3, 64, 64) <= 2 * lib.ebfi_lpips_vgg_workspace(1, 3, 64, 64)
    for bad in ((1, 2, 64, 64), (1, 3, 15, 64), (1, 1, 64, 15), (-1, 3, 64, 64), (1, 3, 2048, 2048), (16385, 3, 16, 16)):
        assert lib.ebfi_lpips_vgg_workspace(*bad) == 0, bad


def test_vgg_argument_errors(lib):
    p = ctypes.c_void_p(256)          # never dereferenced: every case below fails before a launch
    s = N.i64x4((3 * 64 * 64, 64 * 64, 64, 1))
    ws = lib.ebfi_lpips_vgg_workspace(2, 3, 64, 64)
    assert ws > 0

    def call(pred=p, ps=s, target=p, ts=s, n=2, c=3, h=64, w=64, params=p, work=p, nbytes=ws, out=p):
        return lib.ebfi_lpips_vgg(pred, ps, target, ts, n, c, h, w, 1, params, work, nbytes, out, None, None)

    assert call(pred=None) == -1 and b"null" in lib.ebfi_last_error()
    assert call(target=None) == -1 and call(params=None) == -1 and call(work=None) == -1 and call(out=None) == -1
    assert call(ps=None) == -1
    assert call(c=2) == -1 and b"C in {1, 3}" in lib.ebfi_last_error()
    assert call(h=15) == -1 and b"lpips_vgg" in lib.ebfi_last_error()
    assert call(w=15) == -1 and call(n=-1) == -1
    assert call(ts=N.i64x4((3 * 64 * 128, 64 * 128, 128, 2))) == -1 and b"column stride" in lib.ebfi_last_error()
    assert call(h=2048, w=2048, nbytes=1 << 62) == -1 and b"pixels" in lib.ebfi_last_error()
    assert call(nbytes=ws - 1) == -4 and b"workspace" in lib.ebfi_last_error()
    assert call(work=ctypes.c_void_p(264)) == -1 and b"aligned" in lib.ebfi_last_error()
    assert call(n=0, nbytes=0) == 0          # nothing to score: no launch


def test_pack_argument_errors(lib):
    ptrs = (ctypes.c_void_p * 13)(*([256] * 13))
    heads = (ctypes.c_void_p * 5)(*([256] * 5))
    holes = (ctypes.c_void_p * 13)(*([256] * 6 + [None] + [256] * 6))
    head_holes = (ctypes.c_void_p * 5)(256, None, 256, 256, 256)
    nbytes = lib.ebfi_lpips_vgg_params_bytes()
    out = ctypes.c_void_p(256)
    assert lib.ebfi_lpips_vgg_pack_params(ptrs, ptrs, heads, None, nbytes, None) == -1
    assert lib.ebfi_lpips_vgg_pack_params(None, ptrs, heads, out, nbytes, None) == -1
    assert lib.ebfi_lpips_vgg_pack_params(ptrs, holes, heads, out, nbytes, None) == -1
    assert b"convolution 7" in lib.ebfi_last_error()
    assert lib.ebfi_lpips_vgg_pack_params(ptrs, ptrs, head_holes, out, nbytes, None) == -1
    assert b"layer 2" in lib.ebfi_last_error()
    assert lib.ebfi_lpips_vgg_pack_params(ptrs, ptrs, heads, out, nbytes - 4, None) == -4
    assert lib.ebfi_lpips_vgg_pack_params(ptrs, ptrs, heads, ctypes.c_void_p(260), nbytes, None) == -1


def test_exports_are_declared_on_both_sides(lib):
    header = open(os.path.join(ROOT, "include", "ebfi_hip.h")).read()
    for name in ("ebfi_lpips_vgg_params_bytes", "ebfi_lpips_vgg_pack_params", "ebfi_lpips_vgg_workspace", "ebfi_lpips_vgg"):
        assert name in N.SIGNATURES and (name + "(") in header
        assert getattr(lib, name) is not None
    assert "#define EBFI_ABI_VERSION 14" in header
    assert N.SIGNATURES["ebfi_lpips_vgg"] == N.SIGNATURES["ebfi_lpips_alex"]


# ------------------------------------------------------------------ the shim and the command line
def test_shim_without_paths_still_raises():
    from loss import perceptual_loss
    with pytest.raises(NotImplementedError, match="LPIPS"):
        perceptual_loss(net="vgg")
    with pytest.raises(NotImplementedError, match="LPIPS"):
        perceptual_loss(net="vgg", lin_path="vgg.pth")


def test_shim_builds_through_load_lpips(monkeypatch):
    from ebfi_amd import lpips
    from loss import perceptual_loss
    seen = []
    monkeypatch.setattr(lpips, "load_lpips", lambda net, lin, trunk, device="cuda": seen.append((net, lin, trunk, device)) or "model")
    loss = perceptual_loss(weight=0.5, net="vgg", lin_path="vgg.pth", backbone_path="vgg16.pth", gpu_ids=[1])
    assert loss.model == "model" and loss.weight == 0.5
    assert seen == [("vgg", "vgg.pth", "vgg16.pth", "cuda:1")]
    monkeypatch.undo()
    with pytest.raises(NotImplementedError, match="squeeze"):
        perceptual_loss(net="squeeze", lin_path="squeeze.pth", backbone_path="squeezenet.pth")


@pytest.fixture(scope="module")
def cli():
    spec = importlib.util.spec_from_file_location("ebfi_infer_ours_lpips_vgg_host", os.path.join(PKG, "infer_ours.py"))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod


def test_cli_flag_parses_and_defaults_to_alex(cli):
    assert cli.get_flags([]).lpips_net == "alex"
    a = cli.get_flags(["--lpips_net", "vgg", "--lpips_lin", "vgg.pth", "--lpips_backbone", "vgg16.pth"])
    assert (a.lpips_net, a.lpips_lin, a.lpips_backbone) == ("vgg", "vgg.pth", "vgg16.pth")


def test_cli_refuses_squeeze(cli, capsys):
    with pytest.raises(SystemExit) as e:
        cli.get_flags(["--lpips_net", "squeeze"])
    assert e.value.code == 2 and "invalid choice" in capsys.readouterr().err


def test_cli_still_needs_both_weight_files_with_vgg(cli):
    with pytest.raises(SystemExit, match="both weight files"):
        cli.main(["--lpips_net", "vgg", "--lpips_lin", "vgg.pth", "--data_list", "list.txt", "--output_path", "out"])
