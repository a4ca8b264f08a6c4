"""The LPIPS (VGG-16) training loss without a GPU: the training workspace's arithmetic, the argument errors of
ebfi_lpips_vgg_forward_train / ebfi_lpips_vgg_backward (with pointers that are never dereferenced), the refusals of VggLPIPS.loss
and PerceptualTerm, the train_ours.py flags, and the float64 / float32 autograd yardstick on the dead-pixel case."""
import ctypes
import importlib.util
import os
import types

import pytest
import torch

from ebfi_amd import _native as N
from lpips_vgg_grad_ref import CASES, dead_pixels, grad_out_of, make_pair, pair_errors, ref_grad, trunk_of

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
PKG = os.path.join(ROOT, "ebfi-be_amd")


@pytest.fixture(scope="module")
def lib():
    if not os.path.exists(N.LIB_PATH):
        N.build()
    return N.lib()


# ------------------------------------------------------------------ the C entry points (no GPU touched)
def test_train_workspace_is_host_arithmetic(lib):
    # the 13 ReLU maps of the pred images and the 5 tap maps of the target images, in floats per pixel of the input:
    # 64 + 64 + (128 + 128) / 4 + 3 * 256 / 16 + 3 * 512 / 64 + 3 * 512 / 256 and 64 + 128 / 4 + 256 / 16 + 512 / 64 + 512 / 256
    for n, c, h, w in ((1, 3, 16, 16), (2, 1, 32, 64), (1, 3, 720, 1280), (8, 3, 256, 256)):
        train, score = lib.ebfi_lpips_vgg_train_workspace(n, c, h, w), lib.ebfi_lpips_vgg_workspace(n, c, h, w)
        kept = 4 * n * (270 + 122) * h * w
        assert train > score > 0 and train >= kept, (n, c, h, w, train, score)
        assert train <= kept + 4 * n * (6 + 2 * 64 + 16) * h * w * 1.01 + 65536     # + x', two maps, the pooled map, sums, flags
        assert train % 256 == 0
    assert lib.ebfi_lpips_vgg_train_workspace(0, 3, 16, 16) >= 0
    for bad in ((1, 2, 64, 64), (1, 3, 15, 64), (1, 1, 64, 15), (-1, 3, 64, 64), (1, 3, 2048, 2048), (16385, 3, 16, 16)):
        assert lib.ebfi_lpips_vgg_workspace(*bad) == 0 and lib.ebfi_lpips_vgg_train_workspace(*bad) == 0, bad


def test_forward_train_argument_errors(lib):
    p = ctypes.c_void_p(256)          # never dereferenced: every case below fails before a launch
    s = N.i64x4((3 * 64 * 64, 64 * 64, 64, 1))
    ws = lib.ebfi_lpips_vgg_train_workspace(2, 3, 64, 64)

    def call(pred=p, ps=s, target=p, ts=s, n=2, c=3, h=64, w=64, params=p, work=p, nbytes=ws, out=p):
        return lib.ebfi_lpips_vgg_forward_train(pred, ps, target, ts, n, c, h, w, 1, params, work, nbytes, out, None, None)

    assert call(pred=None) == -1 and b"lpips_vgg_forward_train: null" in lib.ebfi_last_error()
    assert call(target=None) == -1 and call(params=None) == -1 and call(work=None) == -1 and call(out=None) == -1
    assert call(ps=None) == -1 and call(ts=None) == -1
    assert call(c=2) == -1 and b"C in {1, 3}" in lib.ebfi_last_error()
    assert call(h=15) == -1 and call(w=15) == -1 and call(n=-1) == -1
    assert call(ps=N.i64x4((3 * 64 * 128, 64 * 128, 128, 2))) == -1 and b"column stride" in lib.ebfi_last_error()
    assert call(h=2048, w=2048, nbytes=1 << 62) == -1 and b"pixels" in lib.ebfi_last_error()
    assert call(nbytes=ws - 1) == -4 and b"workspace" in lib.ebfi_last_error()
    assert call(nbytes=lib.ebfi_lpips_vgg_workspace(2, 3, 64, 64)) == -4          # the evaluation workspace is too small
    assert call(work=ctypes.c_void_p(264)) == -1 and b"aligned" in lib.ebfi_last_error()
    assert call(n=0, nbytes=0) == 0


def test_backward_argument_errors(lib):
    p = ctypes.c_void_p(256)
    s = N.i64x4((3 * 64 * 64, 64 * 64, 64, 1))
    ws = lib.ebfi_lpips_vgg_train_workspace(2, 3, 64, 64)

    def call(gout=p, params=p, work=p, nbytes=ws, n=2, c=3, h=64, w=64, gpred=p, gs=s):
        return lib.ebfi_lpips_vgg_backward(gout, params, work, nbytes, n, c, h, w, 1, gpred, gs, None)

    assert call(gout=None) == -1 and b"lpips_vgg_backward: null" in lib.ebfi_last_error()
    assert call(params=None) == -1 and call(work=None) == -1 and call(gpred=None) == -1 and call(gs=None) == -1
    assert call(c=2) == -1 and b"C in {1, 3}" in lib.ebfi_last_error()
    assert call(h=15) == -1 and call(w=15) == -1 and call(n=-1) == -1
    assert call(gs=N.i64x4((3 * 64 * 128, 64 * 128, 128, 2))) == -1 and b"column stride" in lib.ebfi_last_error()
    assert call(h=2048, w=2048, nbytes=1 << 62) == -1 and b"pixels" in lib.ebfi_last_error()
    assert call(nbytes=ws - 1) == -4 and b"workspace" in lib.ebfi_last_error()
    assert call(work=ctypes.c_void_p(264)) == -1 and b"aligned" in lib.ebfi_last_error()
    assert call(n=0, nbytes=0) == 0


def test_exports_are_declared_on_both_sides(lib):
    header = open(os.path.join(ROOT, "include", "ebfi_hip.h")).read()
    for name in ("ebfi_lpips_vgg_train_workspace", "ebfi_lpips_vgg_forward_train", "ebfi_lpips_vgg_backward"):
        assert name in N.SIGNATURES and (name + "(") in header
        assert getattr(lib, name) is not None
    assert "#define EBFI_ABI_VERSION 14" in header
    assert N.SIGNATURES["ebfi_lpips_vgg_forward_train"] == N.SIGNATURES["ebfi_lpips_vgg"]
    assert N.SIGNATURES["ebfi_lpips_vgg_train_workspace"] == N.SIGNATURES["ebfi_lpips_vgg_workspace"]


# ------------------------------------------------------------------ the Python layer's refusals
def test_loss_refuses_cpu_tensors_and_a_target_that_requires_grad():
    from ebfi_amd.lpips import AlexLPIPS, VggLPIPS
    model = VggLPIPS.__new__(VggLPIPS)                # (no device: both refusals come before anything of the model is read)
    x = torch.rand(1, 3, 16, 16)
    with pytest.raises(NotImplementedError, match="MI355X"):
        model.loss(x.clone().requires_grad_(True), x)
    with pytest.raises(ValueError, match="no gradient for the target"):
        model.loss(x, x.clone().requires_grad_(True))
    assert not hasattr(AlexLPIPS, "loss")              # the AlexNet trunk stays forward-only


def test_perceptual_term_needs_a_model_with_a_backward_and_a_positive_weight():
    from ebfi_amd.loss import PerceptualTerm
    seen = []

    class Model:
        def loss(self, pred, target, normalize=True):
            seen.append((target.requires_grad, normalize))
            return (pred - target).abs().mean((1, 2, 3))

    term = PerceptualTerm(Model(), 0.25)
    pred, target = torch.rand(2, 3, 4, 4, requires_grad=True), torch.rand(2, 3, 4, 4)
    v = term(pred, target)
    assert v.dim() == 0 and seen == [(False, True)]
    assert float(v.detach()) == pytest.approx(0.25 * float((pred - target).detach().abs().mean()), rel=1e-6)
    v.backward()
    assert pred.grad is not None
    with pytest.raises(NotImplementedError, match="score only"):
        PerceptualTerm(object(), 0.25)
    for bad in (0.0, -1.0, float("nan")):
        with pytest.raises(ValueError, match="positive"):
            PerceptualTerm(Model(), bad)


def test_shim_takes_the_loss_path_only_for_vgg_with_grad(monkeypatch):
    from ebfi_amd import lpips
    from loss import perceptual_loss
    calls = []

    class Fake:
        def __init__(self, net):
            self.NET = net

        def __call__(self, pred, target, normalize=True):
            calls.append("score")
            return torch.ones(pred.shape[0])

        def loss(self, pred, target, normalize=True):
            calls.append("loss")
            return pred.mean((1, 2, 3))

    monkeypatch.setattr(lpips, "load_lpips", lambda net, lin, trunk, device="cuda": Fake(net))
    vgg = perceptual_loss(weight=2.0, net="vgg", lin_path="a", backbone_path="b")
    alex = perceptual_loss(weight=2.0, net="alex", lin_path="a", backbone_path="b")
    x, y = torch.rand(2, 3, 4, 4), torch.rand(2, 3, 4, 4)
    xg = x.clone().requires_grad_(True)
    assert float(vgg(x, y)) == 2.0 and calls == ["score"]
    with torch.no_grad():
        assert float(vgg(xg, y)) == 2.0 and calls == ["score"] * 2
    v = vgg(xg, y)
    assert calls[-1] == "loss" and v.requires_grad and float(v.detach()) == pytest.approx(2.0 * float(x.mean()), rel=1e-6)
    two = torch.rand(2, 2, 4, 4, requires_grad=True)
    v2 = vgg(two, torch.rand(2, 2, 4, 4))                       # two channels: the mean of per-channel calls differentiates
    assert calls[-2:] == ["loss", "loss"]
    v2.backward()
    assert two.grad is not None and torch.all(two.grad != 0)
    n = len(calls)
    assert float(alex(xg, y)) == 2.0 and calls[n:] == ["score"]    # alex: what it returned before, with or without grad


# ------------------------------------------------------------------ train_ours.py
@pytest.fixture(scope="module")
def trainer():
    spec = importlib.util.spec_from_file_location("ebfi_train_ours_lpips_host", os.path.join(PKG, "train_ours.py"))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod


def test_trainer_flags_parse_and_default_to_off(trainer):
    a = trainer.get_args([])
    assert (a.lpips_weight, a.lpips_lin, a.lpips_backbone) == (None, None, None)
    assert trainer.perceptual_settings({}, a) == (0.0, None, None)
    assert trainer.perceptual_settings({"trainer": {"lpips_weight": 0}}, a) == (0.0, None, None)
    a = trainer.get_args(["--lpips_weight", "0.1", "--lpips_lin", "vgg.pth", "--lpips_backbone", "vgg16.pth"])
    assert trainer.perceptual_settings({}, a) == (0.1, "vgg.pth", "vgg16.pth")
    # the config key, and the flag over it
    files = trainer.get_args(["--lpips_lin", "vgg.pth", "--lpips_backbone", "vgg16.pth"])
    assert trainer.perceptual_settings({"trainer": {"lpips_weight": 0.05}}, files)[0] == 0.05
    assert trainer.perceptual_settings({"trainer": {"lpips_weight": 0.05}}, a)[0] == 0.1
    off = trainer.get_args(["--lpips_weight", "0"])
    assert trainer.perceptual_settings({"trainer": {"lpips_weight": 0.05}}, off) == (0.0, None, None)


def test_trainer_refuses_a_weight_without_both_files(trainer, tmp_path):
    for extra, missing in (([], "--lpips_lin and --lpips_backbone"), (["--lpips_lin", "vgg.pth"], "missing --lpips_backbone"),
                           (["--lpips_backbone", "vgg16.pth"], "missing --lpips_lin")):
        with pytest.raises(SystemExit, match="both weight files") as e:
            trainer.perceptual_settings({}, trainer.get_args(["--lpips_weight", "0.1"] + extra))
        assert missing in str(e.value)
    with pytest.raises(SystemExit, match="both weight files"):
        trainer.perceptual_settings({"trainer": {"lpips_weight": 0.2}}, trainer.get_args([]))
    with pytest.raises(SystemExit, match="negative"):
        trainer.perceptual_settings({}, trainer.get_args(["--lpips_weight", "-1"]))
    # main() refuses before it touches a device
    cfg = tmp_path / "cfg.yml"
    cfg.write_text("trainer: {lpips_weight: 0.1}\n")
    with pytest.raises(SystemExit, match="both weight files"):
        trainer.main(["-c", str(cfg)])


def test_log_line_names_the_term(trainer, capsys, monkeypatch):
    monkeypatch.setattr(torch.cuda, "synchronize", lambda *a: None)          # (the loop waits for the device before it logs)
    monkeypatch.setattr(trainer, "save_checkpoint", lambda *a, **k: [])      # (and saves after the last iteration)
    class Eng:
        settled, VALID_KEYS = True, ()
        optimizer = types.SimpleNamespace(param_groups=[{"lr": 1e-4}])

        def train_step(self, *batch):
            return torch.tensor(0.5)

    st = {"iterations": 1, "accu_step": 1, "log_step": 1, "save_period": 0, "lr_change_rate": 1, "lr_min": 0.0}
    vs = {"do_validation": False}
    for note in ("", " (with 0.1 x lpips_vgg)"):
        trainer.train_loop(Eng(), lambda it, micro: (), 1, "frames", st, vs, None, None, None, None, "", {}, 0, 1, 0, loss_note=note)
        out = capsys.readouterr().out
        assert ("train_loss: 5.0000e-01%s learning rate" % note) in out and ("lpips_vgg" in out) == bool(note)


# ------------------------------------------------------------------ the yardstick
def test_yardstick_is_finite_on_dead_pixels():
    case = CASES[-1]
    assert case[4] == "dead"
    ws, bs, heads = trunk_of(case)
    pred, target, normalize = make_pair(case)
    dead = dead_pixels(pred, ws, bs, normalize)
    print("lpips_vgg_grad yardstick: %d of %d f1 pixels of the dead case are all-zero" % (dead, case[2] * case[3]))
    assert dead >= case[2] * case[3] // 4
    go = grad_out_of(case[0])
    g64, lp = ref_grad(pred, target, ws, bs, heads, go, normalize)
    g32, _ = ref_grad(pred, target, ws, bs, heads, go, normalize, dtype=torch.float32)
    assert torch.isfinite(g64).all() and torch.isfinite(g32).all() and torch.isfinite(lp).all() and float(lp[0]) > 0
    assert g64.abs().max() > 0 and g64.shape == pred.shape
    (err,) = pair_errors(g32, g64)
    assert 0 < err < 1e-4


def test_yardstick_scales_with_grad_out_and_folds_one_channel():
    case = CASES[1]
    ws, bs, heads = trunk_of(case)
    pred, target, normalize = make_pair(case)
    g, _ = ref_grad(pred, target, ws, bs, heads, grad_out_of(2), normalize)
    assert g.shape == pred.shape and g[0].abs().max() > 0 and torch.all(g[1] == 0)       # grad_out = (1.5, 0)
    one, _ = ref_grad(pred, target, ws, bs, heads, torch.tensor([1.0, 1.0]), normalize)
    assert torch.allclose(g[0], 1.5 * one[0], rtol=1e-12, atol=0)
    three, _ = ref_grad(pred.repeat(1, 3, 1, 1), target.repeat(1, 3, 1, 1), ws, bs, heads, torch.tensor([1.0, 1.0]), normalize)
    assert torch.allclose(one, three.sum(1, keepdim=True), rtol=1e-10, atol=1e-18)
