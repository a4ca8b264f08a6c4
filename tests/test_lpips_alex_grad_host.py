"""The LPIPS (AlexNet) training loss without a GPU: the new symbols and the training workspace's arithmetic, the argument errors
of ebfi_lpips_alex_forward_train / ebfi_lpips_alex_backward / ebfi_lpips_alex_pack_grad_params (with pointers that are never
dereferenced), the refusals of AlexLPIPSLoss.loss, load_lpips(train=True), the perceptual_loss shim's train keyword, the
train_ours.py --lpips_net flag, and the float64 / float32 autograd yardstick on the dead-pixel and the tied-maximum case."""
import ctypes
import importlib.util
import os
import types

import pytest
import torch

from ebfi_amd import _native as N
from lpips_alex_grad_ref import (CASES, dead_pixels, grad_out_of, make_pair, pair_errors, ref_grad, tied_windows, trunk_of)

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
PKG = os.path.join(ROOT, "ebfi-be_amd")
NEW = ("ebfi_lpips_alex_grad_params_bytes", "ebfi_lpips_alex_pack_grad_params", "ebfi_lpips_alex_train_workspace",
       "ebfi_lpips_alex_forward_train", "ebfi_lpips_alex_backward")


@pytest.fixture(scope="module")
def lib():
    if not os.path.exists(N.LIB_PATH):
        N.build()
    return N.lib()


def _case(kind):
    (case,) = [c for c in CASES if c[4] == kind]
    return case


# ------------------------------------------------------------------ the C entry points (no GPU touched)
def test_exports_are_declared_on_both_sides(lib):
    header = open(os.path.join(ROOT, "include", "ebfi_hip.h")).read()
    for name in NEW:
        assert name in N.SIGNATURES and (name + "(") in header
        assert getattr(lib, name) is not None
    assert "#define EBFI_ABI_VERSION 14" in header and lib.ebfi_abi_version() == 14
    assert N.SIGNATURES["ebfi_lpips_alex_forward_train"] == N.SIGNATURES["ebfi_lpips_alex"]
    assert N.SIGNATURES["ebfi_lpips_alex_train_workspace"] == N.SIGNATURES["ebfi_lpips_workspace"]


def test_train_workspace_is_host_arithmetic(lib):
    # the score's workspace and two gradient maps of N images, each the largest of f1 .. f5 (f1 here: 64 channels)
    for n, c, h, w in ((1, 3, 31, 31), (2, 1, 34, 38), (1, 3, 720, 1280), (8, 3, 256, 256)):
        train, score = lib.ebfi_lpips_alex_train_workspace(n, c, h, w), lib.ebfi_lpips_workspace(n, c, h, w)
        f1 = 64 * ((h - 7) // 4 + 1) * ((w - 7) // 4 + 1)
        assert train > score > 0 and train % 256 == 0, (n, c, h, w, train, score)
        assert score + 2 * 4 * n * f1 <= train <= score + 2 * 4 * n * f1 * 1.5 + 1024
    sizes = [lib.ebfi_lpips_alex_train_workspace(n, 3, 64, 80) for n in (0, 1, 2, 3, 8)]
    assert sizes[0] >= 0 and all(a < b for a, b in zip(sizes, sizes[1:]))               # monotone in N
    for bad in ((1, 3, 30, 31), (1, 3, 31, 30), (1, 2, 64, 64), (-1, 3, 64, 64)):
        assert lib.ebfi_lpips_alex_train_workspace(*bad) == 0 and lib.ebfi_lpips_workspace(*bad) == 0, bad
    # the score's sizes did not move
    kpad, cout = [368, 1600, 1728, 3456, 2304], [64, 192, 384, 256, 256]
    assert lib.ebfi_lpips_params_bytes() == 4 * sum(k * c + 2 * c for k, c in zip(kpad, cout))
    assert lib.ebfi_lpips_alex_grad_params_bytes() == 4 * (64 * 363 + 192 * 1600 + 384 * 1728 + 256 * 3456 + 256 * 2304)


def test_forward_train_argument_errors(lib):
    p = ctypes.c_void_p(256)          # never dereferenced: every case below fails before a launch
    s = N.i64x4((3 * 64 * 64, 64 * 64, 64, 1))
    ws = lib.ebfi_lpips_alex_train_workspace(2, 3, 64, 64)

    def call(pred=p, ps=s, target=p, ts=s, n=2, c=3, h=64, w=64, params=p, work=p, nbytes=ws, out=p):
        return lib.ebfi_lpips_alex_forward_train(pred, ps, target, ts, n, c, h, w, 1, params, work, nbytes, out, None, None)

    assert call(pred=None) == -1 and b"lpips_alex_forward_train: null" in lib.ebfi_last_error()
    assert call(target=None) == -1 and call(params=None) == -1 and call(work=None) == -1 and call(out=None) == -1
    assert call(ps=None) == -1 and call(ts=None) == -1
    assert call(c=2) == -1 and b"C in {1, 3}" in lib.ebfi_last_error()
    assert call(h=30) == -1 and call(w=30) == -1 and call(n=-1) == -1
    assert call(ps=N.i64x4((3 * 64 * 128, 64 * 128, 128, 2))) == -1 and b"column stride" in lib.ebfi_last_error()
    assert call(nbytes=ws - 1) == -4 and b"workspace" in lib.ebfi_last_error()
    assert call(nbytes=lib.ebfi_lpips_workspace(2, 3, 64, 64)) == -4          # the score's workspace is too small
    assert call(work=ctypes.c_void_p(264)) == -1 and b"aligned" in lib.ebfi_last_error()
    assert call(n=0, nbytes=0) == 0


def test_backward_and_pack_argument_errors(lib):
    p = ctypes.c_void_p(256)
    s = N.i64x4((3 * 64 * 64, 64 * 64, 64, 1))
    ws = lib.ebfi_lpips_alex_train_workspace(2, 3, 64, 64)

    def call(gout=p, params=p, gparams=p, work=p, nbytes=ws, n=2, c=3, h=64, w=64, gpred=p, gs=s):
        return lib.ebfi_lpips_alex_backward(gout, params, gparams, work, nbytes, n, c, h, w, 1, gpred, gs, None)

    assert call(gout=None) == -1 and b"lpips_alex_backward: null" in lib.ebfi_last_error()
    assert call(params=None) == -1 and call(gparams=None) == -1 and call(work=None) == -1
    assert call(gpred=None) == -1 and call(gs=None) == -1
    assert call(c=2) == -1 and b"C in {1, 3}" in lib.ebfi_last_error()
    assert call(h=30) == -1 and call(w=30) == -1 and call(n=-1) == -1
    assert call(gs=N.i64x4((3 * 64 * 128, 64 * 128, 128, 2))) == -1 and b"column stride" in lib.ebfi_last_error()
    assert call(nbytes=ws - 1) == -4 and b"workspace" in lib.ebfi_last_error()
    assert call(nbytes=lib.ebfi_lpips_workspace(2, 3, 64, 64)) == -4
    assert call(gparams=ctypes.c_void_p(264)) == -1 and b"aligned" in lib.ebfi_last_error()
    assert call(n=0, nbytes=0) == 0

    ptrs = (ctypes.c_void_p * 5)(*([256] * 5))
    holes = (ctypes.c_void_p * 5)(256, 256, None, 256, 256)
    nbytes = lib.ebfi_lpips_alex_grad_params_bytes()
    assert lib.ebfi_lpips_alex_pack_grad_params(None, p, nbytes, None) == -1
    assert lib.ebfi_lpips_alex_pack_grad_params(ptrs, None, nbytes, None) == -1
    assert lib.ebfi_lpips_alex_pack_grad_params(holes, p, nbytes, None) == -1 and b"layer 3" in lib.ebfi_last_error()
    assert lib.ebfi_lpips_alex_pack_grad_params(ptrs, p, nbytes - 4, None) == -4           # a short grad_params block


# ------------------------------------------------------------------ the Python layer
def test_loss_refuses_cpu_tensors_and_a_target_that_requires_grad():
    from ebfi_amd.lpips import AlexLPIPS, AlexLPIPSLoss
    assert issubclass(AlexLPIPSLoss, AlexLPIPS) and not hasattr(AlexLPIPS, "loss")
    model = AlexLPIPSLoss.__new__(AlexLPIPSLoss)       # (no device: both refusals come before anything of the model is read)
    x = torch.rand(1, 3, 31, 31)
    with pytest.raises(NotImplementedError, match="MI355X"):
        model.loss(x.clone().requires_grad_(True), x)
    with pytest.raises(ValueError, match="no gradient for the target"):
        model.loss(x, x.clone().requires_grad_(True))


def test_load_lpips_train_gives_the_loss_class(monkeypatch):
    from ebfi_amd import lpips
    made = []
    monkeypatch.setattr(lpips, "read_alex_weights", lambda lin, trunk: ("w", "b", "h"))
    monkeypatch.setattr(lpips, "read_vgg_weights", lambda lin, trunk: ("w", "b", "h"))
    for cls in (lpips.AlexLPIPS, lpips.AlexLPIPSLoss, lpips.VggLPIPS):
        monkeypatch.setattr(cls, "__init__", lambda self, w, b, h, device: made.append((type(self).__name__, device)))
    assert type(lpips.load_lpips("alex", "a", "b", device="cuda:0")) is lpips.AlexLPIPS
    assert type(lpips.load_lpips("alex", "a", "b", device="cuda:0", train=True)) is lpips.AlexLPIPSLoss
    assert type(lpips.load_alex_lpips("a", "b", device="cuda:0", train=True)) is lpips.AlexLPIPSLoss
    assert type(lpips.load_lpips("vgg", "a", "b", device="cuda:0", train=True)) is lpips.VggLPIPS        # train changes nothing
    assert [m[0] for m in made] == ["AlexLPIPS", "AlexLPIPSLoss", "AlexLPIPSLoss", "VggLPIPS"]
    with pytest.raises(NotImplementedError, match="squeeze"):
        lpips.load_lpips("squeeze", "a", "b", train=True)


def test_shim_takes_the_loss_path_for_alex_only_with_train(monkeypatch):
    from ebfi_amd import lpips
    from loss import perceptual_loss
    calls, loads = [], []

    class Fake:
        def __call__(self, pred, target, normalize=True):
            calls.append("score")
            return torch.ones(pred.shape[0])

        def loss(self, pred, target, normalize=True):
            calls.append("loss")
            return pred.mean((1, 2, 3))

    def load(net, lin, trunk, device="cuda", train=False):
        loads.append((net, train))
        return Fake()

    monkeypatch.setattr(lpips, "load_lpips", load)
    train = perceptual_loss(weight=2.0, net="alex", lin_path="a", backbone_path="b", train=True)
    score = perceptual_loss(weight=2.0, net="alex", lin_path="a", backbone_path="b")
    assert loads == [("alex", True), ("alex", False)]
    x, y = torch.rand(2, 3, 4, 4), torch.rand(2, 3, 4, 4)
    xg = x.clone().requires_grad_(True)
    assert float(train(x, y)) == 2.0 and calls == ["score"]                 # no requires_grad: the score
    with torch.no_grad():
        assert float(train(xg, y)) == 2.0 and calls == ["score"] * 2        # no grad mode: the score
    v = train(xg, y)
    assert calls[-1] == "loss" and v.requires_grad and float(v.detach()) == pytest.approx(2.0 * float(x.mean()), rel=1e-6)
    two = torch.rand(2, 2, 4, 4, requires_grad=True)
    v2 = train(two, torch.rand(2, 2, 4, 4))                     # two channels: the mean of per-channel calls differentiates
    assert calls[-2:] == ["loss", "loss"]
    v2.backward()
    assert two.grad is not None and torch.all(two.grad != 0)
    n = len(calls)
    assert float(score(xg, y)) == 2.0 and calls[n:] == ["score"]            # without train: what it returned before


# ------------------------------------------------------------------ train_ours.py
@pytest.fixture(scope="module")
def trainer():
    spec = importlib.util.spec_from_file_location("ebfi_train_ours_lpips_alex_host", os.path.join(PKG, "train_ours.py"))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod


def test_trainer_net_flag_parses_and_defaults_to_vgg(trainer):
    a = trainer.get_args([])
    assert a.lpips_net is None and trainer.perceptual_net({}, a) == "vgg"
    assert trainer.perceptual_settings({}, a) == (0.0, None, None)                       # still a 3-tuple
    alex = trainer.get_args(["--lpips_net", "alex"])
    assert alex.lpips_net == "alex" and trainer.perceptual_net({}, alex) == "alex"
    # the config key, and the flag over it
    assert trainer.perceptual_net({"trainer": {"lpips_net": "alex"}}, a) == "alex"
    assert trainer.perceptual_net({"trainer": {"lpips_net": "alex"}}, trainer.get_args(["--lpips_net", "vgg"])) == "vgg"
    assert trainer.perceptual_net({"trainer": {"lpips_net": "vgg"}}, alex) == "alex"
    for cfg, args in (({}, ["--lpips_net", "squeeze"]), ({"trainer": {"lpips_net": "resnet"}}, [])):
        with pytest.raises(SystemExit, match="lpips_net"):
            trainer.perceptual_net(cfg, trainer.get_args(args))


def test_trainer_names_the_alexnet_files_and_refuses_before_device_work(trainer, tmp_path):
    with pytest.raises(SystemExit, match="both weight files") as e:
        trainer.perceptual_settings({}, trainer.get_args(["--lpips_weight", "0.1", "--lpips_net", "alex"]))
    assert "alex.pth" in str(e.value) and "alexnet-owt-7be5be79.pth" in str(e.value) and "vgg" not in str(e.value)
    assert "missing --lpips_lin and --lpips_backbone" in str(e.value)
    with pytest.raises(SystemExit, match="both weight files") as e:
        trainer.perceptual_settings({}, trainer.get_args(["--lpips_weight", "0.1"]))
    assert "vgg.pth" in str(e.value) and "alex" not in str(e.value)                       # the default names what it named
    # main() refuses before it touches a device
    cfg = tmp_path / "cfg.yml"
    cfg.write_text("trainer: {lpips_weight: 0.1, lpips_net: alex}\n")
    with pytest.raises(SystemExit, match="alexnet-owt-7be5be79.pth"):
        trainer.main(["-c", str(cfg)])
    cfg.write_text("trainer: {lpips_net: squeeze}\n")
    with pytest.raises(SystemExit, match="lpips_net"):
        trainer.main(["-c", str(cfg)])


def test_trainer_builds_the_alex_term_and_its_log_note(trainer, monkeypatch, capsys):
    from ebfi_amd import lpips
    from ebfi_amd.loss import PerceptualTerm
    seen = []

    class Fake:
        def loss(self, pred, target, normalize=True):
            return pred.mean((1, 2, 3))

    monkeypatch.setattr(lpips, "load_alex_lpips", lambda lin, trunk, device="cuda", train=False: seen.append(("alex", train)) or Fake())
    monkeypatch.setattr(lpips, "load_vgg_lpips", lambda lin, trunk, device="cuda": seen.append(("vgg", None)) or Fake())
    term, note = trainer.perceptual_term("alex", "a", "b", 0.1, "cuda:0")
    assert isinstance(term, PerceptualTerm) and term.weight == 0.1 and note == " (with 0.1 x lpips_alex)"
    term, note = trainer.perceptual_term("vgg", "a", "b", 0.1, "cuda:0")
    assert isinstance(term, PerceptualTerm) and note == " (with 0.1 x lpips_vgg)"
    assert seen == [("alex", True), ("vgg", None)]

    monkeypatch.setattr(torch.cuda, "synchronize", lambda *a: None)          # (the loop waits for the device before it logs)
    monkeypatch.setattr(trainer, "save_checkpoint", lambda *a, **k: [])      # (and saves after the last iteration)

    class Eng:
        settled, VALID_KEYS = True, ()
        optimizer = types.SimpleNamespace(param_groups=[{"lr": 1e-4}])

        def train_step(self, *batch):
            return torch.tensor(0.5)

    st = {"iterations": 1, "accu_step": 1, "log_step": 1, "save_period": 0, "lr_change_rate": 1, "lr_min": 0.0}
    vs = {"do_validation": False}
    trainer.train_loop(Eng(), lambda it, micro: (), 1, "frames", st, vs, None, None, None, None, "", {}, 0, 1, 0,
                       loss_note=" (with 0.1 x lpips_alex)")
    assert "train_loss: 5.0000e-01 (with 0.1 x lpips_alex) learning rate" in capsys.readouterr().out


# ------------------------------------------------------------------ the yardstick
def test_yardstick_is_finite_on_dead_pixels():
    case = _case("dead")
    ws, bs, heads = trunk_of(case)
    pred, target, normalize = make_pair(case)
    dead, pixels = dead_pixels(pred, ws, bs, normalize)
    print("lpips_alex_grad yardstick: %d of %d f1 pixels of the dead case are all-zero" % (dead, pixels))
    assert dead >= pixels / 4
    go = grad_out_of(case[0])
    g64, lp = ref_grad(pred, target, ws, bs, heads, go, normalize)
    g32, _ = ref_grad(pred, target, ws, bs, heads, go, normalize, dtype=torch.float32)
    assert torch.isfinite(g64).all() and torch.isfinite(g32).all() and torch.isfinite(lp).all() and float(lp[0]) > 0
    assert g64.abs().max() > 0 and g64.shape == pred.shape
    (err,) = pair_errors(g32, g64)
    assert 0 < err < 1e-4


def test_yardstick_is_stable_under_tied_maxima():
    """pred = 0.5 everywhere: f1 is constant per channel away from the border, so most windows' maxima are tied and torch's
    first-maximum rule decides where the pooled gradient goes.  float32 and float64 autograd must take the same pixel."""
    case = _case("flat")
    ws, bs, heads = trunk_of(case)
    pred, target, normalize = make_pair(case)
    tied = tied_windows(pred, ws, bs, normalize)
    print("lpips_alex_grad yardstick: %d (window, channel) pairs of f1 of the flat case have a positive tied maximum" % tied)
    assert tied >= 100
    go = grad_out_of(case[0])
    g64, _ = ref_grad(pred, target, ws, bs, heads, go, normalize)
    g32, _ = ref_grad(pred, target, ws, bs, heads, go, normalize, dtype=torch.float32)
    (err,) = pair_errors(g32, g64)
    print("lpips_alex_grad yardstick: flat case float32-CPU error %.3e" % err)
    assert 0 < err < 1e-4


def test_yardstick_scales_with_grad_out_and_folds_one_channel():
    case = CASES[1]
    assert case[1] == 1
    ws, bs, heads = trunk_of(case)
    pred, target, normalize = make_pair(case)
    g, _ = ref_grad(pred, target, ws, bs, heads, grad_out_of(2), normalize)
    assert g.shape == pred.shape and g[0].abs().max() > 0 and torch.all(g[1] == 0)       # grad_out = (1.5, 0)
    assert torch.all(g[:, :, 33] == 0) and g[0, :, 32].abs().max() > 0                   # row 33: in no conv1 window
    one, _ = ref_grad(pred, target, ws, bs, heads, torch.tensor([1.0, 1.0]), normalize)
    assert torch.allclose(g[0], 1.5 * one[0], rtol=1e-12, atol=0)
    three, _ = ref_grad(pred.repeat(1, 3, 1, 1), target.repeat(1, 3, 1, 1), ws, bs, heads, torch.tensor([1.0, 1.0]), normalize)
    assert torch.allclose(one, three.sum(1, keepdim=True), rtol=1e-10, atol=1e-18)
