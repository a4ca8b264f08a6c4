"""Gradient clipping by total norm and the moving average of the weights without a GPU: the header and the library's exports,
the entry points' host side (every refusal returns before a launch), the config keys and flags of both trainers, the CPU path
of FlatOptimizer against the numpy restatement (tests/gradclip_ref.py), the `ema` key of the checkpoints and the monitor's
second ring."""
import ctypes
import importlib.util
import os

import numpy as np
import pytest
import torch

import gradclip_ref as GR
from ebfi_amd import _native as N
from ebfi_amd import dp
from ebfi_amd.graphstep import GraphStepper

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
PKG = os.path.join(ROOT, "ebfi-be_amd")
INF = float("inf")


def _trainer(name="train_ours"):
    spec = importlib.util.spec_from_file_location("ebfi_%s_gradclip" % name, os.path.join(PKG, name + ".py"))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod


# ------------------------------------------------------------------ header, exports, host side of the entry points
def test_new_symbols_are_declared_bound_and_exported():
    new = {"ebfi_grad_norm_workspace", "ebfi_grad_norm", "ebfi_optim_step_ex"}
    assert new <= set(N.declared_symbols()) and new <= set(N.SIGNATURES)
    assert N.CONSTANTS["EBFI_NORM_L2"] == 0 and N.CONSTANTS["EBFI_NORM_INF"] == 1 and N.CONSTANTS["EBFI_GRAD_NORM_CHUNK"] == 16384
    assert N.CONSTANTS["EBFI_ABI_VERSION"] == 14          # a pure addition: the ABI generation does not move
    assert len(N.SIGNATURES["ebfi_optim_step_ex"][1]) == len(N.SIGNATURES["ebfi_optim_step"][1]) + 5
    assert N.PARAMS["ebfi_optim_step_ex"][:18] == N.PARAMS["ebfi_optim_step"][:18]
    if not os.path.exists(N.LIB_PATH):
        N.build()
    h = ctypes.CDLL(N.LIB_PATH)
    for name in new | {"ebfi_optim_step"}:
        assert hasattr(h, name), name
    assert N.lib().ebfi_abi_version() == 14


def test_norm_workspace_arithmetic_and_argument_errors_touch_no_gpu():
    lib = N.lib()
    chunk = N.CONSTANTS["EBFI_GRAD_NORM_CHUNK"]
    assert [lib.ebfi_grad_norm_workspace(n) for n in (-1, 0, 1, chunk, chunk + 1, 3 * chunk + 5)] == [0, 0, 8, 8, 16, 32]
    p = ctypes.c_void_p(16)
    args = lambda **kw: [kw.get("g", p), kw.get("n", 8), kw.get("kind", 0), kw.get("max_norm", 1.0), kw.get("out", p),
                         kw.get("ws", p), kw.get("bytes", 1 << 20), None]
    assert lib.ebfi_grad_norm(*args(n=-1)) == -1
    assert lib.ebfi_grad_norm(*args(kind=2)) == -1 and b"norm_kind" in lib.ebfi_last_error()
    for bad in (0.0, -1.0, float("nan")):
        assert lib.ebfi_grad_norm(*args(max_norm=bad)) == -1 and b"max_norm" in lib.ebfi_last_error()
    assert lib.ebfi_grad_norm(*args(out=None)) == -1 and lib.ebfi_grad_norm(*args(g=None)) == -1
    assert b"null" in lib.ebfi_last_error()
    assert lib.ebfi_grad_norm(*args(g=ctypes.c_void_p(8))) == -1
    assert lib.ebfi_grad_norm(*args(ws=None)) == -4
    assert lib.ebfi_grad_norm(*args(ws=ctypes.c_void_p(8))) == -1
    assert lib.ebfi_grad_norm(*args(bytes=4)) == -4 and lib.ebfi_grad_norm(*args(n=chunk + 1, bytes=8)) == -4


def test_step_ex_argument_errors_touch_no_gpu():
    lib = N.lib()
    p, odd = ctypes.c_void_p(16), ctypes.c_void_p(8)

    def call(kind=0, flags=0, param=p, grad=p, s0=p, s1=p, s2=None, step=p, n=8, wd=0.0, mom=0.0, damp=0.0, guard=None, flag=None,
             scale=p, ema=None, ema_step=None, decay=0.9, warmup=0):
        return lib.ebfi_optim_step_ex(kind, flags, param, grad, s0, s1, s2, step, n, 1e-3, 0.9, 0.999, 1e-8, wd, mom, damp, guard, flag,
                                      scale, ema, ema_step, decay, warmup, None)
    assert call(kind=2) == -3
    assert call(flags=4) == -1 and call(kind=1, flags=2) == -1 and call(flags=8) == -1
    assert call(wd=-1.0) == -1 and call(flag=p) == -1 and call(param=None) == -1 and call(grad=odd) == -1 and call(n=-1) == -1
    assert call(flags=2) == -1 and call(s0=None) == -1 and call(step=None) == -1          # AMSGrad without its buffer, Adam without state
    assert call(kind=1, flags=4) == -1 and call(kind=1, mom=0.9, s0=None) == -1 and call(kind=1, mom=-0.5) == -1
    assert call(ema=p) == -1 and b"step word" in lib.ebfi_last_error()                    # an average without its count
    assert call(ema=odd, ema_step=p) == -1
    for bad in (1.0, -0.1, float("nan"), 1.5):
        assert call(ema=p, ema_step=p, decay=bad) == -1 and b"ema_decay" in lib.ebfi_last_error()
    assert call(scale=None, ema=p, ema_step=p, decay=bad) == -1                           # (also without a scale)
    # nothing to do: accepted, and still no launch (n == 0), with either addition and through the forwarding route
    assert call(n=0) == 0 and call(n=0, scale=None, ema=p, ema_step=p) == 0 and call(n=0, scale=None) == 0
    assert call(kind=1, n=0, mom=0.9, flags=4) == 0


# ------------------------------------------------------------------ settings
def test_clip_and_ema_arguments():
    assert dp.clip_arguments(None) is None and dp.ema_arguments(None) is None
    assert dp.clip_arguments((1.5, 2)) == (1.5, 2.0) and dp.clip_arguments((3, INF)) == (3.0, INF)
    assert dp.clip_arguments({"max_norm": 0.5}) == (0.5, 2.0) and dp.clip_arguments({"max_norm": 1, "norm_type": "inf"}) == (1.0, INF)
    assert dp.ema_arguments((0.999, True)) == (0.999, True) and dp.ema_arguments({"decay": 0.0}) == (0.0, False)
    for bad in ((0.0, 2), (-1.0, 2), (float("nan"), 2), (INF, 2), (1.0, 1), (1.0, 3), (1.0, -INF), {"norm_type": 2}, {"max_norm": 1, "p": 2},
                (1.0,), "x"):
        with pytest.raises(ValueError):
            dp.clip_arguments(bad)
    for bad in ((1.0, False), (-0.01, False), (float("nan"), True), (1.5, True), {"warmup": True}, (0.5,), "x"):
        with pytest.raises(ValueError):
            dp.ema_arguments(bad)
    w = torch.nn.Parameter(torch.zeros(4))
    for kw in ({"clip": (0.0, 2)}, {"clip": (1.0, 1)}, {"ema": (1.0, False)}):
        with pytest.raises(ValueError):
            dp.FlatOptimizer([w], "Adam", **kw)
    assert w.untyped_storage().data_ptr() == w.data_ptr()                # refused before anything was re-pointed


@pytest.mark.parametrize("script", ["train_ours", "train_ours_exposuredecision"])
def test_config_keys_and_flags(script):
    import yaml
    T = _trainer(script)
    parse = (lambda argv: T.get_args(argv)) if script == "train_ours" else (lambda argv: T.build_parser().parse_args(argv))
    off = {"clip_grad": None, "ema": None, "ema_validate": True}
    assert T.averaging_settings({}, parse([])) == off and T.averaging_settings({"trainer": None}) == off
    shipped = yaml.safe_load(open(os.path.join(PKG, "config", script + ".yml")))
    assert T.averaging_settings(shipped, parse([])) == off                # both features are off by default
    cfg = {"trainer": {"clip_grad": {"max_norm": 2.0, "norm_type": INF}, "ema": {"decay": 0.99, "warmup": True, "validate": False}}}
    assert T.averaging_settings(cfg, parse([])) == {"clip_grad": (2.0, INF), "ema": (0.99, True), "ema_validate": False}
    got = T.averaging_settings(cfg, parse(["--clip-grad-norm", "0.5", "--ema-decay", "0.9"]))
    assert got == {"clip_grad": (0.5, INF), "ema": (0.9, True), "ema_validate": False}      # the flags override one value each
    got = T.averaging_settings({}, parse(["--clip-grad-norm", "0.5", "--ema-decay", "0.9"]))
    assert got == {"clip_grad": (0.5, 2.0), "ema": (0.9, False), "ema_validate": True}
    assert T.averaging_settings(yaml.safe_load("trainer: {clip_grad: {max_norm: 1, norm_type: .inf}}"))["clip_grad"] == (1.0, INF)
    for bad in ({"clip_grad": {"max_norm": 0}}, {"clip_grad": {"max_norm": 1, "norm_type": 1}}, {"ema": {"decay": 1.0}},
                {"ema": {"decay": 0.9, "momentum": 1}}, {"clip_grad": {"norm_type": 2}}, {"ema": {"warmup": True}}):
        with pytest.raises(ValueError):
            T.averaging_settings({"trainer": bad}, parse([]))
    for argv in (["--clip-grad-norm", "0"], ["--clip-grad-norm", "-1"], ["--ema-decay", "1"], ["--ema-decay", "-0.5"]):
        with pytest.raises(ValueError):
            T.averaging_settings({}, parse(argv))


# ------------------------------------------------------------------ the CPU path against the restatement
@pytest.mark.parametrize("norm_type", [2, INF], ids=["l2", "inf"])
@pytest.mark.parametrize("warmup", [False, True], ids=["fixed", "warmup"])
@pytest.mark.parametrize("name,args", [("AdamW", {"weight_decay": 1e-2}), ("SGD", {"momentum": 0.9})], ids=["adamw", "sgd"])
def test_cpu_path_follows_the_restatement(name, args, warmup, norm_type):
    n, steps, skipped_at = 37, 5, 2
    g = torch.Generator().manual_seed(7)
    p0 = torch.randn(n, generator=g)
    grads = [torch.randn(n, generator=g) * (10.0 if k % 2 == 0 else 1e-3) for k in range(steps)]
    opt = dp.FlatOptimizer([torch.nn.Parameter(p0.clone())], name, clip=(0.7, norm_type), ema=(0.9, warmup), lr=1e-2, **args)
    assert torch.equal(opt.ema_flat, p0) and float(opt.ema_step) == 0 and opt.last_grad_norm.tolist() == [0.0, 1.0]
    twin = torch.nn.Parameter(p0.clone())                                 # the torch class itself on pre-scaled gradients
    inner = getattr(torch.optim, name)([twin], lr=1e-2, **args)
    ref = GR.EmaRef(p0.numpy(), 0.9, warmup)
    guard = torch.zeros(2, dtype=torch.int32)
    clipped = 0
    for k, grad in enumerate(grads):
        keep = grad.clone()
        skip = k == skipped_at
        guard[0] = 1 if skip else 0
        before = (opt.flat.detach().clone(), opt.ema_flat.clone(), float(opt.ema_step))
        opt.step(grad, guard=guard, flag=torch.zeros(1))
        assert torch.equal(grad, keep)                                    # the packed gradient stays unclipped
        norm64 = GR.total_norm(grad.numpy(), norm_type)
        got = opt.last_grad_norm.numpy()
        assert got[0] in GR.norm_candidates(norm64) and got[1] == GR.clip_coef(got[0], 0.7)
        clipped += got[1] < 1
        if skip:
            assert torch.equal(opt.flat.detach(), before[0]) and torch.equal(opt.ema_flat, before[1]) and float(opt.ema_step) == before[2]
        else:
            twin.grad = grad * torch.tensor(got[1])
            inner.step()
            assert torch.equal(opt.flat.detach(), twin.detach())
        want = ref.update(opt.flat.detach().numpy(), skipped=skip)
        assert np.array_equal(opt.ema_flat.numpy().view(np.uint32), want.view(np.uint32)), k
    assert float(opt.ema_step) == ref.step == steps - 1 and guard.tolist() == [0, 1]
    assert 0 < clipped < steps                                            # both branches of the coefficient ran
    assert not torch.equal(opt.ema_flat, opt.flat.detach())


def test_restatement_edge_values():
    assert GR.total_norm(np.zeros(0, np.float32)) == 0.0 and GR.clip_coef(0.0, 1.0) == 1.0
    assert GR.total_norm(np.full(5, 3e25, np.float32)) == pytest.approx(3e25 * 5 ** 0.5, rel=1e-6)
    assert GR.total_norm(np.full(4, 1e-30, np.float32)) == pytest.approx(2e-30, rel=1e-6)
    assert np.isnan(GR.total_norm(np.array([1, np.nan, 2], np.float32), INF)) and np.isnan(GR.total_norm(np.array([np.nan], np.float32)))
    assert GR.total_norm(np.array([1, -np.inf], np.float32), INF) == np.inf
    assert np.isnan(GR.clip_coef(np.nan, 1.0)) and GR.clip_coef(np.inf, 1.0) == 0.0
    assert GR.clip_coef(np.float32(4.0), 1.0) == np.float32(1.0) / (np.float32(4.0) + np.float32(1e-6))
    assert [GR.ema_decay_at(0.999, True, t) for t in (1, 2)] == [2 / 11, 3 / 12] and GR.ema_decay_at(0.5, True, 100) == 0.5


# ------------------------------------------------------------------ checkpoints, through the stepper the engines share
class TinyEngine(GraphStepper):
    """The optimiser path of the engines over a two-layer host model (one buffer that is not a parameter)."""
    VALID_KEYS = ("valid_loss",)

    def __init__(self, clip_grad=None, ema=None, seed=0):
        super().__init__("cpu")
        torch.manual_seed(seed)
        self.precision, self.bank = "fp32", None
        self.model = torch.nn.Sequential(torch.nn.Linear(3, 4), torch.nn.BatchNorm1d(4), torch.nn.Linear(4, 2))
        self.bucket = dp.FlatGradBucket(self.model)
        self.optimizer = dp.build_flat_optimizer(self.bucket.params, None, 1e-2, (0.9, 0.999), clip=clip_grad, ema=ema)

    def _fwd_bwd(self, x, y):
        loss = ((self.model(x) - y) ** 2).mean() / self.accu_step
        loss.backward()
        return loss.detach()


def _steps(eng, count, seed=0):
    g = torch.Generator().manual_seed(seed)
    for _ in range(count):
        eng.train_step(torch.randn(5, 3, generator=g), torch.randn(5, 2, generator=g))


CONFIG = {"model": {"name": "Tiny"}, "optimizer": {"name": "Adam"}}


def test_checkpoint_round_trip_with_the_ema_key(tmp_path):
    T = _trainer()
    eng = TinyEngine(clip_grad=(0.05, 2), ema=(0.9, True))
    _steps(eng, 4)
    assert float(eng.optimizer.last_grad_norm[1]) < 1                     # the clip was in effect
    path = str(tmp_path / "m" / "checkpoint-iteration3.pth")
    paths = T.save_checkpoint(path, eng, None, CONFIG, 3, None, save_best=True)
    assert [os.path.basename(p) for p in paths] == ["checkpoint-iteration3.pth", "model_best_until_iteration3.pth"]
    trainable = [n for n, p in eng.model.named_parameters()]
    for p in paths:                                                       # the best checkpoint carries both too
        cpt = torch.load(p, weights_only=False)
        assert tuple(cpt) == T.CHECKPOINT_KEYS + ("ema",)
        ema = cpt["ema"]
        assert set(ema) == {"decay", "warmup", "step", "states"} and (ema["decay"], ema["warmup"], ema["step"]) == (0.9, True, 4)
        assert list(ema["states"]) == trainable and "1.running_mean" in cpt["model"]["states"] and "1.running_mean" not in ema["states"]
        for (n, v), e in zip(eng.model.named_parameters(), eng.optimizer.ema_views()):
            assert torch.equal(cpt["model"]["states"][n], v) and torch.equal(ema["states"][n], e)      # model.states: the raw iterate
            assert not torch.equal(ema["states"][n], v)
    # --resume restores the average and its count; the next step is the one the first run takes
    again = TinyEngine(clip_grad=(0.05, 2), ema=(0.9, True), seed=1)
    assert T.resume_checkpoint(path, again, None, CONFIG) == 4
    assert torch.equal(again.optimizer.ema_flat, eng.optimizer.ema_flat) and float(again.optimizer.ema_step) == 4
    assert torch.equal(again.optimizer.flat, eng.optimizer.flat)
    _steps(eng, 1, seed=9), _steps(again, 1, seed=9)
    assert torch.equal(again.optimizer.ema_flat, eng.optimizer.ema_flat) and torch.equal(again.optimizer.flat, eng.optimizer.flat)
    # --reset, and a checkpoint without the key: the average starts from the loaded weights
    fresh = TinyEngine(ema=(0.9, False), seed=2)
    assert T.resume_checkpoint(path, fresh, None, CONFIG, reset=True) == 0
    assert torch.equal(fresh.optimizer.ema_flat, fresh.optimizer.flat.detach()) and float(fresh.optimizer.ema_step) == 0
    assert torch.equal(fresh.optimizer.flat.detach(), torch.cat([cpt["model"]["states"][n].reshape(-1) for n in trainable]))
    plain = TinyEngine()
    _steps(plain, 2)
    old = T.save_checkpoint(str(tmp_path / "p" / "checkpoint-iteration1.pth"), plain, None, CONFIG, 1)[0]
    late = TinyEngine(ema=(0.5, False), seed=3)
    _steps(late, 1)
    assert T.resume_checkpoint(old, late, None, CONFIG) == 2
    assert torch.equal(late.optimizer.ema_flat, plain.optimizer.flat.detach()) and float(late.optimizer.ema_step) == 0
    # a run without an average reads a checkpoint that has one as it always did
    T.resume_checkpoint(path, TinyEngine(), None, CONFIG)


def test_features_off_write_the_five_keys(tmp_path):
    T = _trainer()
    eng = TinyEngine()
    _steps(eng, 2)
    assert eng.optimizer.last_grad_norm is None and eng.optimizer.ema_flat is None and not eng.has_ema and eng.ema_state() is None
    cpt = torch.load(T.save_checkpoint(str(tmp_path / "checkpoint-iteration1.pth"), eng, None, CONFIG, 1)[0], weights_only=False)
    assert tuple(cpt) == T.CHECKPOINT_KEYS and len(cpt) == 5
    with pytest.raises(ValueError):
        with eng.ema_weights():
            pass


def test_ema_weights_swaps_contents_and_restores_bit_for_bit():
    eng = TinyEngine(ema=(0.5, False))
    _steps(eng, 3)
    raw, avg = eng.optimizer.flat.detach().clone(), eng.optimizer.ema_flat.clone()
    stats = eng.model[1].running_mean.clone()
    ptrs = [p.data_ptr() for p in eng.model.parameters()]
    assert not torch.equal(raw, avg)
    with eng.ema_weights():
        assert torch.equal(torch.cat([p.detach().reshape(-1) for p in eng.model.parameters()]), avg)      # the model sees the average
        assert torch.equal(eng.optimizer.ema_flat, raw) and torch.equal(eng.model[1].running_mean, stats)
        inside = eng.ema_state()["states"]
        with eng.ema_weights():                                           # nesting changes nothing
            assert torch.equal(eng.optimizer.flat.detach(), avg)
        assert torch.equal(eng.optimizer.flat.detach(), avg)
    assert torch.equal(eng.optimizer.flat.detach(), raw) and torch.equal(eng.optimizer.ema_flat, avg)
    assert [p.data_ptr() for p in eng.model.parameters()] == ptrs and eng.optimizer.views_intact()
    outside = eng.ema_state()["states"]
    assert all(torch.equal(inside[k], outside[k]) for k in outside)       # the key holds the average wherever it is written
    with pytest.raises(RuntimeError):                                     # an exception inside still restores
        with eng.ema_weights():
            raise RuntimeError("x")
    assert torch.equal(eng.optimizer.flat.detach(), raw) and torch.equal(eng.optimizer.ema_flat, avg)


def test_accumulation_window_clips_the_summed_gradient():
    eng = TinyEngine(clip_grad=(1e-3, 2))
    eng.accu_step = 2
    g = torch.Generator().manual_seed(4)
    wires = []
    for micro in range(2):
        eng.train_step(torch.randn(5, 3, generator=g), torch.randn(5, 2, generator=g))
        wires.append(eng.bucket.flat.clone() if micro == 0 else None)
    assert eng.iteration == 1
    total = eng.bucket.flat                                               # the window's sum: what the norm is taken of
    assert not torch.equal(total, wires[0])
    got = eng.optimizer.last_grad_norm.numpy()
    assert got[0] in GR.norm_candidates(GR.total_norm(total.numpy())) and got[1] == GR.clip_coef(got[0], 1e-3)


# ------------------------------------------------------------------ the monitor's second ring
class ListWriter:
    def __init__(self):
        self.scalars = []

    def add_scalar(self, tag, value, step):
        self.scalars.append((tag, float(value), step))

    def flush(self):
        pass

    def close(self):
        pass


@pytest.mark.parametrize("clip", [None, (0.5, 2)], ids=["off", "on"])
def test_monitor_logs_norm_and_coefficient_through_a_second_ring(clip):
    from ebfi_amd import monitor as M
    eng = TinyEngine(clip_grad=clip)
    writer = ListWriter()
    mon = M.TrainMonitor(M.monitor_settings({"trainer": {"tensorboard": True}}), "unused", rank=0, ring=2, writer=writer)
    seen = []
    for it in range(3):
        _steps(eng, 1, seed=it)
        if clip is not None:
            seen.append(eng.optimizer.last_grad_norm.clone())
        mon.after_step(it, torch.tensor(1.0), 1e-4, eng, None)
    mon.close()
    tags = {}
    for tag, value, step in writer.scalars:
        tags.setdefault(tag, []).append((step, value))
    if clip is None:
        assert set(tags) == {"train_loss/train", "learning rate", "steps_per_sec/train"} and mon.last_grad_norm is None
        return
    assert set(tags) == {"train_loss/train", "learning rate", "steps_per_sec/train", "grad_norm/total", "grad_norm/clip_coef"}
    assert tags["grad_norm/total"] == [(it, float(v[0])) for it, v in enumerate(seen)]
    assert tags["grad_norm/clip_coef"] == [(it, float(v[1])) for it, v in enumerate(seen)]
    assert mon.last_grad_norm == (float(seen[-1][0]), float(seen[-1][1]))


# ------------------------------------------------------------------ inference on the averaged weights
def test_infer_loads_the_average_and_refuses_a_checkpoint_without_one(tmp_path):
    from ebfi_amd.engine import DEFAULT_MODEL_ARGS
    from ebfi_amd.model import EVFIAutoEx
    infer = _trainer("infer_ours")
    margs = dict(DEFAULT_MODEL_ARGS, FrameBasech=8, EventBasech=8, InterCH=8, TB=4, step=2, channels=[4, 4, 8, 8])
    torch.manual_seed(0)
    net = EVFIAutoEx(**margs)
    raw = {k: v.clone() for k, v in net.state_dict().items()}
    avg = {n: p.detach() + 0.25 for n, p in net.named_parameters() if p.requires_grad}
    cpt = {"model": {"name": "EVFIAutoEx", "states": raw}, "config": {"model": {"name": "EVFIAutoEx", "args": margs}},
           "ema": {"decay": 0.9, "warmup": False, "step": 3, "states": avg}}
    torch.save(cpt, str(tmp_path / "with.pth"))
    torch.save({k: v for k, v in cpt.items() if k != "ema"}, str(tmp_path / "without.pth"))
    assert infer.get_flags(["--ema"]).ema is True and infer.get_flags([]).ema is False
    model, _ = infer.load_model(str(tmp_path / "with.pth"), "cpu", ema=True)
    got = dict(model.named_parameters())
    assert all(torch.equal(got[n], avg[n]) for n in avg) and not model.training
    model, _ = infer.load_model(str(tmp_path / "with.pth"), "cpu")                # without the flag: the raw iterate, as always
    assert all(torch.equal(v, raw[k]) for k, v in model.state_dict().items())
    with pytest.raises(SystemExit, match="holds no averaged weights"):
        infer.load_model(str(tmp_path / "without.pth"), "cpu", ema=True)
    with pytest.raises(SystemExit, match="needs a checkpoint"):
        infer.load_model(None, "cpu", ema=True)


def test_an_inference_engine_refuses_both():
    from ebfi_amd.engine import Engine
    small = dict(FrameBasech=8, EventBasech=8, InterCH=8, TB=4, step=2, channels=[4, 4, 8, 8])
    for kw in ({"ema": (0.9, False)}, {"clip_grad": (1.0, 2)}):
        with pytest.raises(ValueError, match="train=True"):
            Engine(small, device="cpu", train=False, **kw)
    assert not Engine(small, device="cpu", train=False).has_ema
