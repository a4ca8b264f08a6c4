"""ebfi_optim_step (csrc/optim.hip) and ebfi_amd.dp.FlatOptimizer on the device: Adam / AdamW with weight decay and AMSGrad,
SGD with weight decay, momentum, dampening and Nesterov, each as one launch over a flat buffer -- against the same torch.optim
class on the CPU (what the reference trainer builds from its `optimizer` section, train_ours.py:770-771).

Accuracy bound: e = max_i |x_i - x64_i| / max(|x64_i|, lr) against the class run in float64, for the parameters and for every
state buffer; the yardstick e32 is the same figure for torch's own float32 CPU run; pass when e <= 4 e32.  The kernels round
operation by operation as torch's float32 CPU kernels do, so on most buffers e == e32 (profiles/optim.md holds the ratios)."""
import os
import subprocess
import sys

import pytest
import torch
import yaml

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
PKG = os.path.join(ROOT, "ebfi-be_amd")
SMALL = dict(FrameBasech=8, EventBasech=8, InterCH=8, TB=4, step=2, channels=[4, 4, 8, 8])

CONFIGS = [
    ("Adam", {}),
    ("Adam", {"weight_decay": 1e-2, "amsgrad": True, "eps": 1e-6}),
    ("AdamW", {"weight_decay": 1e-1}),
    ("AdamW", {"amsgrad": True}),
    ("SGD", {}),
    ("SGD", {"momentum": 0.9, "dampening": 0.1, "weight_decay": 1e-3}),
    ("SGD", {"momentum": 0.9, "nesterov": True}),
]
IDS = ["adam", "adam_l2_ams_eps", "adamw_wd", "adamw_ams", "sgd", "sgd_mom_damp_wd", "sgd_nesterov"]
SIZES = (1, 3, 4, 7, 1027, 2053)       # tail only | tail only | one vector | vector + tail | > 1 workgroup of float4 | > 2 workgroups
LR, STEPS, FACTOR = 1e-2, 5, 4.0
STATE_KEYS = ("exp_avg", "exp_avg_sq", "max_exp_avg_sq", "momentum_buffer")


def _data(n, steps, seed):
    """Parameters N(0,1) exp(U(-6,1)); gradients N(0,1) exp(U(-12,2)) with every fifth element (from index 2) zero on every step."""
    g = torch.Generator().manual_seed(seed)
    p = torch.randn(n, generator=g) * torch.exp(torch.rand(n, generator=g) * 7 - 6)
    grads = []
    for _ in range(steps):
        x = torch.randn(n, generator=g) * torch.exp(torch.rand(n, generator=g) * 14 - 12)
        x[2::5] = 0.0
        grads.append(x)
    return p, grads


def _torch_run(name, args, p0, grads, dtype, lrs):
    """The class itself on the CPU in `dtype` -> (parameters, {state key: buffer})."""
    p = torch.nn.Parameter(p0.to(dtype).clone())
    opt = getattr(torch.optim, name)([p], lr=lrs[0], **args)
    for g, lr in zip(grads, lrs):
        opt.param_groups[0]["lr"] = lr
        p.grad = g.to(dtype)
        opt.step()
    return p.detach(), {k: v for k, v in opt.state[p].items() if k in STATE_KEYS and v is not None}


def _err(x, x64, lr):
    if x.numel() == 0:
        return 0.0
    return float(((x.double().cpu() - x64).abs() / x64.abs().clamp_min(lr)).max())


def _schedule(steps=STEPS):
    return [LR if s < 2 else LR / 2 for s in range(steps)]         # halved before step 3, as a scheduler would


def _flat_optimizer(name, args, p0, lr=LR):
    from ebfi_amd.dp import FlatOptimizer
    opt = FlatOptimizer([torch.nn.Parameter(p0.clone().cuda())], name, lr=lr, **args)
    assert opt.flat.data_ptr() % 16 == 0
    return opt


def _buffers(opt):
    """Every device buffer a step may write: parameters, states, the step words."""
    st = opt.inner.state.get(opt.flat, {})
    out = {"param": opt.flat.data}
    out.update((k, v) for k, v in st.items() if torch.is_tensor(v))
    if opt._sgd_step is not None:
        out["sgd_step"] = opt._sgd_step
    return out


@pytest.mark.parametrize("name,args", CONFIGS, ids=IDS)
def test_every_variant_within_four_times_torch_float32_error(name, args):
    lrs = _schedule()
    worst = {}
    for n in SIZES:
        p0, grads = _data(n, STEPS, seed=1000 + n)
        opt = _flat_optimizer(name, args, p0)
        for g, lr in zip(grads, lrs):
            opt.param_groups[0]["lr"] = lr
            opt.step(g.cuda())
        got = {"param": opt.flat.detach()}
        got.update((k, v) for k, v in opt.inner.state.get(opt.flat, {}).items() if k in STATE_KEYS)
        p64, s64 = _torch_run(name, args, p0, grads, torch.float64, lrs)
        p32, s32 = _torch_run(name, args, p0, grads, torch.float32, lrs)
        ref64, ref32 = dict(s64, param=p64), dict(s32, param=p32)
        assert set(got) == set(ref64) == set(ref32), (n, sorted(got), sorted(ref64))
        if name != "SGD":
            assert float(opt.inner.state[opt.flat]["step"]) == STEPS
        for key in sorted(got):
            e, e32 = _err(got[key], ref64[key], lrs[-1]), _err(ref32[key], ref64[key], lrs[-1])
            print("optim-accuracy %-16s n=%-5d %-16s e=%.3e e32=%.3e ratio=%s"       # (shown with pytest -s)
                  % (IDS[CONFIGS.index((name, args))], n, key, e, e32, "%.2f" % (e / e32) if e32 > 0 else ("1.00" if e == 0 else "inf")))
            if not e <= FACTOR * e32:
                worst[(n, key)] = (e, e32)
    assert not worst, worst


def test_plain_adam_is_the_launch_it_has_always_been():
    """Adam without weight decay and AMSGrad through ebfi_optim_step and through ebfi_adam_step_guarded, same start: same bits."""
    from ebfi_amd import _native as N
    n = 2053
    p0, grads = _data(n, 3, seed=5)
    dev = torch.device("cuda")
    runs = []
    for new in (False, True):
        p, m, v = p0.clone().to(dev), torch.zeros(n, device=dev), torch.zeros(n, device=dev)
        step, guard = torch.zeros((), device=dev), torch.zeros(2, dtype=torch.int32, device=dev)
        for g in grads:
            g = g.to(dev)
            step += 1
            if new:
                rc = N.lib().ebfi_optim_step(0, 0, N.ptr(p), N.ptr(g), N.ptr(m), N.ptr(v), N.ptr(None), N.ptr(step), n, 1e-3, 0.9,
                                             0.999, 1e-8, 0.0, 0.0, 0.0, N.ptr(guard), N.ptr(None), N.stream_ptr(dev))
            else:
                rc = N.lib().ebfi_adam_step_guarded(N.ptr(p), N.ptr(g), N.ptr(m), N.ptr(v), N.ptr(step), n, 1e-3, 0.9, 0.999, 1e-8,
                                                    N.ptr(guard), N.ptr(None), N.stream_ptr(dev))
            N.check(rc, "adam step")
        torch.cuda.synchronize()
        runs.append((p, m, v, step))
    assert all(torch.equal(a, b) for a, b in zip(*runs)) and float(runs[0][3]) == 3 and not torch.equal(runs[0][0], p0.to(dev))


def test_entry_point_refuses_what_it_does_not_implement():
    from ebfi_amd import _native as N
    dev = torch.device("cuda")
    p, g, b, step = (torch.zeros(8, device=dev) for _ in range(4))
    call = lambda kind, flags, mom=0.0, damp=0.0, wd=0.0, buf=b: N.lib().ebfi_optim_step(
        kind, flags, N.ptr(p), N.ptr(g), N.ptr(buf), N.ptr(b), N.ptr(None), N.ptr(step), 8, 1e-3, 0.9, 0.999, 1e-8, wd, mom, damp,
        N.ptr(None), N.ptr(None), N.stream_ptr(dev))
    assert call(2, 0) == -3                                    # unknown kind: EBFI_ERR_UNSUPPORTED
    assert call(0, 4) == -1 and call(1, 2) == -1 and call(0, 8) == -1       # a flag of the other family, an unknown flag
    assert call(1, 4) == -1 and call(1, 4, mom=0.9, damp=0.1) == -1         # Nesterov needs momentum and zero dampening
    assert call(0, 2) == -1                                    # AMSGrad without max_exp_avg_sq
    assert call(1, 0, mom=0.9, buf=None) == -1 and call(1, 0, wd=-1.0) == -1
    assert call(1, 0) == 0 and call(1, 4, mom=0.9) == 0
    torch.cuda.synchronize()


GUARDED = [("AdamW", {"weight_decay": 0.1, "amsgrad": True}), ("SGD", {"momentum": 0.9, "dampening": 0.1, "weight_decay": 1e-3})]


@pytest.mark.parametrize("name,args", GUARDED, ids=["adamw_ams", "sgd_mom_damp_wd"])
def test_a_skipped_step_writes_nothing_and_takes_the_step_word_back(name, args):
    n = 1027
    p0, grads = _data(n, 2, seed=11)
    opt = _flat_optimizer(name, args, p0)
    opt.step(grads[0].cuda())                                   # (a real step first: every state buffer holds something)
    before = {k: v.clone() for k, v in _buffers(opt).items()}
    assert {"param", "sgd_step", "momentum_buffer"} <= set(before) if name == "SGD" else {"param", "step", "max_exp_avg_sq"} <= set(before)
    g = grads[1].cuda()
    skipped = 0
    for word, flag in ((1, None), (0, 1.0), (0, float("nan"))):
        guard = torch.tensor([word, skipped], dtype=torch.int32, device="cuda")
        opt.step(g, guard=guard, flag=None if flag is None else torch.tensor([flag], device="cuda"))
        skipped += 1
        assert guard.tolist() == [1, skipped], (word, flag, guard.tolist())
        after = _buffers(opt)
        assert set(after) == set(before)
        for k in before:
            assert torch.equal(after[k].view(torch.int32) if after[k].is_floating_point() else after[k],
                               before[k].view(torch.int32) if before[k].is_floating_point() else before[k]), (k, word, flag)
    guard = torch.zeros(2, dtype=torch.int32, device="cuda")
    opt.step(g, guard=guard, flag=torch.zeros(1, device="cuda"))                  # and a clean step still updates
    assert guard.tolist() == [0, 0] and not torch.equal(opt.flat.data, before["param"])
    assert float(_buffers(opt)["sgd_step" if name == "SGD" else "step"]) == 2


def test_sgd_first_step_skipped_by_the_guard_leaves_the_next_one_the_first():
    """dampening = 0.1: torch's first step sets buf = d, every later one buf = momentum buf + 0.9 d.  The decision is the
    device's: the host never learns of the skip."""
    name, args = GUARDED[1]
    n = 1027
    p0, grads = _data(n, 1, seed=12)
    opt = _flat_optimizer(name, args, p0)
    guard = torch.tensor([1, 0], dtype=torch.int32, device="cuda")
    opt.step(grads[0].cuda(), guard=guard, flag=torch.zeros(1, device="cuda"))
    assert guard.tolist() == [1, 1] and torch.equal(opt.flat.data.cpu(), p0) and opt.state_dict()["state"] == {}
    guard.zero_()
    opt.step(grads[0].cuda(), guard=guard, flag=torch.zeros(1, device="cuda"))
    p32, s32 = _torch_run(name, args, p0, grads, torch.float32, [LR])
    buf = opt.inner.state[opt.flat]["momentum_buffer"].cpu()
    d = grads[0] + 1e-3 * p0
    assert torch.allclose(buf, d, rtol=1e-6, atol=0) and not torch.allclose(buf, 0.9 * d, rtol=1e-2, atol=0)
    assert torch.allclose(buf, s32["momentum_buffer"], rtol=1e-6, atol=0) and torch.allclose(opt.flat.data.cpu(), p32, rtol=1e-6, atol=1e-9)
    assert set(opt.state_dict()["state"][0]) == {"momentum_buffer"}               # the private step word is not exported


@pytest.mark.parametrize("name,args", [("Adam", {"weight_decay": 1e-2}), ("AdamW", {"weight_decay": 1e-1}),
                                       ("SGD", {"weight_decay": 1e-3, "momentum": 0.9})], ids=["adam_l2", "adamw", "sgd_l2"])
def test_weight_decay_never_writes_the_gradient_buffer(name, args):
    n = 1027
    p0, grads = _data(n, 2, seed=13)
    opt = _flat_optimizer(name, args, p0)
    for g in grads:
        g = g.cuda()
        keep = g.clone()
        opt.step(g)
        assert torch.equal(g.view(torch.int32), keep.view(torch.int32))
    assert not torch.equal(opt.flat.data.cpu(), p0)


def _engine_run(graph, optimizer=None, **kw):
    """Three train_steps, lr changed through param_groups before the third -> (start, packed gradients, lrs, final flat)."""
    from ebfi_amd.engine import Engine, synthetic_batch
    eng = Engine(SMALL, device="cuda", precision="fp32", seed=3, graph=graph, optimizer=optimizer, **kw)
    start = eng.optimizer.flat.detach().clone().cpu()
    grads, lrs = [], []
    for it in range(3):
        if it == 2:
            eng.optimizer.param_groups[0]["lr"] *= 0.5
        lrs.append(eng.optimizer.param_groups[0]["lr"])
        eng.train_step(*synthetic_batch(2, 64, 64, TB=4, device="cuda", seed=50 + it))
        grads.append(eng.bucket.flat.detach().clone().cpu())
    assert eng.optimizer.views_intact() and eng.bucket.views_intact()
    return eng, start, grads, lrs, eng.optimizer.flat.detach().clone().cpu()


@pytest.mark.parametrize("graph", [False, True], ids=["eager", "graph"])
def test_engine_trains_with_the_configured_optimizer(graph):
    name, args = "AdamW", {"lr": 1e-3, "weight_decay": 0.1, "amsgrad": True}
    eng, start, grads, lrs, final = _engine_run(graph, {"name": name, "args": args})
    assert isinstance(eng.optimizer.inner, torch.optim.AdamW) and lrs == [1e-3, 1e-3, 5e-4]
    assert graph == (len(eng._graphs) == 1)
    st = eng.optimizer.inner.state[eng.optimizer.flat]
    assert float(st["step"]) == 3 and st["max_exp_avg_sq"].abs().sum() > 0
    extra = {k: v for k, v in args.items() if k != "lr"}
    p64, _ = _torch_run(name, extra, start, grads, torch.float64, lrs)
    p32, _ = _torch_run(name, extra, start, grads, torch.float32, lrs)
    e, e32 = _err(final, p64, lrs[-1]), _err(p32, p64, lrs[-1])
    print("optim-engine %s e=%.3e e32=%.3e ratio=%.2f" % ("graph" if graph else "eager", e, e32, e / e32))
    assert e <= FACTOR * e32, (e, e32)


def test_engine_named_adam_is_the_engine_given_only_lr():
    a = _engine_run(False, {"name": "Adam", "args": {"lr": 1e-3}})[4]
    b = _engine_run(False, None, lr=1e-3)[4]
    assert torch.equal(a, b)


def test_exposure_engine_takes_sgd_under_accumulation_and_graph_replay():
    """Stage 1 with SGD (momentum, dampening, weight decay), accu_step 2, replayed from a graph, the weight bank reading the
    optimiser's flat buffer: three optimiser steps equal torch.optim.SGD replayed over the accumulated packed gradients."""
    from ebfi_amd.exposure_engine import ExposureEngine, synthetic_exposure_batch
    name, args = "SGD", {"lr": 1e-2, "momentum": 0.9, "dampening": 0.1, "weight_decay": 1e-3}
    eng = ExposureEngine(fashion="RGBDark", device="cuda", precision="bf16x3", seed=4, graph=True, accu_step=2,
                         optimizer={"name": name, "args": args})
    assert isinstance(eng.optimizer.inner, torch.optim.SGD) and eng.bank is not None
    start = eng.optimizer.flat.detach().clone().cpu()
    grads = []
    for micro in range(6):
        eng.train_step(*synthetic_exposure_batch(2, 32, 32, TB=16, device="cuda", seed=60 + micro))
        if micro % 2 == 1:
            grads.append(eng.bucket.flat.detach().clone().cpu())
    assert eng.iteration == 3 and len(eng._graphs) == 1 and eng.optimizer.views_intact()
    assert all(g.abs().sum() > 0 for g in grads)
    final = eng.optimizer.flat.detach().clone().cpu()
    extra = {k: v for k, v in args.items() if k != "lr"}
    p64, s64 = _torch_run(name, extra, start, grads, torch.float64, [1e-2] * 3)
    p32, s32 = _torch_run(name, extra, start, grads, torch.float32, [1e-2] * 3)
    buf = eng.optimizer.inner.state[eng.optimizer.flat]["momentum_buffer"]
    for key, got, r64, r32 in (("param", final, p64, p32), ("momentum_buffer", buf, s64["momentum_buffer"], s32["momentum_buffer"])):
        e, e32 = _err(got, r64, 1e-2), _err(r32, r64, 1e-2)
        print("optim-exposure sgd %-16s e=%.3e e32=%.3e" % (key, e, e32))
        assert e <= FACTOR * e32, (key, e, e32)
    sd = eng.optimizer.state_dict()
    assert len(sd["state"]) == len(eng.optimizer.params) and all(set(e) == {"momentum_buffer"} for e in sd["state"].values())


def test_train_ours_with_adamw_amsgrad_checkpoints_resumes_and_refuses_rmsprop(tmp_path):
    cfg = yaml.safe_load(open(os.path.join(PKG, "config", "train_ours.yml")))
    cfg["model"]["args"].update(SMALL)
    cfg["trainer"].update(batch_size=2, height=64, width=64, output_path=str(tmp_path / "out"))
    cfg["trainer"]["iteration_based_train"].update(iterations=3, save_period=0)
    cfg["optimizer"] = {"name": "AdamW", "args": {"lr": 1e-4, "weight_decay": 0.05, "amsgrad": True}}
    cfg_path = tmp_path / "cfg.yml"
    cfg_path.write_text(yaml.safe_dump(cfg))
    env = dict(os.environ, PYTHONPATH=PKG)
    train = [sys.executable, os.path.join(PKG, "train_ours.py")]
    r = subprocess.run(train + ["-c", str(cfg_path), "-id", "w"], capture_output=True, text=True, env=env, timeout=600)
    assert r.returncode == 0, r.stderr[-2000:]
    ckpt = tmp_path / "out" / "models" / "Ours" / "w" / "checkpoint-iteration2.pth"
    cpt = torch.load(str(ckpt), map_location="cpu", weights_only=False)
    states = cpt["optimizer"]["states"]
    assert cpt["optimizer"]["name"] == "AdamW" and states["param_groups"][0]["weight_decay"] == 0.05
    assert states["param_groups"][0]["amsgrad"] is True and states["param_groups"][0]["decoupled_weight_decay"] is True
    assert states["state"] and all(set(e) == {"step", "exp_avg", "exp_avg_sq", "max_exp_avg_sq"} and float(e["step"]) == 3
                                   for e in states["state"].values())
    from ebfi_amd.engine import DEFAULT_MODEL_ARGS
    from ebfi_amd.model import EVFIAutoEx
    model = EVFIAutoEx(**dict(DEFAULT_MODEL_ARGS, **SMALL))
    torch.optim.AdamW(model.parameters(), amsgrad=True).load_state_dict(states)
    r = subprocess.run(train + ["-c", str(cfg_path), "-id", "w2", "--resume", str(ckpt), "--iterations", "4"], capture_output=True,
                       text=True, env=env, timeout=600)
    assert r.returncode == 0 and "Iteration: 3/4" in r.stdout and "Iteration: 2/4" not in r.stdout, r.stderr[-2000:] + r.stdout[-500:]
    cpt2 = torch.load(str(tmp_path / "out" / "models" / "Ours" / "w2" / "checkpoint-iteration3.pth"), map_location="cpu", weights_only=False)
    assert float(cpt2["optimizer"]["states"]["state"][0]["step"]) == 4
    cfg["optimizer"]["name"] = "RMSprop"
    cfg_path.write_text(yaml.safe_dump(cfg))
    r = subprocess.run(train + ["-c", str(cfg_path), "-id", "x"], capture_output=True, text=True, env=env, timeout=600)
    assert r.returncode != 0 and "Adam, AdamW, SGD" in r.stderr and not (tmp_path / "out" / "models" / "Ours" / "x").exists()
