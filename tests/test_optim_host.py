"""The optimizer section of the config on the host (no kernels run): ebfi_amd.dp.FlatOptimizer against torch.optim.Adam / AdamW /
SGD on the same gradients -- what the reference trainer itself builds from the section (train_ours.py:770-771) -- checkpoint
interchange in torch's per-parameter layout in both directions, `optimizer_settings` of both trainers, and FlatAdam as the
thin subclass it has become."""
import copy
import importlib.util
import os

import pytest
import torch
import yaml

from ebfi_amd.dp import FlatAdam, FlatGradBucket, FlatOptimizer
from ebfi_amd.engine import Engine

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


def _net():
    torch.manual_seed(3)
    return torch.nn.Sequential(torch.nn.Conv2d(3, 4, 3), torch.nn.Conv2d(4, 2, 1))


def _step_both(net_a, opt_a, net_b, opt_b, bucket, x):
    """One step on identical gradients: torch on the per-parameter original, ours on the flat copy."""
    opt_a.zero_grad()
    net_a(x).square().sum().backward()
    opt_a.step()
    bucket.zero()
    net_b(x).square().sum().backward()
    opt_b.step(bucket.gather())


def _assert_same(net_a, net_b):
    for pa, pb in zip(net_a.parameters(), net_b.parameters()):
        assert torch.allclose(pa, pb, rtol=1e-6, atol=1e-7)


def _key_sets(sd):
    return ({pid: set(e) for pid, e in sd["state"].items()}, set(sd["param_groups"][0]))


@pytest.mark.parametrize("name,args", CONFIGS, ids=IDS)
def test_flat_optimizer_matches_torch_and_speaks_its_checkpoint_layout(name, args):
    cls = getattr(torch.optim, name)
    net_a = _net()
    net_b = copy.deepcopy(net_a)
    opt_a = cls(net_a.parameters(), lr=1e-2, **args)
    opt_b = FlatOptimizer(list(net_b.parameters()), name, lr=1e-2, **args)
    assert opt_b.views_intact() and isinstance(opt_b.inner, cls)
    bucket = FlatGradBucket(net_b)
    x = torch.randn(2, 3, 8, 8)
    if name == "SGD":                                           # nothing before the first applied step
        assert opt_b.state_dict()["state"] == {} == opt_a.state_dict()["state"]
    for _ in range(3):
        _step_both(net_a, opt_a, net_b, opt_b, bucket, x)
    _assert_same(net_a, net_b)
    # the exported key sets are exactly torch's: per-parameter entries and the param_group
    sd_a, sd_b = opt_a.state_dict(), opt_b.state_dict()
    assert _key_sets(sd_a) == _key_sets(sd_b)
    want = {"Adam": {"step", "exp_avg", "exp_avg_sq"}, "AdamW": {"step", "exp_avg", "exp_avg_sq"}, "SGD": {"momentum_buffer"}}[name]
    if args.get("amsgrad"):
        want = want | {"max_exp_avg_sq"}
    if name == "SGD" and not args.get("momentum"):
        assert sd_b["state"] == {}
    else:
        assert len(sd_b["state"]) == 4 and all(set(e) == want for e in sd_b["state"].values())
        key = sorted(want - {"step"})[0]
        assert sd_b["state"][0][key].shape == (4, 3, 3, 3)
    # ours -> a fresh torch optimiser, torch's -> a fresh FlatOptimizer (built with another lr: the checkpoint's wins)
    net_c, net_d = copy.deepcopy(net_b), copy.deepcopy(net_a)
    opt_c = cls(net_c.parameters(), lr=1e-2, **args)
    opt_c.load_state_dict(sd_b)
    opt_d = FlatOptimizer(list(net_d.parameters()), name, lr=5e-1, **args)
    opt_d.load_state_dict(copy.deepcopy(sd_a))
    assert opt_d.param_groups[0]["lr"] == 1e-2
    bucket_d = FlatGradBucket(net_d)
    opt_a.zero_grad()
    net_a(x).square().sum().backward()
    opt_a.step()
    opt_c.zero_grad()
    net_c(x).square().sum().backward()
    opt_c.step()
    net_d(x).square().sum().backward()
    opt_d.step(bucket_d.gather())
    _assert_same(net_a, net_c)
    _assert_same(net_a, net_d)


def test_adam_checkpoint_loads_into_an_amsgrad_run_with_a_zero_maximum():
    net = _net()
    ref = torch.optim.Adam(net.parameters(), lr=1e-2)
    net(torch.randn(1, 3, 8, 8)).square().sum().backward()
    ref.step()
    sd = copy.deepcopy(ref.state_dict())
    del sd["param_groups"][0]["amsgrad"]                        # (so that the run's own amsgrad=True stays)
    opt = FlatOptimizer(list(copy.deepcopy(net).parameters()), "Adam", lr=1e-2, amsgrad=True)
    opt.load_state_dict(sd)
    st = opt.inner.state[opt.flat]
    assert float(st["step"]) == 1 and st["max_exp_avg_sq"].abs().sum() == 0 and st["exp_avg_sq"].abs().sum() > 0
    opt.step(torch.randn(opt.flat.numel()))
    assert torch.isfinite(opt.flat).all() and set(opt.state_dict()["state"][0]) == {"step", "exp_avg", "exp_avg_sq", "max_exp_avg_sq"}


def test_unsupported_optimizers_and_options_are_refused():
    params = lambda: list(_net().parameters())
    with pytest.raises(ValueError, match="Adam, AdamW, SGD"):
        FlatOptimizer(params(), "RMSprop", lr=1e-3)
    for bad in ({"maximize": True}, {"differentiable": True}, {"lr": torch.tensor(1e-3)}):
        with pytest.raises(ValueError):
            FlatOptimizer(params(), "Adam", **bad)
    with pytest.raises(ValueError):
        FlatOptimizer(params(), "SGD", lr=1e-2, nesterov=True)              # torch's own constructor check
    with pytest.raises(ValueError):
        FlatOptimizer(params(), "SGD", lr=1e-2, no_such_argument=1)
    assert FlatOptimizer(params(), "AdamW").param_groups[0]["weight_decay"] == 1e-2      # torch's default for AdamW
    # run-mode flags stay this process's decision
    opt = FlatOptimizer(params(), "Adam", lr=1e-3, fused=None, foreach=True, capturable=True)
    assert opt.param_groups[0]["fused"] is False and opt.param_groups[0]["foreach"] is None and opt.param_groups[0]["capturable"] is False
    # an option switched on later through param_groups is refused at the step, not ignored
    opt.param_groups[0]["maximize"] = True
    with pytest.raises(ValueError):
        opt.step(torch.zeros(opt.flat.numel()))


def _module(filename):
    spec = importlib.util.spec_from_file_location("ebfi_" + filename[:-3], os.path.join(PKG, filename))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod


@pytest.mark.parametrize("filename,config", [("train_ours.py", "train_ours.yml"),
                                             ("train_ours_exposuredecision.py", "train_ours_exposuredecision.yml")])
def test_optimizer_settings_of_both_trainers(filename, config):
    T = _module(filename)
    cfg = yaml.safe_load(open(os.path.join(PKG, "config", config)))
    args = type("Args", (), {"learning_rate": None})()
    # the shipped section: today's Adam
    plain = T.optimizer_settings(cfg, args)
    assert plain == {"name": "Adam", "args": {"lr": 1e-4, "betas": (0.9, 0.999), "amsgrad": False}}
    eng = Engine(SMALL, device="cpu", seed=1, optimizer=plain)
    base = Engine(SMALL, device="cpu", seed=1, lr=1e-4)
    ga, gb = eng.optimizer.param_groups[0], base.optimizer.param_groups[0]
    assert isinstance(eng.optimizer.inner, torch.optim.Adam) and {k: v for k, v in ga.items() if k != "params"} == \
        {k: v for k, v in gb.items() if k != "params"}
    assert ga["weight_decay"] == 0 and ga["amsgrad"] is False and ga["eps"] == 1e-8 and not ga.get("decoupled_weight_decay")
    # every argument of the section reaches the optimiser
    cfg["optimizer"] = {"name": "AdamW", "args": {"lr": 2e-4, "weight_decay": 1e-4, "eps": 1e-6, "amsgrad": True, "betas": [0.8, 0.99]}}
    got = T.optimizer_settings(cfg, args)
    g = Engine(SMALL, device="cpu", seed=1, optimizer=got).optimizer.param_groups[0]
    assert got["name"] == "AdamW" and (g["lr"], g["weight_decay"], g["eps"], g["amsgrad"], g["betas"]) == (2e-4, 1e-4, 1e-6, True, (0.8, 0.99))
    assert g["decoupled_weight_decay"] is True
    # -lr of the stage-1 trainer overrides optimizer.args.lr
    args.learning_rate = 3e-5
    assert T.optimizer_settings(cfg, args)["args"]["lr"] == 3e-5
    args.learning_rate = None
    cfg["optimizer"] = {"name": "SGD", "args": {"lr": 1e-2, "momentum": 0.9}}
    assert T.optimizer_settings(cfg, args) == {"name": "SGD", "args": {"lr": 1e-2, "momentum": 0.9}}
    # refused loudly
    cfg["optimizer"] = {"name": "RMSprop", "args": {"lr": 1e-4}}
    with pytest.raises(ValueError, match="Adam, AdamW, SGD"):
        T.optimizer_settings(cfg, args)
    cfg["optimizer"] = {"name": "Adam", "args": {"lr": 1e-4, "maximize": True}}
    with pytest.raises(ValueError, match="maximize"):
        T.optimizer_settings(cfg, args)


def test_checkpoint_names_the_configured_optimizer_and_resumes_only_on_a_match(tmp_path):
    T = _module("train_ours.py")
    cfg = yaml.safe_load(open(os.path.join(PKG, "config", "train_ours.yml")))
    cfg["model"]["args"].update(SMALL)
    cfg["optimizer"] = {"name": "AdamW", "args": {"lr": 1e-3, "weight_decay": 0.1, "amsgrad": True}}
    eng = Engine(cfg["model"]["args"], device="cpu", seed=1, optimizer=T.optimizer_settings(cfg))
    g = torch.Generator().manual_seed(0)
    for _ in range(2):
        eng.optimizer.step(torch.randn(eng.optimizer.flat.numel(), generator=g))
    path = str(tmp_path / "checkpoint-iteration1.pth")
    T.save_checkpoint(path, eng, None, cfg, 1)
    cpt = torch.load(path, map_location="cpu", weights_only=False)
    assert cpt["optimizer"]["name"] == "AdamW" and "max_exp_avg_sq" in cpt["optimizer"]["states"]["state"][0]
    probe = torch.optim.AdamW([torch.nn.Parameter(p.detach().clone()) for p in eng.optimizer.params], amsgrad=True)
    probe.load_state_dict(cpt["optimizer"]["states"])
    eng2 = Engine(cfg["model"]["args"], device="cpu", seed=2, optimizer=T.optimizer_settings(cfg))
    assert T.resume_checkpoint(path, eng2, None, cfg) == 2
    sa, sb = eng.optimizer.inner.state[eng.optimizer.flat], eng2.optimizer.inner.state[eng2.optimizer.flat]
    assert torch.equal(sa["max_exp_avg_sq"], sb["max_exp_avg_sq"]) and float(sb["step"]) == 2
    cfg3 = copy.deepcopy(cfg)
    cfg3["optimizer"] = {"name": "SGD", "args": {"lr": 1e-3, "momentum": 0.9}}      # another name: the states stay out
    eng3 = Engine(cfg["model"]["args"], device="cpu", seed=3, optimizer=T.optimizer_settings(cfg3))
    assert T.resume_checkpoint(path, eng3, None, cfg3) == 2 and not eng3.optimizer.inner.state


def test_flat_adam_is_a_thin_subclass_with_its_old_signature():
    net_a = _net()
    net_b = copy.deepcopy(net_a)
    opt_a = torch.optim.Adam(net_a.parameters(), lr=3e-3, betas=(0.8, 0.99), eps=1e-7)
    opt_b = FlatAdam(list(net_b.parameters()), lr=3e-3, betas=(0.8, 0.99), eps=1e-7)
    assert isinstance(opt_b, FlatOptimizer) and type(opt_b.inner) is torch.optim.Adam
    g = opt_b.param_groups[0]
    assert (g["lr"], g["betas"], g["eps"], g["weight_decay"], g["amsgrad"], g["fused"]) == (3e-3, (0.8, 0.99), 1e-7, 0, False, False)
    assert FlatAdam(list(_net().parameters())).param_groups[0]["lr"] == 1e-4
    bucket = FlatGradBucket(net_b)
    x = torch.randn(2, 3, 8, 8)
    for _ in range(2):
        _step_both(net_a, opt_a, net_b, opt_b, bucket, x)
    _assert_same(net_a, net_b)
    guard = torch.zeros(2, dtype=torch.int32)
    before = opt_b.flat.detach().clone()
    opt_b.step(bucket.flat, guard=guard, flag=torch.ones(1))                 # the host-side guard in front of torch's own step
    assert guard.tolist() == [1, 1] and torch.equal(before, opt_b.flat.detach())
    assert float(opt_b.inner.state[opt_b.flat]["step"]) == 2
