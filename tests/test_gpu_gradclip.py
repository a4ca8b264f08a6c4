"""ebfi_grad_norm (csrc/gradnorm.hip), ebfi_optim_step_ex (csrc/optim.hip) and what the engines and trainers build on them
(FlatOptimizer(clip=, ema=), Engine.ema_weights, the `ema` key of the checkpoints, infer_ours.py --ema) on the device, against
the numpy restatement tests/gradclip_ref.py.

Norm bound: float64 accumulation of <= 6e6 terms errs by <= 6e6 * 2^-53 ~ 7e-10 relative, far below the float32 spacing of 6e-8,
so out[0] is float32(sqrt(float64 sum)) or, where that value straddles a rounding boundary, one of its two float32 neighbours;
the max norm and the coefficient (from the kernel's own out[0]) are bit-exact.  Update: a scale s < 1 gives the bits
ebfi_optim_step gives on a gradient pre-multiplied by s in float32; plain Adam with a scale runs the spelled-out law instead of
the kernel of ebfi_adam_step, and is held to the yardstick of tests/test_gpu_optim.py (four times the error of torch's own
float32 run against float64).  The moving average is bit-exact against the restatement, given the kernel's own parameters."""
import os
import subprocess
import sys

import numpy as np
import pytest
import torch
import yaml

import gradclip_ref as GR

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
PKG = os.path.join(ROOT, "ebfi-be_amd")
SMALL = dict(FrameBasech=8, EventBasech=8, InterCH=8, TB=4, step=2, channels=[4, 4, 8, 8])
INF = float("inf")
CHUNK = 16384
SIZES = (1, 3, 255, 256, 257, CHUNK, CHUNK + 1, 3 * CHUNK + 5)
DEV = "cuda"


def _bits(t):
    return t.detach().cpu().contiguous().view(torch.int32)


def _same_bits(a, b):
    return torch.equal(_bits(a), _bits(b))


# ------------------------------------------------------------------------------------------------ the norm kernel
def _norm(g, norm_type, max_norm=1.0):
    """One call of the entry point on a device tensor -> (norm, coefficient) as numpy float32 scalars."""
    from ebfi_amd import _native as N
    n = g.numel()
    need = N.lib().ebfi_grad_norm_workspace(n)
    assert need == 8 * ((n + CHUNK - 1) // CHUNK)
    ws = torch.full((max(1, need // 8),), float("nan"), dtype=torch.float64, device=g.device)      # (no partial may survive unwritten)
    out = torch.full((2,), -7.0, dtype=torch.float32, device=g.device)
    rc = N.lib().ebfi_grad_norm(N.ptr(g), n, 1 if norm_type == INF else 0, float(max_norm), N.ptr(out), N.ptr(ws), need,
                                N.stream_ptr(g.device))
    N.check(rc, "ebfi_grad_norm")
    got = out.cpu().numpy()
    return got[0], got[1]


def _values(kind, n):
    if kind == "gauss":
        return torch.randn(n, generator=torch.Generator().manual_seed(100 + n))
    return torch.full((n,), 3e25 if kind == "huge" else 1e-30)


@pytest.mark.parametrize("kind", ["gauss", "huge", "tiny"])
def test_norms_match_the_float64_restatement(kind):
    """huge: every square overflows float32 (9e50), the sum stays finite in float64; tiny: every square (1e-60) is below the
    smallest float32 subnormal."""
    for n in SIZES:
        host = _values(kind, n)
        g = host.to(DEV)
        for norm_type, max_norm in ((2, 0.25), (INF, 0.25), (2, 1e30)):
            norm, coef = _norm(g, norm_type, max_norm)
            norm64 = GR.total_norm(host.numpy(), norm_type)
            print("grad-norm %-5s n=%-6d type=%-3s got=%.9e float64=%.17e" % (kind, n, norm_type, norm, norm64))
            assert np.isfinite(norm) and norm > 0
            if norm_type == INF:
                assert norm == np.float32(norm64), (n, norm, norm64)             # bit for bit
            else:
                assert norm in GR.norm_candidates(norm64), (n, norm, norm64)
            want = GR.clip_coef(norm, max_norm)
            assert coef.view(np.uint32) == want.view(np.uint32), (n, norm_type, max_norm, coef, want)
            again = _norm(g, norm_type, max_norm)                                # two calls, the same bits
            assert again[0].view(np.uint32) == norm.view(np.uint32) and again[1].view(np.uint32) == coef.view(np.uint32)


def test_coefficient_branches():
    g = torch.full((1000,), 2.0, device=DEV)
    norm, coef = _norm(g, 2, 1e30)
    assert coef == 1.0                                                           # nothing to clip: exactly 1
    norm, coef = _norm(g, INF, 0.5)
    assert norm == 2.0 and coef == np.float32(0.5) / (np.float32(2.0) + np.float32(1e-6)) and coef < 1


@pytest.mark.parametrize("norm_type", [2, INF], ids=["l2", "inf"])
def test_non_finite_values_reach_the_norm(norm_type):
    for n in (257, CHUNK + 1, 3 * CHUNK + 5):
        for where in (0, n // 2, n - 1):                                         # first vector, the middle, the scalar tail
            host = _values("gauss", n)
            host[where] = float("nan")
            norm, coef = _norm(host.to(DEV), norm_type)
            assert np.isnan(norm) and np.isnan(coef), (n, where)                 # torch: NaN norm -> NaN coefficient
            host[where] = INF if where % 2 == 0 else -INF
            norm, coef = _norm(host.to(DEV), norm_type)
            assert norm == np.inf and coef == 0.0, (n, where)                    # ... an infinite norm -> 0
            host[(where + 7) % n] = float("nan")                                 # a NaN beside an Inf still wins
            assert np.isnan(_norm(host.to(DEV), norm_type)[0])


def test_empty_gradient_gives_norm_zero_and_coefficient_one():
    from ebfi_amd import _native as N
    out = torch.full((2,), -7.0, device=DEV)
    rc = N.lib().ebfi_grad_norm(N.ptr(None), 0, 0, 0.5, N.ptr(out), N.ptr(None), 0, N.stream_ptr(torch.device(DEV)))
    N.check(rc, "ebfi_grad_norm")
    assert out.tolist() == [0.0, 1.0]


# ------------------------------------------------------------------------------------------------ the update kernel
N_UPD = 4099                                                                     # 1024 float4 + 3: more than one workgroup and the tail
HYPER = dict(lr=1e-2, b1=0.9, b2=0.999, eps=1e-8, wd=0.0, mom=0.0, damp=0.0)
SPELLED = {"adamw_ams": (0, 1 | 2, dict(wd=0.1)), "adam_l2": (0, 0, dict(wd=1e-2)), "sgd_nesterov_l2": (1, 4, dict(wd=1e-3, mom=0.9))}


def _data(n, steps, seed):
    g = torch.Generator().manual_seed(seed)
    p = torch.randn(n, generator=g) * torch.exp(torch.rand(n, generator=g) * 7 - 6)
    grads = []
    for _ in range(steps):
        x = torch.randn(n, generator=g) * torch.exp(torch.rand(n, generator=g) * 14 - 12)
        x[2::5] = 0.0
        grads.append(x)
    return p, grads


class Flat:
    """The buffers of one run of an entry point: parameters, three state maps, the step words, the guard, the average."""

    def __init__(self, p0, kind, flags, **hyper):
        n = p0.numel()
        self.kind, self.flags, self.h = kind, flags, dict(HYPER, **hyper)
        self.p = p0.clone().to(DEV)
        self.s = [torch.zeros(n, device=DEV) for _ in range(3)]
        self.step, self.ema_step = torch.zeros((), device=DEV), torch.zeros((), device=DEV)
        self.guard = torch.zeros(2, dtype=torch.int32, device=DEV)
        self.ema = p0.clone().to(DEV)

    def tensors(self):
        return {"p": self.p, "s0": self.s[0], "s1": self.s[1], "s2": self.s[2], "step": self.step, "ema": self.ema,
                "ema_step": self.ema_step}

    def run(self, g, scale=None, ema=None, plain=False):
        """plain: ebfi_optim_step; otherwise ebfi_optim_step_ex with scale (a device float or None) and ema = (decay, warmup)."""
        from ebfi_amd import _native as N
        h, lib = self.h, N.lib()
        self.step += 1                                                           # the host increments both words before the launch
        if ema is not None:
            self.ema_step += 1
        head = (self.kind, self.flags, N.ptr(self.p), N.ptr(g), N.ptr(self.s[0]), N.ptr(self.s[1]),
                N.ptr(self.s[2] if self.flags & 2 and self.kind == 0 else None), N.ptr(self.step), self.p.numel(), h["lr"], h["b1"],
                h["b2"], h["eps"], h["wd"], h["mom"], h["damp"], N.ptr(self.guard), N.ptr(None))
        if plain:
            rc = lib.ebfi_optim_step(*head, N.stream_ptr(torch.device(DEV)))
        else:
            decay, warmup = ema if ema is not None else (0.0, False)
            rc = lib.ebfi_optim_step_ex(*head, N.ptr(scale), N.ptr(self.ema if ema is not None else None),
                                        N.ptr(self.ema_step if ema is not None else None), decay, int(warmup),
                                        N.stream_ptr(torch.device(DEV)))
        N.check(rc, "optim step")


@pytest.mark.parametrize("config", sorted(SPELLED))
def test_a_scale_gives_the_bits_of_a_pre_multiplied_gradient(config):
    kind, flags, hyper = SPELLED[config]
    p0, grads = _data(N_UPD, 3, seed=21)
    s = np.float32(0.37)
    scale = torch.tensor([float(s)], device=DEV)
    a, b = Flat(p0, kind, flags, **hyper), Flat(p0, kind, flags, **hyper)
    for g in grads:
        dev = g.to(DEV)
        keep = dev.clone()
        a.run(dev, scale=scale)
        assert _same_bits(dev, keep)                                             # the gradient buffer is only read
        b.run(torch.from_numpy(g.numpy() * s).to(DEV), plain=True)               # multiplied in float32 on the host
    torch.cuda.synchronize()
    for key in ("p", "s0", "s1", "s2", "step"):
        assert _same_bits(a.tensors()[key], b.tensors()[key]), key
    assert float(a.step) == 3 and not torch.equal(a.p.cpu(), p0) and _same_bits(a.ema, p0)      # (no average asked: none written)


def test_plain_adam_with_a_scale_within_four_times_torch_float32_error():
    import test_gpu_optim as TO
    p0, grads = _data(N_UPD, 3, seed=22)
    s = np.float32(0.37)
    scale = torch.tensor([float(s)], device=DEV)
    run = Flat(p0, 0, 0)
    for g in grads:
        run.run(g.to(DEV), scale=scale)
    pre = [torch.from_numpy(g.numpy() * s) for g in grads]
    lrs = [HYPER["lr"]] * 3
    p64, s64 = TO._torch_run("Adam", {}, p0, pre, torch.float64, lrs)
    p32, s32 = TO._torch_run("Adam", {}, p0, pre, torch.float32, lrs)
    worst = {}
    for key, got, r64, r32 in (("param", run.p, p64, p32), ("exp_avg", run.s[0], s64["exp_avg"], s32["exp_avg"]),
                               ("exp_avg_sq", run.s[1], s64["exp_avg_sq"], s32["exp_avg_sq"])):
        e, e32 = TO._err(got, r64, HYPER["lr"]), TO._err(r32, r64, HYPER["lr"])
        print("optim-ex plain adam + scale %-10s e=%.3e e32=%.3e ratio=%.2f" % (key, e, e32, e / e32 if e32 > 0 else float(e > 0)))
        if not e <= 4.0 * e32:
            worst[key] = (e, e32)
    assert not worst, worst


def test_null_route_is_ebfi_optim_step():
    p0, grads = _data(N_UPD, 3, seed=23)
    a, b = Flat(p0, 0, 0), Flat(p0, 0, 0)
    for g in grads:
        a.run(g.to(DEV))                                                         # grad_scale == NULL, ema == NULL
        b.run(g.to(DEV), plain=True)
    torch.cuda.synchronize()
    assert all(_same_bits(a.tensors()[k], b.tensors()[k]) for k in a.tensors()) and not torch.equal(a.p.cpu(), p0)


@pytest.mark.parametrize("warmup", [False, True], ids=["fixed", "warmup"])
@pytest.mark.parametrize("config", ["adam", "adam_scaled", "sgd_nesterov_l2"])
def test_moving_average_matches_the_restatement_and_a_skipped_step_moves_nothing(config, warmup):
    kind, flags, hyper = (0, 0, {}) if config.startswith("adam") else SPELLED[config]
    scale = torch.tensor([0.5], device=DEV) if config == "adam_scaled" else None
    p0, grads = _data(N_UPD, 5, seed=24)
    run, ref = Flat(p0, kind, flags, **hyper), GR.EmaRef(p0.numpy(), 0.9, warmup)
    for k, g in enumerate(grads):
        skip = k == 2                                                            # step 3 is skipped by the guard
        run.guard[0] = 1 if skip else 0
        before = {key: t.clone() for key, t in run.tensors().items()}
        skipped_before = int(run.guard[1])
        run.run(g.to(DEV), scale=scale, ema=(0.9, warmup))
        if skip:
            for key, t in run.tensors().items():                                 # parameters, state, both step words, the average
                assert _same_bits(t, before[key]), key
            assert run.guard.tolist() == [1, skipped_before + 1]                 # counted exactly once
        else:
            assert not _same_bits(run.p, before["p"]) and int(run.guard[1]) == skipped_before
        want = ref.update(run.p.cpu().numpy(), skipped=skip)
        assert np.array_equal(run.ema.cpu().numpy().view(np.uint32), want.view(np.uint32)), k
    assert float(run.ema_step) == ref.step == 4 and float(run.step) == 4 and run.guard.tolist() == [0, 1]
    assert not _same_bits(run.ema, run.p)


# ------------------------------------------------------------------------------------------------ engines
def _batch(seed):
    from ebfi_amd.engine import synthetic_batch
    return synthetic_batch(2, 64, 64, TB=4, device=DEV, seed=seed)


def _engine(**kw):
    from ebfi_amd.engine import Engine
    kw.setdefault("precision", "fp32")
    return Engine(SMALL, device=DEV, seed=3, **kw)


ADAMW = {"name": "AdamW", "args": {"lr": 1e-3, "weight_decay": 1e-2}}


@pytest.fixture(scope="module")
def unclipped_sgd():
    """One SGD step without clipping -> (start, parameters after it, the float64 norm of its packed gradient)."""
    eng = _engine(optimizer={"name": "SGD", "args": {"lr": 1e-2}})
    start = eng.optimizer.flat.detach().clone()
    eng.train_step(*_batch(50))
    return start.cpu(), eng.optimizer.flat.detach().clone().cpu(), float(GR.total_norm(eng.bucket.flat.cpu().numpy()))


@pytest.mark.parametrize("graph", [False, True], ids=["eager", "graph"])
def test_a_bound_that_never_binds_changes_no_bit(graph):
    finals = []
    for clip in (None, (1e30, 2)):
        eng = _engine(graph=graph, optimizer=ADAMW, clip_grad=clip)
        for it in range(3):
            eng.train_step(*_batch(50 + it))
        assert graph == (len(eng._graphs) == 1)
        finals.append(eng.optimizer.flat.detach().clone())
        if clip is not None:
            assert float(eng.optimizer.last_grad_norm[1]) == 1.0 and float(eng.optimizer.last_grad_norm[0]) > 0
    assert _same_bits(*finals)


def test_an_effective_clip_shrinks_the_first_update(unclipped_sgd):
    start, unclipped, norm64 = unclipped_sgd
    max_norm = 0.1 * norm64
    eng = _engine(optimizer={"name": "SGD", "args": {"lr": 1e-2}}, clip_grad=(max_norm, 2))
    eng.train_step(*_batch(50))
    got = eng.optimizer.last_grad_norm.cpu().numpy()
    flat = eng.bucket.flat.cpu().numpy()
    assert got[0] in GR.norm_candidates(GR.total_norm(flat)) and got[1] == GR.clip_coef(got[0], max_norm) and got[1] < 1
    assert eng.bucket.views_intact() and float(GR.total_norm(flat)) == norm64              # p.grad keeps the unclipped gradient
    moved = (eng.optimizer.flat.detach().cpu().double() - start.double()).norm()
    free = (unclipped.double() - start.double()).norm()
    print("clip: first update %.6e against %.6e unclipped (ratio %.6f)" % (moved, free, moved / free))
    # SGD: the update is lr * c * g with c ~ 0.1, so the clipped update is a tenth of the free one up to the roundings of
    # p - lr c g (2^-24 relative to |p| per element); "smaller" is the bar, and half leaves those roundings no say
    assert 0 < moved < 0.5 * free


def test_under_accumulation_the_norm_is_the_windows():
    eng = _engine(optimizer=ADAMW, clip_grad=(1e-6, INF), accu_step=2)
    eng.train_step(*_batch(60))
    first = eng.bucket.flat.detach().clone()
    assert eng.iteration == 0 and eng.optimizer.last_grad_norm.tolist() == [0.0, 1.0]      # no step yet: no norm launched
    eng.train_step(*_batch(61))
    assert eng.iteration == 1
    window = eng.bucket.flat.cpu().numpy()                                                   # the summed gradient of both passes
    got = eng.optimizer.last_grad_norm.cpu().numpy()
    assert got[0] == np.float32(GR.total_norm(window, INF)) and got[1] == GR.clip_coef(got[0], 1e-6)
    assert got[0] != np.float32(GR.total_norm(first.cpu().numpy(), INF))


def test_bf16x3_overflow_skips_the_step_and_leaves_the_average():
    eng = _engine(precision="bf16x3", ema=(0.5, False), clip_grad=(1.0, 2))
    assert eng.book is not None
    for it in range(2):
        eng.train_step(*_batch(70 + it))
    opt = eng.optimizer
    s0 = eng.book.skipped_steps()                                                # (0 is expected; a genuine skip counts on both sides)
    assert float(opt.ema_step) == 2 - s0 and s0 < 2
    before = (opt.flat.detach().clone(), opt.ema_flat.clone(), opt.inner.state[opt.flat]["exp_avg"].clone())
    begin = eng.book.begin_step

    def planted():                                                               # an overflow raised right after the guard was cleared
        begin()
        eng.book.guard[0] = 1
    eng.book.begin_step = planted
    eng.train_step(*_batch(72))
    eng.book.begin_step = begin
    assert eng.book.skipped_steps() == s0 + 1 and float(opt.ema_step) == 2 - s0 and float(opt.inner.state[opt.flat]["step"]) == 2 - s0
    assert _same_bits(opt.flat, before[0]) and _same_bits(opt.ema_flat, before[1])
    assert _same_bits(opt.inner.state[opt.flat]["exp_avg"], before[2])
    eng.train_step(*_batch(73))                                                  # and the next clean step moves both again
    assert eng.book.skipped_steps() == s0 + 1 and float(opt.ema_step) == 3 - s0
    assert not _same_bits(opt.flat, before[0]) and not _same_bits(opt.ema_flat, before[1])


def test_ema_weights_restores_and_leaves_training_as_found():
    from ebfi_amd.engine import synthetic_validation_batch
    vb = synthetic_validation_batch(2, 64, 64, TB=4, num_frames=2, device=DEV, seed=5)
    engines = [_engine(ema=(0.5, False)) for _ in range(2)]
    for eng in engines:
        for it in range(3):
            eng.train_step(*_batch(80 + it))
    eng, twin = engines
    opt = eng.optimizer
    raw, avg = opt.flat.detach().clone(), opt.ema_flat.clone()
    assert not _same_bits(raw, avg) and _same_bits(raw, twin.optimizer.flat)
    buffers = {k: v.clone() for k, v in eng.model.named_buffers()}
    with eng.ema_weights():
        assert _same_bits(opt.flat, avg) and _same_bits(opt.ema_flat, raw)
        inside = eng.validate(vb)
        assert _same_bits(opt.flat, avg)                                         # (the nested context of validate changed nothing)
    assert _same_bits(opt.flat, raw) and _same_bits(opt.ema_flat, avg) and opt.views_intact()
    assert all(torch.equal(v, buffers[k]) for k, v in eng.model.named_buffers())
    averaged, plain = eng.validate(vb), eng.validate(vb, use_ema=False)          # by default validate scores the average
    assert _same_bits(opt.flat, raw) and _same_bits(opt.ema_flat, avg)
    for key in eng.VALID_KEYS:
        assert float(averaged[key]) == float(inside[key]) and float(averaged[key]) != float(plain[key]), key
    # checkpoints: model.states the raw iterate, ema.states the average
    state = eng.ema_state()
    flat_of = lambda states: torch.cat([states[n].reshape(-1) for n, p in eng.model.named_parameters() if p.requires_grad])
    assert _same_bits(flat_of(state["states"]), avg) and _same_bits(flat_of(eng.model.state_dict()), raw) and state["step"] == 3
    # the next training step is the one of the run that never entered the context
    for e in engines:
        e.train_step(*_batch(83))
    assert _same_bits(opt.flat, twin.optimizer.flat) and _same_bits(opt.ema_flat, twin.optimizer.ema_flat)
    assert not _same_bits(opt.flat, raw)
    with pytest.raises(ValueError):
        _engine().validate(vb, use_ema=True)


def test_exposure_engine_takes_both_through_the_shared_stepper():
    from ebfi_amd.exposure_engine import ExposureEngine, synthetic_exposure_batch
    eng = ExposureEngine(fashion="RGBDark", device=DEV, precision="fp32", seed=4, clip_grad=(1e-3, 2), ema=(0.9, True))
    start = eng.optimizer.flat.detach().clone()
    batch = synthetic_exposure_batch(2, 32, 32, TB=16, device=DEV, seed=60)
    eng.train_step(*batch)
    got = eng.optimizer.last_grad_norm.cpu().numpy()
    assert got[0] in GR.norm_candidates(GR.total_norm(eng.bucket.flat.cpu().numpy())) and got[1] == GR.clip_coef(got[0], 1e-3)
    want = GR.ema_update(start.cpu().numpy(), eng.optimizer.flat.detach().cpu().numpy(), 0.9, True, 1)
    assert np.array_equal(eng.optimizer.ema_flat.cpu().numpy().view(np.uint32), want.view(np.uint32))
    a, b = eng.validate(batch), eng.validate(batch, use_ema=False)
    assert float(a["valid_loss"]) != float(b["valid_loss"])


def test_default_step_launches_no_new_kernel():
    """Both features off: the labels of one eager step hold the update it has always launched and none of the new ones; with
    them on, the two norm launches and the extended update replace it."""
    from ebfi_amd import _native as N
    seen = []
    for kw in ({}, {"clip_grad": (1.0, 2), "ema": (0.9, False)}):
        eng = _engine(**kw)
        eng.train_step(*_batch(90))
        torch.cuda.synchronize()
        N.prof_reset()
        N.prof_enable(True)
        try:
            eng.train_step(*_batch(91))
            torch.cuda.synchronize()
            seen.append({k: v[0] for k, v in N.prof_collect().items() if v[0]})
        finally:
            N.prof_enable(False)
            N.prof_reset()
    off, on = seen
    new = ("grad_norm_chunk", "grad_norm_finish", "optim_ex_adam_ema")
    assert off.get("adam_flat") == 1 and not any(k.startswith(("grad_norm", "optim_ex")) for k in off), sorted(off)
    assert all(on.get(k) == 1 for k in new) and "adam_flat" not in on, sorted(on)
    assert {k: v for k, v in on.items() if k not in new} == {k: v for k, v in off.items() if k != "adam_flat"}


# ------------------------------------------------------------------------------------------------ trainer and inference
def test_trainer_checkpoints_resumes_and_infers_the_average(tmp_path):
    cfg = yaml.safe_load(open(os.path.join(PKG, "config", "train_ours.yml")))
    cfg["model"]["args"].update(SMALL)
    cfg["trainer"].update(batch_size=2, height=64, width=64, output_path=str(tmp_path / "out"),
                          clip_grad={"max_norm": 1e-3, "norm_type": 2}, ema={"decay": 0.9, "warmup": True})
    cfg["trainer"]["iteration_based_train"].update(iterations=4, save_period=0, train_log_step=1)
    cfg_path = tmp_path / "cfg.yml"
    cfg_path.write_text(yaml.safe_dump(cfg))
    env = dict(os.environ, PYTHONPATH=PKG)
    train = [sys.executable, os.path.join(PKG, "train_ours.py"), "-c", str(cfg_path), "--precision", "fp32"]
    r = subprocess.run(train + ["-id", "a"], capture_output=True, text=True, env=env, timeout=600)
    assert r.returncode == 0, r.stderr[-2000:]
    assert "Iteration: 3/4" in r.stdout and r.stdout.count(" grad_norm: ") == 4, r.stdout[-1500:]
    ckpt = tmp_path / "out" / "models" / "Ours" / "a" / "checkpoint-iteration3.pth"
    cpt = torch.load(str(ckpt), map_location="cpu", weights_only=False)
    assert tuple(cpt)[:5] == ("model", "lr_scheduler", "optimizer", "config", "trainer") and tuple(cpt)[5:] == ("ema",)
    ema = cpt["ema"]
    assert (ema["decay"], ema["warmup"], ema["step"]) == (0.9, True, 4)
    trainable = [k for k in cpt["model"]["states"] if k in ema["states"]]
    assert len(trainable) == len(ema["states"]) > 0
    assert any(not torch.equal(ema["states"][k], cpt["model"]["states"][k]) for k in trainable)
    # --resume restores the average: one more iteration from it, with --ema-decay overriding the config's decay
    r = subprocess.run(train + ["-id", "b", "--resume", str(ckpt), "--iterations", "5", "--ema-decay", "0.5", "--clip-grad-norm", "1e30"],
                       capture_output=True, text=True, env=env, timeout=600)
    assert r.returncode == 0 and "Iteration: 4/5" in r.stdout and "Iteration: 3/5" not in r.stdout, r.stderr[-2000:] + r.stdout[-500:]
    cpt2 = torch.load(str(tmp_path / "out" / "models" / "Ours" / "b" / "checkpoint-iteration4.pth"), map_location="cpu", weights_only=False)
    assert (cpt2["ema"]["decay"], cpt2["ema"]["step"]) == (0.5, 5)
    for k in trainable:                                                          # e5 = e4 + w (p5 - e4), from the RESTORED e4
        want = GR.ema_update(ema["states"][k].numpy(), cpt2["model"]["states"][k].numpy(), 0.5, True, 5)
        assert np.array_equal(cpt2["ema"]["states"][k].numpy().view(np.uint32), want.view(np.uint32)), k
    # inference on the averaged weights; a checkpoint without them is refused with a message
    infer = [sys.executable, os.path.join(PKG, "infer_ours.py"), "--batch", "1", "--height", "64", "--width", "64", "--num_ts", "2",
             "--precision", "fp32"]
    r = subprocess.run(infer + ["--model_path", str(ckpt), "--ema"], capture_output=True, text=True, env=env, timeout=600)
    assert r.returncode == 0 and "interpolated 2 frames" in r.stdout, r.stderr[-2000:]
    bare = {k: v for k, v in cpt.items() if k != "ema"}
    torch.save(bare, str(tmp_path / "bare.pth"))
    import importlib.util                                                        # (the flag's whole path ran above: the refusal needs no process)
    spec = importlib.util.spec_from_file_location("ebfi_infer_ours_gradclip", os.path.join(PKG, "infer_ours.py"))
    infer_mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(infer_mod)
    with pytest.raises(SystemExit, match="holds no averaged weights"):
        infer_mod.load_model(str(tmp_path / "bare.pth"), torch.device(DEV), ema=True)
    assert infer_mod.get_flags(["--ema"]).ema is True and infer_mod.get_flags([]).ema is False
