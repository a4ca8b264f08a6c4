"""Validation on the MI355X: the Charbonnier kernels (csrc/charbonnier.hip) against the float64 restatement of
tests/test_validation_host.py, Engine.validate against the reference's validation loop restated here (train_ours.py:566-591),
the two traps of validating with a training engine (stale weights, isolation of the training state), and train_ours.py with
validation switched on: stamps, best checkpoints, monitor_best through a resume, early stop."""
import os
import re
import subprocess
import sys

import numpy as np
import pytest
import torch
import yaml

from test_validation_host import ref_charbonnier

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
PKG = os.path.join(ROOT, "ebfi-be_amd")
EPS = 1e-3


def _pairs():
    """(name, x, y) device pairs: one and three channels, a ragged tail, 720x1280, a strided row view, a view with a ragged tail
    on 16-byte aligned rows, and a base pointer one element off 16 bytes (the scalar-load path)."""
    g = torch.Generator(device="cpu").manual_seed(0)
    rnd = lambda *s: torch.rand(*s, generator=g).cuda()
    out = [("one channel", rnd(2, 1, 16, 16), rnd(2, 1, 16, 16)),
           ("three channels", rnd(2, 3, 64, 64), rnd(2, 3, 64, 64)),
           ("ragged tail", rnd(3, 3, 37, 129), rnd(3, 3, 37, 129)),
           ("720x1280", rnd(8, 3, 720, 1280), rnd(8, 3, 720, 1280))]
    bx, by = rnd(2, 3, 40, 160), rnd(2, 3, 40, 160)
    out.append(("strided rows", bx[:, :, 4:36, 16:144], by[:, :, 4:36, 16:144]))
    out.append(("strided rows, ragged", bx[:, 1:, :, :126], by[:, 1:, :, :126]))
    n = 2 * 3 * 20 * 24
    fx, fy = rnd(n + 4), rnd(n + 4)
    out.append(("offset base", fx[1:n + 1].view(2, 3, 20, 24), fy[1:n + 1].view(2, 3, 20, 24)))
    assert out[-1][1].data_ptr() % 16 == 4 and out[4][1].data_ptr() % 16 == 0 and not out[4][1].is_contiguous()
    return out


def test_charbonnier_forward_matches_float64():
    """relative 1e-6 on every per-sample sum -- derived, not measured: every term is positive and carries the fp32 roundings of
    the subtraction, the fused multiply-add and the root (each <= 2^-24 relative), the fp64 accumulation adds nothing visible, and
    the sum is rounded to fp32 once: about 3e-7 in the worst case."""
    from ebfi_amd.loss import CharbonnierLoss, charbonnier_per_sample
    for name, x, y in _pairs():
        got = charbonnier_per_sample(x, y, EPS)
        want = ref_charbonnier(x.cpu().numpy(), y.cpu().numpy(), EPS)
        rel = np.abs(got.cpu().numpy().astype(np.float64) - want) / want
        print("charbonnier forward %-22s max rel err %.2e" % (name, rel.max()))
        assert got.shape == (x.shape[0],) and got.dtype == torch.float32
        assert rel.max() <= 1e-6, (name, rel)
        total = CharbonnierLoss(EPS)(x, y)
        assert total.dim() == 0 and abs(total.item() - want.sum()) <= 1e-6 * want.sum(), name
    # hand-derivable: equal inputs give n * sqrt(eps), a constant offset d gives n * sqrt(d^2 + eps)
    x = torch.rand(2, 3, 33, 47, device="cuda")
    n = 3 * 33 * 47
    assert np.allclose(charbonnier_per_sample(x, x.clone()).cpu().numpy(), n * np.sqrt(1e-3), rtol=1e-6)
    assert np.allclose(charbonnier_per_sample(torch.zeros_like(x), torch.full_like(x, 0.25)).cpu().numpy(),
                       n * np.sqrt(0.0625 + 1e-3), rtol=1e-6)


def test_charbonnier_backward_matches_float64_autograd():
    """absolute 1e-6 * |g| per element: |d / sqrt(d^2 + eps)| <= 1, so the forward's relative bound is this absolute one."""
    from ebfi_amd.loss import CharbonnierLoss
    gscale = 2.5
    for name, x, y in _pairs():
        if name == "720x1280":
            x, y = x[:2], y[:2]
        xg = x.detach().clone().requires_grad_(True) if x.is_contiguous() else x.detach().requires_grad_(True)
        (CharbonnierLoss(EPS)(xg, y) * gscale).backward()
        x64 = x.detach().cpu().double().requires_grad_(True)
        d = x64 - y.cpu().double()
        (torch.sqrt(d * d + EPS).sum() * gscale).backward()
        err = (xg.grad.cpu().double() - x64.grad).abs().max().item()
        print("charbonnier backward %-22s max abs err %.2e (bound %.2e)" % (name, err, 1e-6 * gscale))
        assert xg.grad.shape == x.shape and err <= 1e-6 * gscale, (name, err)
    # the gradient with respect to y is the negative
    x, y = torch.rand(1, 3, 9, 11, device="cuda", requires_grad=True), torch.rand(1, 3, 9, 11, device="cuda", requires_grad=True)
    CharbonnierLoss()(x, y).backward()
    assert torch.equal(x.grad, -y.grad) and x.grad.abs().max() > 0


def test_charbonnier_nan_reproducibility_and_graph_capture():
    from ebfi_amd.loss import CharbonnierLoss, charbonnier_per_sample
    g = torch.Generator(device="cpu").manual_seed(1)
    x, y = torch.rand(3, 3, 50, 70, generator=g).cuda(), torch.rand(3, 3, 50, 70, generator=g).cuda()
    a, b = charbonnier_per_sample(x, y), charbonnier_per_sample(x, y)
    assert torch.equal(a, b)                                   # no atomics: bit-identical
    bad = y.clone()
    bad[1, 2, 49, 69] = float("nan")
    got = charbonnier_per_sample(x, bad)
    assert torch.isnan(got[1]) and torch.equal(got[[0, 2]], a[[0, 2]])
    bad[1, 2, 49, 69] = float("inf")
    assert not torch.isfinite(charbonnier_per_sample(x, bad)[1])
    # both entry points inside a captured graph: replays follow new inputs
    sx, sy = x.clone().requires_grad_(True), y.clone()
    loss_fn = CharbonnierLoss()
    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):
        loss_fn(sx, sy).backward()                              # warm-up: workspace, autograd buffers
    torch.cuda.current_stream().wait_stream(side)
    sx.grad = None
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        per = charbonnier_per_sample(sx.detach(), sy)
        total = loss_fn(sx, sy)
        total.backward()
    eager_x = x.flip(0).contiguous().requires_grad_(True)
    eager = loss_fn(eager_x, y)
    eager.backward()
    with torch.no_grad():
        sx.copy_(eager_x)
    graph.replay()
    torch.cuda.synchronize()
    assert torch.equal(total, eager) and torch.equal(sx.grad, eager_x.grad) and torch.equal(per, charbonnier_per_sample(eager_x.detach(), y))


# ------------------------------------------------------------------ Engine.validate
SMALL = dict(step=2, channels=[8, 8, 16, 16])


def _signal(eng, seed):
    """The default x0.1 initialisation gives Final == 0.5 everywhere: give the weights a size that produces an image."""
    g = torch.Generator(device="cpu").manual_seed(seed)
    with torch.no_grad():
        for p in eng.model.parameters():
            if p.dim() > 1:
                p.copy_((torch.randn(p.shape, generator=g) * (1.2 / p[0].numel() ** 0.5)).to(p.device))
    return eng


def _reference_loop(eng, batch):
    """train_ours.py:573-588 restated: eval mode, one module call per latent timestamp, the float64 Charbonnier sum of
    Final vs LatentF over the whole batch, divided by NumI.  Returns (valid_loss, frames [B, NumI, 3, H, W])."""
    from ebfi_amd import conv
    frame, event, ts, gtex, latent = batch
    model = eng.model
    modes = [(m, m.training) for m in model.modules()]
    prev = conv.get_compute_dtype()
    conv.set_compute_dtype(eng.precision)
    model.eval()
    try:
        with torch.no_grad():
            frames = [model(frame, event, ts[:, [i]].contiguous(), gtex)[-1].float() for i in range(ts.shape[1])]
    finally:
        conv.set_compute_dtype(prev)
        for m, flag in modes:
            m.training = flag
    num_i = len(frames)
    loss = sum(ref_charbonnier(f.cpu().numpy(), latent[:, i].cpu().numpy(), EPS).sum() for i, f in enumerate(frames)) / num_i
    return loss, torch.stack(frames, 1)


def test_validate_equals_the_reference_loop_fp32():
    from ebfi_amd.engine import Engine, synthetic_validation_batch
    from ebfi_amd.metrics import frame_metrics
    eng = _signal(Engine(SMALL, device="cuda", seed=3, precision="fp32"), 3)
    batch = synthetic_validation_batch(2, 64, 64, 16, num_frames=4, device="cuda", seed=-1)
    want, frames = _reference_loop(eng, batch)
    got = eng.validate(batch, group=1)
    assert set(got) == {"valid_loss", "valid_psnr", "valid_ssim"} and all(v.is_cuda and v.dim() == 0 for v in got.values())
    print("validate fp32 group=1: valid_loss %.9e, reference loop %.9e" % (got["valid_loss"].item(), want))
    # group=1 is bit-identical to the module call (test_hoisted_inference_is_bit_identical): only the loss arithmetic differs
    assert abs(got["valid_loss"].item() - want) <= 1e-6 * want
    assert frames.std() > 1e-3 and want > 2 * 3 * 64 * 64 * np.sqrt(EPS)
    psnr, ssim, _ = frame_metrics(frames.reshape(-1, 3, 64, 64), batch[4].reshape(-1, 3, 64, 64))
    assert got["valid_psnr"].item() == pytest.approx(psnr.double().mean().item(), rel=1e-12)
    assert got["valid_ssim"].item() == pytest.approx(ssim.double().mean().item(), rel=1e-12)
    # the same call through a collated clipdata batch (dict layout [B, L=1, ...])
    frame, event, ts, gtex, latent = batch
    as_dict = {"SeqLatentF": latent[:, None, None], "SeqBlurryF": frame[:, None, None], "SeqHREv": event[:, None],
               "RelativeLatentTs": ts[:, None, None], "SeqExposureDuty": gtex[:, None, None]}
    again = eng.validate(as_dict, group=1)
    assert all(torch.equal(again[k], got[k]) for k in got)
    assert eng.validator(1) is eng.validator(1) and all(m.training for m in eng.model.modules())


def test_grouped_validation_agrees_with_one_timestamp_per_pass():
    """Grouped passes agree with group=1 to 1e-5 of the frame maximum per pixel (tests/test_gpu_entrypoints.py:254).  Every term
    sqrt(d^2 + eps) has slope <= 1 in d, so a frame error of delta per pixel moves a term by at most delta; valid_loss sums
    B * 3 * H * W terms per timestamp and averages over the timestamps: |difference| <= B * 3 * H * W * 1e-5 * max|Final|."""
    from ebfi_amd.engine import Engine, synthetic_validation_batch
    eng = _signal(Engine(SMALL, device="cuda", seed=4, precision="bf16x3"), 4)
    B, H, W = 2, 64, 64
    batch = synthetic_validation_batch(B, H, W, 16, num_frames=4, device="cuda", seed=-2)
    one = eng.validate(batch, group=1)
    grouped = eng.validate(batch)
    assert eng.validator(None).last_group == 4 and eng.validator(1).last_group == 1
    fmax = eng.validator(1)(batch[0], batch[1], batch[3], [batch[2][:, i] for i in range(4)]).abs().max().item()
    bound = B * 3 * H * W * 1e-5 * fmax
    diff = abs(grouped["valid_loss"].item() - one["valid_loss"].item())
    print("grouped vs group=1: valid_loss %.9e / %.9e, difference %.3e, bound %.3e" %
          (grouped["valid_loss"].item(), one["valid_loss"].item(), diff, bound))
    assert diff <= bound and fmax > 0.1


def test_validation_sees_the_weights_of_the_native_optimiser():
    """FlatAdam's native step writes the flat parameter buffer through a raw pointer: no tensor version counter moves, and the
    validator's inference bank would serve the weights it packed when it was built.  validate() re-packs it."""
    from ebfi_amd.engine import Engine, synthetic_batch, synthetic_validation_batch
    eng = _signal(Engine(SMALL, device="cuda", seed=5, precision="bf16x3", lr=1e-3), 5)
    batch = synthetic_validation_batch(2, 64, 64, 16, num_frames=4, device="cuda", seed=-3)
    before = {k: v.clone() for k, v in eng.validate(batch).items()}
    for k in range(3):
        eng.train_step(*synthetic_batch(2, 64, 64, device="cuda", seed=900 + k))
    stale = eng.validate(batch, refresh=False)                  # (reported, not asserted: what the bank serves when nobody re-packs it)
    print("without a re-pack the validator serves the old weights: %s" % torch.equal(stale["valid_loss"], before["valid_loss"]))
    after = eng.validate(batch)
    fresh = Engine(SMALL, device="cuda", seed=99, precision="bf16x3")
    fresh.model.load_state_dict(eng.model.state_dict())
    want = fresh.validate(batch)
    print("valid_loss before %.9e, after three steps %.9e, fresh engine %.9e" %
          (before["valid_loss"].item(), after["valid_loss"].item(), want["valid_loss"].item()))
    for key in want:
        assert torch.equal(after[key], want[key]), key
    assert not torch.equal(after["valid_loss"], before["valid_loss"])


def test_validation_leaves_the_training_state_alone():
    """Two engines from one seed take the four steps of test_training_step_is_bit_reproducible (two eager calibration steps,
    the capture, a replay); one of them validates after steps 1 and 3.  Losses, packed gradients and parameters stay
    bit-identical, no step is skipped, and every piece of training state validate could touch is as it was."""
    from ebfi_amd import conv, f16scale, weightbank
    from ebfi_amd.engine import Engine, synthetic_batch, synthetic_validation_batch
    vbatch = synthetic_validation_batch(2, 128, 128, 16, num_frames=4, device="cuda", seed=-4)
    runs = []
    for validating in (False, True):
        eng = Engine(dict(step=3), device="cuda", seed=21, graph=True, precision="bf16x3")
        losses, grads = [], []
        for k in range(4):
            losses.append(eng.train_step(*synthetic_batch(2, 128, 128, device="cuda", seed=500 + k)).item())
            grads.append(eng.bucket.flat.detach().clone())
            if validating and k in (0, 2):
                snap = lambda: ([m.training for m in eng.model.modules()], eng.book.slots.clone(), eng.book.guard.clone(),
                                set(eng.book.calibrated), dict(eng.book.index), list(eng._graphs), eng._micro, eng._accum,
                                eng._steps_run, eng.iteration, conv.get_compute_dtype(), weightbank.active_bank(),
                                f16scale.active_book(), [None if p.grad is None else p.grad.data_ptr() for p in eng.bucket.params], eng.optimizer.flat.clone())
                was = snap()
                vals = eng.validate(vbatch)
                now = snap()
                assert torch.isfinite(vals["valid_loss"]) and vals["valid_loss"] > 0
                for i, (a, b) in enumerate(zip(was, now)):
                    assert torch.equal(a, b) if torch.is_tensor(a) else a == b, i
                assert all(was[0]) and eng.bucket.views_intact() and eng.optimizer.views_intact()
                assert eng.validator().bank is not eng.bank and eng.validator().book is not eng.book
        torch.cuda.synchronize()
        assert eng.book is not None and eng.book.skipped_steps() == 0 and len(eng._graphs) == 1
        runs.append((losses, grads, eng.optimizer.flat.detach().clone()))
        del eng
    (la, ga, pa), (lb, gb, pb) = runs
    assert la == lb, (la, lb)
    for k in range(4):
        assert torch.equal(ga[k], gb[k]), k
    assert torch.equal(pa, pb)


# ------------------------------------------------------------------ train_ours.py
def _run(cfg_path, *extra):
    env = dict(os.environ, PYTHONPATH=PKG)
    return subprocess.run([sys.executable, os.path.join(PKG, "train_ours.py"), "-c", str(cfg_path)] + list(extra),
                          capture_output=True, text=True, env=env, timeout=900)


def test_trainer_validates_saves_the_best_and_stops_early(tmp_path):
    from ebfi_amd import clipdata
    clip = clipdata.write_synthetic_clip(str(tmp_path / "clip.npz"), num_imgs=33, H=64, W=64, seed=1)
    cfg = yaml.safe_load(open(os.path.join(PKG, "config", "train_ours.yml")))
    cfg["model"]["args"].update(FrameBasech=16, EventBasech=16, InterCH=16, TB=4, step=2, channels=[4, 4, 8, 8])
    cfg["trainer"].update(batch_size=2, height=64, width=64, output_path=str(tmp_path / "out"), do_validation=True,
                          monitor="min valid_loss", early_stop=10)
    cfg["trainer"]["iteration_based_train"].update(iterations=5, save_period=1000, valid_step=2, train_log_step=1)
    dataset = dict(scale=1, ori_scale="ori", time_bins=4, NumFramePerPeriod=4, NumFramePerBlurry=4, ExposureMethod="Fixed")
    cfg["train_dataloader"] = {"dataset": dict(dataset)}
    cfg["valid_dataloader"]["dataset"].update(dataset)
    cfg_path = tmp_path / "cfg.yml"
    cfg_path.write_text(yaml.safe_dump(cfg))
    r = _run(cfg_path, "-id", "v", "--data", clip, "--valid-data", clip)
    assert r.returncode == 0, r.stderr[-3000:]
    print(r.stdout[-3000:])
    stamps = re.findall(r"^Valid stamp: (\d+) valid_loss: (\S+) valid_psnr: (\S+) valid_ssim: (\S+) \(best (\S+)\)$", r.stdout, re.M)
    assert [s[0] for s in stamps] == ["1", "2"]
    lines = r.stdout.splitlines()
    at = lambda text: next(i for i, l in enumerate(lines) if l.startswith(text))
    # stamps follow the log lines of iterations 2 and 4; none at iteration 0 (train_ours.py:312)
    assert at("Iteration: 2/5") < at("Valid stamp: 1") < at("Iteration: 3/5") and at("Iteration: 4/5") < at("Valid stamp: 2")
    assert at("Iteration: 0/5") < at("Iteration: 1/5") < at("Valid stamp: 1")
    run_dir = tmp_path / "out" / "models" / "Ours" / "v"
    first, best = run_dir / "checkpoint-iteration2.pth", run_dir / "model_best_until_iteration2.pth"
    assert first.exists() and best.exists()                    # the first stamp always improves on +inf: both files
    a, b = (torch.load(str(p), map_location="cpu", weights_only=False) for p in (first, best))
    assert a["trainer"] == b["trainer"] and a["trainer"]["iteration"] == 2
    assert a["trainer"]["monitor_best"] == float(stamps[0][4]) == pytest.approx(float(stamps[0][1]), rel=1e-6)
    n_pix = 2 * 3 * 64 * 64
    assert float(stamps[0][1]) >= n_pix * np.sqrt(1e-3) and 0 < float(stamps[0][3]) < 1 and np.isfinite(float(stamps[0][2]))
    last = torch.load(str(run_dir / "checkpoint-iteration4.pth"), map_location="cpu", weights_only=False)
    assert last["trainer"]["monitor_best"] == float(stamps[1][4]) == min(float(stamps[0][4]), float(stamps[1][4]))
    assert (run_dir / "model_best_until_iteration4.pth").exists() == (float(stamps[1][1]) <= float(stamps[0][4]))

    # early stop, deterministic: a best of 0.0 cannot be reached (the loss is at least n * sqrt(eps) > 0)
    a["trainer"]["monitor_best"] = 0.0
    rewritten = tmp_path / "rewritten.pth"
    torch.save(a, str(rewritten))
    cfg["trainer"]["early_stop"] = 1
    cfg["trainer"]["iteration_based_train"]["iterations"] = 20
    cfg_path.write_text(yaml.safe_dump(cfg))
    r = _run(cfg_path, "-id", "stop", "--data", clip, "--valid-data", clip, "--resume", str(rewritten))
    assert r.returncode == 0, r.stderr[-3000:]
    print(r.stdout[-3000:])
    stamps = re.findall(r"^Valid stamp: (\d+) .* \(best (\S+)\)$", r.stdout, re.M)
    assert stamps == [("1", "0.0"), ("2", "0.0")]              # iterations 4 and 6: not_improved_count 1, then 2 > early_stop
    assert "Validation performance didn't improve for 1 stamps. Training stops." in r.stdout
    assert "Iteration: 3/20" in r.stdout and "Iteration: 6/20" in r.stdout and "Iteration: 7/20" not in r.stdout
    stop_dir = tmp_path / "out" / "models" / "Ours" / "stop"
    assert sorted(os.listdir(str(stop_dir))) == ["checkpoint-iteration6.pth"]         # resumable; no model_best_*
    end = torch.load(str(stop_dir / "checkpoint-iteration6.pth"), map_location="cpu", weights_only=False)
    assert end["trainer"] == {"training_mode": "iteration_based_train", "iteration": 6, "monitor_best": 0.0}


def test_trainer_validates_on_synthetic_batches_with_max_psnr(tmp_path):
    """No validation clips: the fixed synthetic set; monitor 'max valid_psnr' works through the same path."""
    cfg = yaml.safe_load(open(os.path.join(PKG, "config", "train_ours.yml")))
    cfg["model"]["args"].update(FrameBasech=16, EventBasech=16, InterCH=16, TB=4, step=2, channels=[4, 4, 8, 8])
    cfg["trainer"].update(batch_size=2, height=64, width=64, output_path=str(tmp_path / "out"), do_validation=True,
                          monitor="max valid_psnr", valid_batches=2)
    cfg["trainer"]["iteration_based_train"].update(iterations=3, save_period=1000, valid_step=2, train_log_step=1)
    cfg["valid_dataloader"]["dataset"].update(NumFramePerPeriod=3)
    cfg_path = tmp_path / "cfg.yml"
    cfg_path.write_text(yaml.safe_dump(cfg))
    r = _run(cfg_path, "-id", "s", "--graph")
    assert r.returncode == 0, r.stderr[-3000:]
    stamps = re.findall(r"^Valid stamp: (\d+) valid_loss: (\S+) valid_psnr: (\S+) valid_ssim: (\S+) \(best (\S+)\)$", r.stdout, re.M)
    assert len(stamps) == 1 and float(stamps[0][4]) == pytest.approx(float(stamps[0][2]), rel=1e-6)
    run_dir = tmp_path / "out" / "models" / "Ours" / "s"
    assert sorted(os.listdir(str(run_dir))) == ["checkpoint-iteration2.pth", "model_best_until_iteration2.pth"]
    cpt = torch.load(str(run_dir / "checkpoint-iteration2.pth"), map_location="cpu", weights_only=False)
    assert cpt["trainer"]["monitor_best"] == float(stamps[0][4])
    assert "0 of 3 optimiser steps skipped" in r.stdout
