#!/usr/bin/env python3
"""The STGAN adversarial loss (ebfi_amd.gan) timed on the device at B = 8, 128 x 128 and 256 x 256.  One JSON line per row:

  call       one Adversarial call + the backward into `fake` (the discriminator's step: two passes, their parameter gradients,
             Adamax; then the generator's pass and its data gradient), eager launches, device events around each of `iters`
             calls after a warm-up: mean / min / max microseconds; per-kernel rows from the library's event profiler (a
             separate pass: its events serialise the launches) and, from them, the share of the two linear layers
  eager      the same law as PyTorch eager modules in float32 on the same GPU (nn.Conv2d / BatchNorm2d / LeakyReLU / Linear,
             autograd, torch.optim.Adamax): what the reference runs.  --no-eager skips it (MIOpen may compile kernels for the
             sixteen convolution shapes first)
  step       the captured training step of the default model with and without the term (--no-step skips it): frames / s

usage: python tools/ganbench.py [iters] [--sizes 128 256] [--no-eager] [--no-step]"""
import argparse
import json
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "ebfi-be_amd"))
import torch  # noqa: E402
import torch.nn.functional as F  # noqa: E402

from ebfi_amd import _native as N  # noqa: E402
from ebfi_amd.gan import Adversarial, AdversarialTerm  # noqa: E402


def inputs(B, P, seed=0):
    g = torch.Generator(device="cuda").manual_seed(seed)
    real = torch.rand(B, 3, P, P, device="cuda", generator=g)
    fake = (real + 0.05 * torch.randn(B, 3, P, P, device="cuda", generator=g)).requires_grad_(True)
    return fake, real, torch.rand(B, 2, 3, P, P, device="cuda", generator=g)


def time_steps(step, iters):
    for _ in range(3):
        step()
    torch.cuda.synchronize()
    ev = [(torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)) for _ in range(iters)]
    for t0, t1 in ev:
        t0.record()
        step()
        t1.record()
    torch.cuda.synchronize()
    us = [t0.elapsed_time(t1) * 1e3 for t0, t1 in ev]
    return dict(us_mean=round(sum(us) / len(us), 1), us_min=round(min(us), 1), us_max=round(max(us), 1))


def kernel_rows(step, iters):
    N.prof_enable(True)
    N.prof_reset()
    try:
        for _ in range(iters):
            step()
            torch.cuda.synchronize()
            N.prof_fold()
        stats = N.prof_collect(strict=False)
    finally:
        N.prof_enable(False)
        N.prof_reset()
    return {k: dict(launches_per_call=v[0] // iters, us_per_call=round(v[1] * 1e3 / iters, 1),
                    gbytes_per_s=round(v[3] / max(v[1] * 1e-3, 1e-12) / 1e9, 1) if v[3] else None)
            for k, v in sorted(stats.items()) if not k.startswith("__") and v[0]}


def bench_call(B, P, iters):
    adv = Adversarial(P, "STGAN").cuda()
    fake, real, frames = inputs(B, P)

    def step():
        fake.grad = None
        adv(fake, real, frames).backward()

    row = dict(row="call", shape=[B, 3, P, P], parameters=adv.discriminator.flat.numel(), **time_steps(step, iters))
    kernels = kernel_rows(step, min(iters, 3))
    total = sum(v["us_per_call"] for v in kernels.values())
    linear = sum(v["us_per_call"] for k, v in kernels.items() if k.startswith("linear_"))
    row.update(kernel_us_total=round(total, 1), linear_us=round(linear, 1), linear_share=round(linear / max(total, 1e-9), 3), kernels=kernels)
    print(json.dumps(row), flush=True)
    return adv


def bench_eager(adv, B, P, iters):
    """The containers of a discriminator ARE torch modules: run them as such (fresh copies, so nothing is shared)."""
    import copy
    D = adv.discriminator
    s_f, t_f, cls = (copy.deepcopy(m).cuda() for m in (D.s_features, D.t_features, D.classifier))
    params = [p for m in (s_f, t_f, cls) for p in m.parameters()]
    opt = torch.optim.Adamax(params, lr=1e-3, betas=(0.9, 0.999), eps=1e-8)
    fake, real, frames = inputs(B, P)
    f0, f2 = frames[:, 0], frames[:, 1]

    def disc(f1):
        s, t = s_f(f1), t_f(torch.cat([f1 - f0, f1 - f2], 1))
        return cls(torch.cat([s.reshape(B, -1), t.reshape(B, -1)], 1))

    def step():
        opt.zero_grad()
        d_fake, d_real = disc(fake.detach()), disc(real)
        loss_d = F.binary_cross_entropy_with_logits(d_fake, torch.zeros_like(d_fake)) + \
            F.binary_cross_entropy_with_logits(d_real, torch.ones_like(d_real))
        loss_d.backward()
        opt.step()
        fake.grad = None
        d_g = disc(fake)
        F.binary_cross_entropy_with_logits(d_g, torch.ones_like(d_g)).backward()

    t = time.perf_counter()
    step()
    torch.cuda.synchronize()
    first = time.perf_counter() - t
    print(json.dumps(dict(row="eager", shape=[B, 3, P, P], first_call_s=round(first, 2), **time_steps(step, iters))), flush=True)


def bench_step(B, P, steps):
    from ebfi_amd.engine import Engine, synthetic_batch
    for with_term in (False, True):
        term = AdversarialTerm(Adversarial(P, "STGAN"), 0.01) if with_term else None
        eng = Engine(device="cuda", precision="bf16x3", lr=1e-4, seed=7, graph=True, adversarial=term)
        batch = synthetic_batch(B, P, P, device="cuda", seed=5, on_device=True)
        if with_term:
            batch = batch + (torch.rand(B, 2, 3, P, P, device="cuda"),)
        for _ in range(5):                      # two calibration steps, the capture, two replays
            eng.train_step(*batch)
        torch.cuda.synchronize()
        t = time.perf_counter()
        for _ in range(steps):
            eng.train_step(*batch)
        torch.cuda.synchronize()
        dt = (time.perf_counter() - t) / steps
        print(json.dumps(dict(row="step", shape=[B, 3, P, P], adversarial=with_term, captured=bool(eng._graphs) and eng.use_graph,
                              ms_per_step=round(dt * 1e3, 3), frames_per_s=round(B / dt, 1))), flush=True)
        del eng


if __name__ == "__main__":
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("iters", type=int, nargs="?", default=10)
    ap.add_argument("--sizes", type=int, nargs="+", default=[128, 256])
    ap.add_argument("--no-eager", action="store_true")
    ap.add_argument("--no-step", action="store_true")
    a = ap.parse_args()
    assert torch.cuda.is_available(), "ganbench needs the MI355X"
    advs = {P: bench_call(8, P, a.iters) for P in a.sizes}
    if not a.no_step:
        for P in a.sizes:
            bench_step(8, P, max(a.iters, 10))
    if not a.no_eager:
        for P in a.sizes:
            bench_eager(advs[P], 8, P, a.iters)
