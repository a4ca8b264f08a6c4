#!/usr/bin/env python3
"""Launches and milliseconds per stage-1 step (ExposureEngine: blur level -> ExposureDecision -> duty head + MSE -> backward ->
gradient packing -> Adam) at the reference's stage-1 shape, with the native duty head (csrc/dutyhead.hip) and, for comparison,
with the torch tail it replaces (AdaptiveAvgPool2d + sigmoid + MSELoss / accu_step).  Information only: prints one JSON line per
variant.  The two variants alternate in one process; times are device-event times over `--steps` steps after `--warmup`, launches
are the device kernels of one eager step as torch.profiler counts them (taken after the timing, in a pass of their own).

    python tools/stage1_step.py [--batch 4 --size 128 --tb 16 --fashion RGBLap --precision bf16x3 --steps 200 --rounds 3]
"""
import argparse
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [ROOT, os.path.join(ROOT, "ebfi-be_amd")]

import torch  # noqa: E402
import torch.nn as nn  # noqa: E402


class TorchTail(nn.Module):
    """What DutyMSELoss replaces, with its call contract."""

    def __init__(self, scale):
        super().__init__()
        self.scale, self.pool, self.mse, self.Ex = scale, nn.AdaptiveAvgPool2d(1), nn.MSELoss(), None

    def forward(self, ex, duty):
        Ex = torch.sigmoid(self.pool(ex).view(-1, 1))
        self.Ex = Ex.detach()
        return self.mse(Ex, duty) * self.scale


def make(args, tail, graph):
    from ebfi_amd.exposure_engine import BLURRY_FASHIONS, ExposureEngine
    eng = ExposureEngine(dict(EventInch=2 * args.tb, BLInch=BLURRY_FASHIONS[args.fashion]), fashion=args.fashion, precision=args.precision,
                         seed=1, graph=graph)
    if tail == "torch":
        eng.loss = TorchTail(1.0 / eng.accu_step)
    return eng


def timed(eng, batch, steps):
    ev = [torch.cuda.Event(enable_timing=True) for _ in range(2)]
    ev[0].record()
    for _ in range(steps):
        eng.train_step(*batch)
    ev[1].record()
    ev[1].synchronize()
    return ev[0].elapsed_time(ev[1]) / steps


def launches(eng, batch):
    from torch.profiler import ProfilerActivity, profile
    torch.cuda.synchronize()
    with profile(activities=[ProfilerActivity.CPU, ProfilerActivity.CUDA]) as prof:
        eng.train_step(*batch)
        torch.cuda.synchronize()
    dev = [e for e in prof.events() if str(getattr(e, "device_type", "")).endswith("CUDA")]
    kernels = [e for e in dev if not e.name.lower().startswith(("memcpy", "memset"))]
    return len(kernels), len(dev) - len(kernels)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--batch", type=int, default=4)
    ap.add_argument("--size", type=int, default=128)
    ap.add_argument("--tb", type=int, default=16)
    ap.add_argument("--fashion", default="RGBLap")
    ap.add_argument("--precision", default="bf16x3")
    ap.add_argument("--steps", type=int, default=200)
    ap.add_argument("--warmup", type=int, default=20)
    ap.add_argument("--rounds", type=int, default=3)
    args = ap.parse_args()
    assert torch.cuda.is_available(), "needs the GPU"
    from ebfi_amd.exposure_engine import synthetic_exposure_batch
    batch = synthetic_exposure_batch(args.batch, args.size, args.size, args.tb, device="cuda", seed=3)
    for graph in (False, True):
        engines = {tail: make(args, tail, graph) for tail in ("native", "torch")}
        times = {tail: [] for tail in engines}
        for eng in engines.values():
            for _ in range(args.warmup):
                eng.train_step(*batch)
        torch.cuda.synchronize()
        for _ in range(args.rounds):                 # alternate the variants: other work shares the machine
            for tail, eng in engines.items():
                times[tail].append(timed(eng, batch, args.steps))
        for tail, eng in engines.items():
            out = {"variant": tail + "_tail", "graph": graph, "precision": args.precision, "fashion": args.fashion,
                   "shape": [args.batch, args.size, args.size, args.tb], "ms_per_step": [round(t, 4) for t in times[tail]],
                   "ms_per_step_min": round(min(times[tail]), 4), "graph_capture_failed": eng.graph_capture_failed}
            if not graph:
                out["kernel_launches_per_step"], out["copies_per_step"] = launches(eng, batch)
            print(json.dumps(out), flush=True)


if __name__ == "__main__":
    main()
