#!/usr/bin/env python3
"""Evaluation metrics (ebfi_amd.metrics.frame_metrics: tile + finalize kernels) at the size of one config 5 load -- 16 frames of
3 x 720 x 1280, the NumF of one load -- and at 16 x 3 x 256 x 256: device events around `iters` calls after a warm-up; prints
microseconds per call and per frame and the achieved bytes/s (2 N C H W 4 bytes read per call) as a fraction of the 8 TB/s HBM
peak.  usage: python tools/metricsbench.py [iters]"""
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "ebfi-be_amd"))
import torch  # noqa: E402

from ebfi_amd.metrics import frame_metrics  # noqa: E402

HBM_PEAK = 8e12
ITERS = int(sys.argv[1]) if len(sys.argv) > 1 else 50


def bench(N, C, H, W):
    g = torch.Generator(device="cuda").manual_seed(0)
    target = torch.rand(N, C, H, W, device="cuda", generator=g)
    pred = (target + 0.05 * torch.randn(N, C, H, W, device="cuda", generator=g)).clamp(0, 1)
    for _ in range(5):
        frame_metrics(pred, target)
    # a buffer larger than the 256 MiB last-level cache written between calls would keep the inputs from staying resident;
    # at config 5 they are 354 MB and do not fit anyway, so the calls run back to back
    torch.cuda.synchronize()
    t0, t1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    t0.record()
    for _ in range(ITERS):
        frame_metrics(pred, target)
    t1.record()
    torch.cuda.synchronize()
    us = t0.elapsed_time(t1) * 1e3 / ITERS
    nbytes = 2.0 * N * C * H * W * 4
    row = dict(shape=[N, C, H, W], us_per_call=round(us, 2), us_per_frame=round(us / N, 3), bytes=int(nbytes),
               tb_per_s=round(nbytes / us / 1e6, 3), hbm_fraction=round(nbytes / (us * 1e-6) / HBM_PEAK, 3))
    print(json.dumps(row), flush=True)
    return row


if __name__ == "__main__":
    assert torch.cuda.is_available(), "metricsbench needs the MI355X"
    bench(16, 3, 720, 1280)
    bench(16, 3, 256, 256)
