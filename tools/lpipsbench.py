#!/usr/bin/env python3
"""LPIPS (ebfi_amd.lpips: finite check, five implicit-GEMM convolutions on fp32 MFMA, distance + finalize kernels) at the size of
one config 5 load -- 16 pairs of 3 x 720 x 1280 -- and at 16 x 3 x 256 x 256: device events around `iters` calls after a
warm-up, with a random AlexNet trunk (the time does not depend on the weights).  Prints microseconds per call, the algorithmic
FLOPs of each trunk layer (2 * pixels * Cout * Cin * k * k per image, from the shapes here) and the achieved fraction of the
157.3 TF fp32 matrix peak.  usage: python tools/lpipsbench.py [iters]"""
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "ebfi-be_amd"))
import torch  # noqa: E402

from ebfi_amd.lpips import CONV_SHAPES, AlexLPIPS  # noqa: E402

FP32_MATRIX_PEAK = 157.3e12
ITERS = int(sys.argv[1]) if len(sys.argv) > 1 else 10


def layer_flops(n_images, H, W):
    h1, w1 = (H + 4 - 11) // 4 + 1, (W + 4 - 11) // 4 + 1
    h2, w2 = (h1 - 3) // 2 + 1, (w1 - 3) // 2 + 1
    h3, w3 = (h2 - 3) // 2 + 1, (w2 - 3) // 2 + 1
    pixels = [h1 * w1, h2 * w2, h3 * w3, h3 * w3, h3 * w3]
    return [2.0 * n_images * p * co * ci * k * k for p, (co, ci, k, _) in zip(pixels, CONV_SHAPES)]


def bench(model, N, C, H, W):
    g = torch.Generator(device="cuda").manual_seed(0)
    target = torch.rand(N, C, H, W, device="cuda", generator=g)
    pred = target + 0.05 * torch.randn(N, C, H, W, device="cuda", generator=g)
    for _ in range(3):
        model(pred, target)
    torch.cuda.synchronize()
    t0, t1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    t0.record()
    for _ in range(ITERS):
        model(pred, target)
    t1.record()
    torch.cuda.synchronize()
    us = t0.elapsed_time(t1) * 1e3 / ITERS
    fl = layer_flops(2 * N, H, W)
    row = dict(shape=[N, C, H, W], us_per_call=round(us, 1), us_per_pair=round(us / N, 2),
               gflop_per_layer=[round(f / 1e9, 2) for f in fl], gflop=round(sum(fl) / 1e9, 1),
               tflops=round(sum(fl) / (us * 1e-6) / 1e12, 2), fp32_matrix_peak_fraction=round(sum(fl) / (us * 1e-6) / FP32_MATRIX_PEAK, 3))
    print(json.dumps(row), flush=True)
    return row


if __name__ == "__main__":
    assert torch.cuda.is_available(), "lpipsbench needs the MI355X"
    g = torch.Generator().manual_seed(0)
    ws = [torch.randn(s, generator=g) * (2.0 / (s[1] * s[2] * s[3])) ** 0.5 for s in CONV_SHAPES]
    bs = [0.01 + 0.05 * torch.rand(s[0], generator=g) for s in CONV_SHAPES]
    hs = [torch.rand(s[0], generator=g) for s in CONV_SHAPES]
    model = AlexLPIPS(ws, bs, hs, "cuda")
    bench(model, 16, 3, 720, 1280)
    bench(model, 16, 3, 256, 256)
