#!/usr/bin/env python3
"""LPIPS (ebfi_amd.lpips) timed with device events around `iters` calls after a warm-up, with a random trunk (the time does not
depend on the weights).  Prints one JSON line per shape: microseconds per call, the algorithmic FLOPs of each trunk layer
(2 * pixels * Cout * Cin * k * k per image, from the shapes here) and the achieved fraction of the 157.3 TF fp32 matrix peak.

  --net alex (default)  finite check, five implicit-GEMM convolutions on fp32 MFMA, distance + finalize kernels, at the size of
                        one config 5 load -- 16 pairs of 3 x 720 x 1280 -- and at 16 x 3 x 256 x 256
  --net vgg             prologue, 13 exact-fp32 3x3 convolutions, five tap kernels, finalize: one 720 x 1280 pair and sixteen
                        256 x 256 pairs; mean and spread (min / max) over the timed calls, the share of the fp32 matrix bound
                        (FLOPs / peak: arithmetic from the shapes, not a measurement), per-kernel rows from the library's event
                        profiler (a separate pass: its events serialise the launches), and the AlexNet figure of the same call

  --net vgg --backward  the training loss: VggLPIPS.loss forward + backward (ebfi_lpips_vgg_forward_train / _backward) at
                        8 x 3 x 256 x 256 and at one 720 x 1280 pair: mean and spread per step, the forward alone, per-kernel rows
                        from the event profiler (the tap adjoint's bytes and rate among them), the 64 -> 3 data gradient timed
                        alone and its share, the training workspace, and -- as context: it is what the reference runs -- PyTorch
                        eager autograd through the same trunk (F.conv2d / F.max_pool2d / F.relu in float32) on the same device

  --net alex --backward the same rows for AlexLPIPSLoss.loss (ebfi_lpips_alex_forward_train / _backward): step, forward alone,
                        backward (the difference), score, the training workspace, per-kernel rows from the event profiler (the
                        five tap adjoints, the MFMA data gradients of conv5 .. conv2 and the direct 11x11 stride-4 kernel
                        with its input epilogue), and PyTorch eager autograd through the AlexNet trunk

usage: python tools/lpipsbench.py [iters] [--net {alex,vgg}] [--backward]"""
import argparse
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "ebfi-be_amd"))
import torch  # noqa: E402

from ebfi_amd import _native as N  # noqa: E402
from ebfi_amd.lpips import CONV_SHAPES, VGG_CONV_SHAPES, VGG_HEAD_CHANNELS, AlexLPIPS, AlexLPIPSLoss, VggLPIPS  # noqa: E402

FP32_MATRIX_PEAK = 157.3e12


def layer_flops(n_images, H, W):
    h1, w1 = (H + 4 - 11) // 4 + 1, (W + 4 - 11) // 4 + 1
    h2, w2 = (h1 - 3) // 2 + 1, (w1 - 3) // 2 + 1
    h3, w3 = (h2 - 3) // 2 + 1, (w2 - 3) // 2 + 1
    pixels = [h1 * w1, h2 * w2, h3 * w3, h3 * w3, h3 * w3]
    return [2.0 * n_images * p * co * ci * k * k for p, (co, ci, k, _) in zip(pixels, CONV_SHAPES)]


def vgg_layer_flops(n_images, H, W):
    level = [0, 0, 1, 1, 2, 2, 2, 3, 3, 3, 4, 4, 4]          # pools before each of the 13 convolutions
    return [2.0 * n_images * (H >> s) * (W >> s) * co * ci * 9 for s, (co, ci, _, _) in zip(level, VGG_CONV_SHAPES)]


def pair(N_, C, H, W):
    g = torch.Generator(device="cuda").manual_seed(0)
    target = torch.rand(N_, C, H, W, device="cuda", generator=g)
    pred = target + 0.05 * torch.randn(N_, C, H, W, device="cuda", generator=g)
    return pred, target


def time_calls(model, pred, target, iters):
    """Per-call microseconds of `iters` calls, each between its own pair of device events."""
    for _ in range(3):
        model(pred, target)
    torch.cuda.synchronize()
    ev = [(torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)) for _ in range(iters)]
    for t0, t1 in ev:
        t0.record()
        model(pred, target)
        t1.record()
    torch.cuda.synchronize()
    return [t0.elapsed_time(t1) * 1e3 for t0, t1 in ev]


def bench(model, N_, C, H, W, iters):
    pred, target = pair(N_, C, H, W)
    for _ in range(3):
        model(pred, target)
    torch.cuda.synchronize()
    t0, t1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    t0.record()
    for _ in range(iters):
        model(pred, target)
    t1.record()
    torch.cuda.synchronize()
    us = t0.elapsed_time(t1) * 1e3 / iters
    fl = layer_flops(2 * N_, H, W)
    row = dict(shape=[N_, C, H, W], us_per_call=round(us, 1), us_per_pair=round(us / N_, 2),
               gflop_per_layer=[round(f / 1e9, 2) for f in fl], gflop=round(sum(fl) / 1e9, 1),
               tflops=round(sum(fl) / (us * 1e-6) / 1e12, 2), fp32_matrix_peak_fraction=round(sum(fl) / (us * 1e-6) / FP32_MATRIX_PEAK, 3))
    print(json.dumps(row), flush=True)
    return row


def kernel_rows(model, pred, target, iters):
    """{kernel: microseconds per call} from the library's event profiler."""
    N.prof_enable(True)
    N.prof_reset()
    try:
        for _ in range(iters):
            model(pred, target)
            torch.cuda.synchronize()
            N.prof_fold()
        stats = N.prof_collect(strict=False)
    finally:
        N.prof_enable(False)
        N.prof_reset()
    return {k: dict(launches_per_call=v[0] // iters, us_per_call=round(v[1] * 1e3 / iters, 1),
                    tflops=round(v[2] / max(v[1] * 1e-3, 1e-12) / 1e12, 2) if v[2] else None,
                    gbytes_per_s=round(v[3] / max(v[1] * 1e-3, 1e-12) / 1e9, 1) if v[3] else None)
            for k, v in sorted(stats.items()) if not k.startswith("__") and v[0]}


def bench_vgg(vgg, alex, N_, C, H, W, iters):
    pred, target = pair(N_, C, H, W)
    us = time_calls(vgg, pred, target, iters)
    us_alex = time_calls(alex, pred, target, iters)
    mean = sum(us) / len(us)
    fl = vgg_layer_flops(2 * N_, H, W)
    bound_us = sum(fl) / FP32_MATRIX_PEAK * 1e6
    row = dict(net="vgg", shape=[N_, C, H, W], chunk=vgg._chunk(N_, C, H, W), us_per_call=round(mean, 1), us_min=round(min(us), 1),
               us_max=round(max(us), 1), us_per_pair=round(mean / N_, 1), gflop_per_conv=[round(f / 1e9, 2) for f in fl],
               gflop=round(sum(fl) / 1e9, 1), fp32_matrix_bound_us=round(bound_us, 1), tflops=round(sum(fl) / (mean * 1e-6) / 1e12, 2),
               fp32_matrix_peak_fraction=round(bound_us / mean, 3),
               alex_us_per_call=round(sum(us_alex) / len(us_alex), 1), alex_us_min=round(min(us_alex), 1),
               alex_us_max=round(max(us_alex), 1), kernels=kernel_rows(vgg, pred, target, min(iters, 3)))
    print(json.dumps(row), flush=True)
    return row


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


def torch_eager_loss(ws, bs, hs, pred, target, net="vgg"):
    """The reference's path: the same trunk and distances as torch ops in float32 (normalize=True), lpips [N]."""
    import torch.nn.functional as F
    shift = torch.tensor([-0.030, -0.088, -0.188], device=pred.device).view(1, 3, 1, 1)
    scale = torch.tensor([0.458, 0.448, 0.450], device=pred.device).view(1, 3, 1, 1)
    blocks = (2, 2, 3, 3, 3)

    def vgg_taps(x):
        x, out, i = (2 * x - 1 - shift) / scale, [], 0
        for k, n in enumerate(blocks):
            if k:
                x = F.max_pool2d(x, 2, 2)
            for _ in range(n):
                x = F.relu(F.conv2d(x, ws[i], bs[i], padding=1))
                i += 1
            out.append(x)
        return out

    def alex_taps(x):
        x = (2 * x - 1 - shift) / scale
        f1 = F.relu(F.conv2d(x, ws[0], bs[0], stride=4, padding=2))
        f2 = F.relu(F.conv2d(F.max_pool2d(f1, 3, 2), ws[1], bs[1], padding=2))
        f3 = F.relu(F.conv2d(F.max_pool2d(f2, 3, 2), ws[2], bs[2], padding=1))
        f4 = F.relu(F.conv2d(f3, ws[3], bs[3], padding=1))
        return [f1, f2, f3, f4, F.relu(F.conv2d(f4, ws[4], bs[4], padding=1))]

    taps = alex_taps if net == "alex" else vgg_taps
    unit = lambda f: f / (torch.sqrt((f ** 2).sum(1, keepdim=True)) + 1e-10)     # noqa: E731
    with torch.no_grad():
        t_taps = taps(target)
    total = 0
    for f0, f1, h in zip(taps(pred), t_taps, hs):
        total = total + (h.view(1, -1, 1, 1) * (unit(f0) - unit(f1)) ** 2).sum(1).mean((1, 2))
    return total


def bench_alex_backward(alex, weights, N_, C, H, W, iters):
    pred, target = pair(N_, C, H, W)
    pred.requires_grad_(True)

    def step():
        pred.grad = None
        alex.loss(pred, target).sum().backward()

    def forward_only():
        with torch.no_grad():
            alex.loss(pred, target)

    row = dict(net="alex", mode="forward_train+backward", shape=[N_, C, H, W],
               train_workspace_bytes=int(N.lib().ebfi_lpips_alex_train_workspace(N_, C, H, W)),
               score_workspace_bytes=int(N.lib().ebfi_lpips_workspace(N_, C, H, W)))
    row["step"] = time_steps(step, iters)
    row["forward_train"] = time_steps(forward_only, iters)
    row["score"] = time_steps(lambda: alex(pred.detach(), target), iters)
    row["backward_us"] = round(row["step"]["us_mean"] - row["forward_train"]["us_mean"], 1)

    class Both:                                    # (kernel_rows calls model(pred, target))
        def __call__(self, p, t):
            step()

    row["kernels"] = kernel_rows(Both(), pred, target, min(iters, 3))
    ws, bs, hs = ([t.to("cuda") for t in part] for part in weights)

    def eager_step():
        pred.grad = None
        torch_eager_loss(ws, bs, hs, pred, target, net="alex").sum().backward()

    row["torch_eager_step"] = time_steps(eager_step, iters)
    print(json.dumps(row), flush=True)
    return row


def bench_vgg_backward(vgg, weights, N_, C, H, W, iters):
    pred, target = pair(N_, C, H, W)
    pred.requires_grad_(True)

    def step():
        pred.grad = None
        vgg.loss(pred, target).sum().backward()

    def forward_only():
        with torch.no_grad():
            vgg.loss(pred, target)

    row = dict(net="vgg", mode="forward_train+backward", shape=[N_, C, H, W],
               train_workspace_bytes=int(N.lib().ebfi_lpips_vgg_train_workspace(N_, C, H, W)),
               score_workspace_bytes=int(N.lib().ebfi_lpips_vgg_workspace(N_, C, H, W)))
    row["step"] = time_steps(step, iters)
    row["forward_train"] = time_steps(forward_only, iters)
    row["score"] = time_steps(lambda: vgg(pred.detach(), target), iters)

    class Both:                                    # (kernel_rows calls model(pred, target))
        def __call__(self, p, t):
            step()

    row["kernels"] = kernel_rows(Both(), pred, target, min(iters, 3))
    # the first layer's data gradient (64 -> 3 on the generic tile) alone
    go, y = torch.randn(N_, 64, H, W, device="cuda"), torch.rand(N_, 64, H, W, device="cuda")
    gi, w0 = torch.empty(N_, 3, H, W, device="cuda"), vgg._keep[0][0]

    def dgrad0():
        rc = N.lib().ebfi_conv2d_backward_data(N.ptr(go), N.ptr(y), N.ptr(w0), N.ptr(gi), N_, 3, H, W, 64, 3, 1, 1, 1, 0.0, N.EBFI_F32,
                                               N.stream_ptr(vgg.device))
        N.check(rc, "ebfi_conv2d_backward_data")

    row["dgrad_64_to_3"] = time_steps(dgrad0, iters)
    backward_us = row["step"]["us_mean"] - row["forward_train"]["us_mean"]
    row["backward_us"] = round(backward_us, 1)
    row["dgrad_64_to_3_share_of_backward"] = round(row["dgrad_64_to_3"]["us_mean"] / max(backward_us, 1e-9), 3)
    dg = row["kernels"].get("conv_fwd_f32/dgrad")
    if dg:
        row["dgrad_share_of_backward_kernels"] = round(
            dg["us_per_call"] / max(sum(v["us_per_call"] for k, v in row["kernels"].items()
                                        if k in ("conv_fwd_f32/dgrad", "lpips_vgg_tap_bwd", "lpips_vgg_epilogue")), 1e-9), 3)
    ws, bs, hs = ([t.to("cuda") for t in part] for part in weights)

    def eager_step():
        pred.grad = None
        torch_eager_loss(ws, bs, hs, pred, target).sum().backward()

    row["torch_eager_step"] = time_steps(eager_step, iters)
    print(json.dumps(row), flush=True)
    return row


def random_weights(shapes, heads, g):
    ws = [torch.randn(s, generator=g) * (2.0 / (s[1] * s[2] * s[3])) ** 0.5 for s in shapes]
    bs = [0.01 + 0.05 * torch.rand(s[0], generator=g) for s in shapes]
    hs = [torch.rand(c, generator=g) for c in heads]
    return ws, bs, hs


if __name__ == "__main__":
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("iters", type=int, nargs="?", default=10)
    ap.add_argument("--net", choices=("alex", "vgg"), default="alex")
    ap.add_argument("--backward", action="store_true", help="time the training loss (forward_train + backward)")
    a = ap.parse_args()
    assert torch.cuda.is_available(), "lpipsbench needs the MI355X"
    g = torch.Generator().manual_seed(0)
    alex_weights = random_weights(CONV_SHAPES, [s[0] for s in CONV_SHAPES], g)
    if a.net == "alex" and a.backward:
        loss_model = AlexLPIPSLoss(*alex_weights, "cuda")
        bench_alex_backward(loss_model, alex_weights, 8, 3, 256, 256, a.iters)
        bench_alex_backward(loss_model, alex_weights, 1, 3, 720, 1280, a.iters)
        sys.exit(0)
    alex = AlexLPIPS(*alex_weights, "cuda")
    if a.net == "alex":
        bench(alex, 16, 3, 720, 1280, a.iters)
        bench(alex, 16, 3, 256, 256, a.iters)
    else:
        weights = random_weights(VGG_CONV_SHAPES, VGG_HEAD_CHANNELS, g)
        vgg = VggLPIPS(*weights, "cuda")
        if a.backward:
            bench_vgg_backward(vgg, weights, 8, 3, 256, 256, a.iters)
            bench_vgg_backward(vgg, weights, 1, 3, 720, 1280, a.iters)
            sys.exit(0)
        bench_vgg(vgg, alex, 1, 3, 720, 1280, a.iters)
        bench_vgg(vgg, alex, 16, 3, 256, 256, a.iters)
