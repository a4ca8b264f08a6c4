#!/usr/bin/env python3
"""The recurrent cells, the bilinear up-sampling (csrc/recurrent.hip) and one UNetFlow step timed on the device.  One JSON line
per row:

  cell       ConvLSTM / ConvGRU tails at B = 8, C = 64, 64 x 64 and 128 x 128: the native launch(es) through the C ABI, forward
             and backward, against the same expressions in PyTorch eager on the same GPU (forward under no_grad; backward =
             autograd.grad on the kept graph).  Device events around `iters` back-to-back calls after a warm-up; microseconds
             per call.  `floor_share`: the algorithmic traffic (LSTM forward: 7 C 4 bytes per pixel) at 8 TB/s over the time.
  bilinear   x2 at 8 x 64 x 128 x 128, forward and backward, against F.interpolate and its (atomic) adjoint
  gates      the GRU's update and reset convolutions on the stacked input: two C-output launches against one 2C-output launch
  step       one UNetFlow step (base 32, 3 encoders, 2 residual blocks, kernel_size 3 or --kernel-size, sum, convlstm,
             8 x 5 x 256 x 256), forward + backward from a fresh state, in both compute modes: milliseconds

usage: python tools/recurrentbench.py [iters] [--no-step | --step-only] [--kernel-size K]"""
import argparse
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "ebfi-be_amd"))
import torch  # noqa: E402
import torch.nn.functional as F  # noqa: E402

from ebfi_amd import _native as N  # noqa: E402
from ebfi_amd import conv  # noqa: E402

HBM = 8e12          # bytes / s, the figure README.md uses


def timed(call, iters):
    """microseconds per call: one event pair around `iters` back-to-back calls, three windows, the best and the worst."""
    for _ in range(5):
        call()
    torch.cuda.synchronize()
    us = []
    for _ in range(3):
        t0, t1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        t0.record()
        for _ in range(iters):
            call()
        t1.record()
        torch.cuda.synchronize()
        us.append(t0.elapsed_time(t1) * 1e3 / iters)
    return round(min(us), 2), round(max(us), 2)


def rand(*shape):
    return torch.randn(*shape, device="cuda")


def row(**kw):
    print(json.dumps(kw), flush=True)


def bench_lstm(B, C, S, iters):
    lib, st = N.lib(), N.stream_ptr()
    HW, n = S * S, B * C * S * S
    gates, prev, gh, gc = rand(B, 4 * C, S, S), rand(B, C, S, S), rand(B, C, S, S), rand(B, C, S, S)
    hidden, cell, dg, dp = torch.empty_like(prev), torch.empty_like(prev), torch.empty_like(gates), torch.empty_like(prev)
    fwd = lambda: lib.ebfi_lstm_cell_forward(N.ptr(gates), N.ptr(prev), N.ptr(hidden), N.ptr(cell), B, C, HW, st)
    bwd = lambda: lib.ebfi_lstm_cell_backward(N.ptr(gates), N.ptr(prev), N.ptr(cell), N.ptr(gh), N.ptr(gc), N.ptr(dg), N.ptr(dp), B, C, HW, st)

    def law(g, p):
        i, f, o, c = g.chunk(4, 1)
        i, f, o = torch.sigmoid(i), torch.sigmoid(f), torch.sigmoid(o)
        cl = f * p + i * torch.tanh(c)
        return o * torch.tanh(cl), cl

    def eager_fwd():
        with torch.no_grad():
            law(gates, prev)

    g_, p_ = gates.clone().requires_grad_(True), prev.clone().requires_grad_(True)
    outs = law(g_, p_)
    eager_bwd = lambda: torch.autograd.grad(outs, (g_, p_), (gh, gc), retain_graph=True)
    for kind, native, eager, nbytes in (("lstm forward", fwd, eager_fwd, 7 * 4 * n), ("lstm backward", bwd, eager_bwd, 13 * 4 * n)):
        (lo, hi), (elo, ehi) = timed(native, iters), timed(eager, iters)
        row(row="cell", kind=kind, shape=[B, C, S, S], native_us=lo, native_us_max=hi, eager_us=elo, eager_us_max=ehi,
            speedup=round(elo / lo, 2), algorithmic_bytes=nbytes, floor_us=round(nbytes / HBM * 1e6, 2),
            floor_share=round(nbytes / HBM * 1e6 / lo, 3))


def bench_gru(B, C, S, iters):
    lib, st = N.lib(), N.stream_ptr()
    HW, n = S * S, B * C * S * S
    rp, up, op, x, h = (rand(B, C, S, S) for _ in range(5))
    cat, new = torch.empty(B, 2 * C, S, S, device="cuda"), torch.empty_like(h)
    g_cat, g_new = rand(B, 2 * C, S, S), rand(B, C, S, S)
    dx, dr, dh1, du, do, dh2 = (torch.empty_like(h) for _ in range(6))

    def fwd():
        lib.ebfi_gru_reset_forward(N.ptr(rp), N.ptr(x), N.ptr(h), N.ptr(cat), B, C, C, HW, st)
        lib.ebfi_gru_update_forward(N.ptr(up), N.ptr(op), N.ptr(h), N.ptr(new), B, C, HW, st)

    def bwd():
        lib.ebfi_gru_update_backward(N.ptr(up), N.ptr(op), N.ptr(h), N.ptr(g_new), N.ptr(du), N.ptr(do), N.ptr(dh2), B, C, HW, st)
        lib.ebfi_gru_reset_backward(N.ptr(g_cat), N.ptr(rp), N.ptr(h), N.ptr(dh2), N.ptr(dx), N.ptr(dr), N.ptr(dh1), B, C, C, HW, st)

    def law(rp, up, op, x, h):
        u, r = torch.sigmoid(up), torch.sigmoid(rp)
        return torch.cat([x, h * r], 1), h * (1 - u) + torch.tanh(op) * u

    def eager_fwd():
        with torch.no_grad():
            law(rp, up, op, x, h)

    leaves = [t.clone().requires_grad_(True) for t in (rp, up, op, x, h)]
    outs = law(*leaves)
    eager_bwd = lambda: torch.autograd.grad(outs, leaves, (g_cat, g_new), retain_graph=True)
    for kind, native, eager, nbytes in (("gru forward (both halves)", fwd, eager_fwd, (5 + 4) * 4 * n),
                                        ("gru backward (both halves)", bwd, eager_bwd, (7 + 8) * 4 * n)):
        (lo, hi), (elo, ehi) = timed(native, iters), timed(eager, iters)
        row(row="cell", kind=kind, shape=[B, C, S, S], native_us=lo, native_us_max=hi, eager_us=elo, eager_us_max=ehi,
            speedup=round(elo / lo, 2), algorithmic_bytes=nbytes, floor_us=round(nbytes / HBM * 1e6, 2),
            floor_share=round(nbytes / HBM * 1e6 / lo, 3))


def bench_bilinear(B, C, S, scale, iters):
    lib, st = N.lib(), N.stream_ptr()
    x, g = rand(B, C, S, S), rand(B, C, scale * S, scale * S)
    out, dx = torch.empty_like(g), torch.empty_like(x)
    fwd = lambda: lib.ebfi_bilinear_up_forward(N.ptr(x), N.ptr(out), B * C, S, S, scale, st)
    bwd = lambda: lib.ebfi_bilinear_up_backward(N.ptr(g), N.ptr(dx), B * C, S, S, scale, st)

    def eager_fwd():
        with torch.no_grad():
            F.interpolate(x, scale_factor=scale, mode="bilinear", align_corners=False)

    x_ = x.clone().requires_grad_(True)
    y = F.interpolate(x_, scale_factor=scale, mode="bilinear", align_corners=False)
    eager_bwd = lambda: torch.autograd.grad(y, x_, g, retain_graph=True)
    nbytes = (1 + scale * scale) * 4 * x.numel()
    for kind, native, eager in (("bilinear x%d forward" % scale, fwd, eager_fwd), ("bilinear x%d backward" % scale, bwd, eager_bwd)):
        (lo, hi), (elo, ehi) = timed(native, iters), timed(eager, iters)
        row(row="bilinear", kind=kind, shape=[B, C, S, S], native_us=lo, native_us_max=hi, eager_us=elo, eager_us_max=ehi,
            speedup=round(elo / lo, 2), algorithmic_bytes=nbytes, floor_us=round(nbytes / HBM * 1e6, 2),
            floor_share=round(nbytes / HBM * 1e6 / lo, 3))


def bench_gates(B, C, S, iters):
    """update_gate and reset_gate read the same stacked input: two launches of C outputs, or one of 2C."""
    for mode in ("fp32", "bf16x3"):
        conv.set_compute_dtype(mode)
        try:
            x = rand(B, 2 * C, S, S)
            wu, wr, bu, br = rand(C, 2 * C, 3, 3) * 0.03, rand(C, 2 * C, 3, 3) * 0.03, rand(C), rand(C)
            w2, b2 = torch.cat([wu, wr]).contiguous(), torch.cat([bu, br]).contiguous()

            def two():
                with torch.no_grad():
                    conv.conv_bias_act(x, wu, bu, 1, 1)
                    conv.conv_bias_act(x, wr, br, 1, 1)

            def one():
                with torch.no_grad():
                    conv.conv_bias_act(x, w2, b2, 1, 1)

            (lo2, hi2), (lo1, hi1) = timed(two, iters), timed(one, iters)
            row(row="gates", mode=mode, shape=[B, 2 * C, S, S], two_launches_us=lo2, two_launches_us_max=hi2, one_launch_us=lo1,
                one_launch_us_max=hi1)
        finally:
            conv.set_compute_dtype("fp32")


def bench_step(iters, kernel_size=3):
    from ebfi_amd.unet import UNetFlow
    torch.manual_seed(0)
    net = UNetFlow(dict(base_num_channels=32, num_encoders=3, num_residual_blocks=2, skip_type="sum", norm=None,
                        use_upsample_conv=True, num_bins=5, recurrent_block_type="convlstm", kernel_size=kernel_size)).cuda()
    x, cot = rand(8, 5, 256, 256), rand(8, 3, 256, 256)
    params = list(net.parameters())

    def step():
        net.states = [None] * net.num_encoders
        out = net(x)
        loss = (torch.cat([out["image"], out["flow"]], 1) * cot).sum()
        torch.autograd.grad(loss, params)

    for mode in ("fp32", "bf16x3"):
        conv.set_compute_dtype(mode)
        try:
            lo, hi = timed(step, iters)
        finally:
            conv.set_compute_dtype("fp32")
        row(row="step", net="UNetFlow base 32, 3 encoders, 2 residual blocks, k%d, sum, convlstm" % kernel_size, shape=[8, 5, 256, 256], mode=mode,
            ms_per_step=round(lo / 1e3, 3), ms_per_step_max=round(hi / 1e3, 3), parameters=sum(p.numel() for p in params))


if __name__ == "__main__":
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("iters", type=int, nargs="?", default=100)
    which = ap.add_mutually_exclusive_group()
    which.add_argument("--no-step", action="store_true")
    which.add_argument("--step-only", action="store_true", help="the step rows alone")
    ap.add_argument("--kernel-size", type=int, default=3, help="kernel_size of the step's UNetFlow (3; 5 is the reference's default)")
    a = ap.parse_args()
    assert torch.cuda.is_available(), "recurrentbench needs the MI355X"
    if not a.step_only:
        for S in (64, 128):
            bench_lstm(8, 64, S, a.iters)
            bench_gru(8, 64, S, a.iters)
        bench_bilinear(8, 64, 128, 2, a.iters)
        for S in (64, 128):
            bench_gates(8, 64, S, max(a.iters // 4, 10))
    if not a.no_step:
        bench_step(max(a.iters // 10, 5), a.kernel_size)
