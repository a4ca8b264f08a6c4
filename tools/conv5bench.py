#!/usr/bin/env python3
"""The 5x5 convolution kernels (ebfi_conv5x5_* of include/ebfi_hip.h, csrc/conv2d.hip) timed on the device.  One JSON line per
row:

  layer      the seven 5x5 layers of a UNetFlow with base 32 and three encoders at 8 x 5 x 256 x 256 (head, three stride-2
             encoders, three decoders behind the x2 up-sampling; ReLU, bias): the native forward, data gradient (on
             grad_output * act', as the training step runs it) and weight + bias gradient (with the grad * act' side output)
             through the C ABI, each beside the same operation in PyTorch eager on the same GPU -- F.conv2d + relu under
             no_grad, torch.nn.grad.conv2d_input / conv2d_weight on the masked gradient; the bias sum is not in eager's weight
             figure.  Eager is timed after its own warm-up, so MIOpen's find / compile is not in the number.
             Microseconds per call and the dense fp32 TFLOP/s (2 * B * Ho * Wo * Cout * Cin * 25 per operation).
  parity     the three encoder shapes: the stride-2 data gradient by output parity beside the zero-inserted route through
             the new entry point (memset of the [B, Cout, H + 2 pad - 4, W + 2 pad - 4] map, strided scatter of the gradient,
             stride-1 data gradient on it).

Device events around `iters` back-to-back calls after a warm-up; three windows, the best and the worst.

usage: python tools/conv5bench.py [iters] [--layers 0,1,..] [--no-parity]     (--layers: indices into LAYERS, default all)"""
import argparse
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "ebfi-be_amd"))
import torch  # noqa: E402
import torch.nn.functional as F  # noqa: E402

from ebfi_amd import _native as N  # noqa: E402

# (name, Cin, H = W of the layer's input, Cout, stride): UNetFlow base 32, 3 encoders, skip "sum", 256 x 256 input
LAYERS = [("head 5->32", 5, 256, 32, 1),
          ("encoder0 32->64 s2", 32, 256, 64, 2), ("encoder1 64->128 s2", 64, 128, 128, 2), ("encoder2 128->256 s2", 128, 64, 256, 2),
          ("decoder0 256->128", 256, 64, 128, 1), ("decoder1 128->64", 128, 128, 64, 1), ("decoder2 64->32", 64, 256, 32, 1)]
B, PAD = 8, 2


def timed(call, iters, warm=5):
    for _ in range(warm):
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


def row(**kw):
    print(json.dumps(kw), flush=True)


def tensors(Cin, S, Cout, stride):
    So = (S + 2 * PAD - 5) // stride + 1
    x = torch.randn(B, Cin, S, S, device="cuda")
    w = torch.randn(Cout, Cin, 5, 5, device="cuda") / (Cin * 25) ** 0.5
    b = torch.randn(Cout, device="cuda") * 0.1
    g = torch.randn(B, Cout, So, So, device="cuda")
    return x, w, b, g, So


def bench_layer(name, Cin, S, Cout, stride, iters):
    lib, st = N.lib(), N.stream_ptr()
    x, w, b, g, So = tensors(Cin, S, Cout, stride)
    geo = (B, Cin, S, S, Cout, stride, PAD)
    y, gx, gw, gb, gpre = torch.empty_like(g), torch.empty_like(x), torch.empty_like(w), torch.empty_like(b), torch.empty_like(g)
    need = int(lib.ebfi_conv5x5_backward_weight_workspace(*geo))
    ws = torch.empty(need, dtype=torch.uint8, device="cuda")
    fwd = lambda: N.check(lib.ebfi_conv5x5_forward(N.ptr(x), N.ptr(w), N.ptr(b), N.ptr(y), *geo, 1, 0.0, st), "forward")
    wgr = lambda: N.check(lib.ebfi_conv5x5_backward_weight(N.ptr(x), N.ptr(g), N.ptr(y), N.ptr(gw), N.ptr(gb), N.ptr(gpre), *geo, 1, 0.0,
                                                           N.ptr(ws), need, st), "backward_weight")
    dgr = lambda: N.check(lib.ebfi_conv5x5_backward_data(N.ptr(gpre), N.ptr(None), N.ptr(w), N.ptr(gx), *geo, 0, 0.0, st), "backward_data")
    fwd()
    wgr()

    def eager_fwd():
        with torch.no_grad():
            F.relu(F.conv2d(x, w, b, stride, PAD))

    gm = g * (y > 0)
    eager_dgr = lambda: torch.nn.grad.conv2d_input(x.shape, w, gm, stride=stride, padding=PAD)
    eager_wgr = lambda: torch.nn.grad.conv2d_weight(x, w.shape, gm, stride=stride, padding=PAD)
    flop = 2.0 * B * So * So * Cout * Cin * 25
    for op, native, eager in (("forward", fwd, eager_fwd), ("data gradient", dgr, eager_dgr), ("weight gradient", wgr, eager_wgr)):
        (elo, ehi) = timed(eager, iters, warm=8)
        (lo, hi) = timed(native, iters)
        row(row="layer", layer=name, op=op, shape=[B, Cin, S, S], cout=Cout, stride=stride, native_us=lo, native_us_max=hi,
            eager_us=elo, eager_us_max=ehi, speedup=round(elo / lo, 2), gflop=round(flop / 1e9, 2),
            native_tflops=round(flop / lo / 1e6, 1), eager_tflops=round(flop / elo / 1e6, 1))


def bench_parity(name, Cin, S, Cout, iters):
    lib, st = N.lib(), N.stream_ptr()
    x, w, b, g, So = tensors(Cin, S, Cout, 2)
    geo2, gx = (B, Cin, S, S, Cout, 2, PAD), torch.empty_like(x)
    U = S + 2 * PAD - 4                                  # the zero-inserted map: a stride-1 layer's output on the same input
    geo1 = (B, Cin, S, S, Cout, 1, PAD)
    parity = lambda: N.check(lib.ebfi_conv5x5_backward_data(N.ptr(g), N.ptr(None), N.ptr(w), N.ptr(gx), *geo2, 0, 0.0, st), "parity")

    def zero_inserted():
        up = g.new_zeros((B, Cout, U, U))
        up[:, :, ::2, ::2][:, :, :So, :So] = g
        N.check(lib.ebfi_conv5x5_backward_data(N.ptr(up), N.ptr(None), N.ptr(w), N.ptr(gx), *geo1, 0, 0.0, st), "zero-inserted")

    parity()
    a = gx.clone()
    zero_inserted()
    err = float((a - gx).abs().max() / gx.abs().max())
    (lo, hi), (zlo, zhi) = timed(parity, iters), timed(zero_inserted, iters)
    flop = 2.0 * B * So * So * Cout * Cin * 25
    row(row="parity", layer=name, shape=[B, Cin, S, S], cout=Cout, parity_us=lo, parity_us_max=hi, zero_inserted_us=zlo,
        zero_inserted_us_max=zhi, speedup=round(zlo / lo, 2), gflop=round(flop / 1e9, 2), parity_tflops=round(flop / lo / 1e6, 1),
        max_rel_difference=err)


if __name__ == "__main__":
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("iters", type=int, nargs="?", default=20)
    ap.add_argument("--layers", default=",".join(str(i) for i in range(len(LAYERS))))
    ap.add_argument("--no-parity", action="store_true")
    a = ap.parse_args()
    assert torch.cuda.is_available(), "conv5bench needs the MI355X"
    chosen = [LAYERS[int(i)] for i in a.layers.split(",") if i != ""]
    for layer in chosen:
        bench_layer(*layer, a.iters)
    for name, Cin, S, Cout, stride in chosen:
        if stride == 2 and not a.no_parity:
            bench_parity(name, Cin, S, Cout, a.iters)
