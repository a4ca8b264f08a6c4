#!/usr/bin/env python3
"""The deferred weight-gradient work of one training step (ebfi_amd.wgradqueue), single launches against the batched ones.

One eager step of the default model at B=8 256x256 records what the queue holds at its flush: the geometry of every pure layer
and the index tables of every fold gather.  Two arms then run that work on random operands of those shapes:
  single  per layer ebfi_conv2d_backward_weight_f16g_ex (act none) and per table ebfi_gather_sum -- what the step launches
          without the queue;
  multi   one ebfi_conv2d_backward_weight_f16g_multi and one ebfi_gather_sum_multi.
Each arm is captured into a hipGraph (the step is replayed from one, and a launch costs there what it costs there) and the two
graphs are replayed alternately in one process, timed with event pairs.  Printed: per arm min / mean / max microseconds per
replay over the rounds, the difference, the single arm's max - min spread, and the rows of the library's own event pairs
(one eager pass per arm).
Usage (GPU box): python tools/wgradbench.py [--rounds 20] [--reps 10] [--out FILE.json]"""
import argparse
import ctypes
import json
import os
import sys

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "ebfi-be_amd"))
from ebfi_amd import _native as N  # noqa: E402
from ebfi_amd import wgradqueue  # noqa: E402
from ebfi_amd.engine import DEFAULT_MODEL_ARGS, Engine, synthetic_batch  # noqa: E402


def record_step_work(B, H, W):
    """-> ([(B, Cin, H, W, Cout, has_bias)], [(n_src, inv table, R, n_out)]) of the last flush of three eager steps."""
    seen = {}
    flush = wgradqueue.WgradQueue.flush

    def spy(self):
        layers = [(L[3][0], L[3][1], L[3][2], L[3][3], L[3][4], L[0].has_bias) for L in self.layers]
        gathers = [(g[0].numel(), g[1], g[2], int(torch.Size(g[3]).numel())) for g in self.gathers]
        for L in self.layers:                     # the gathers the queued layers will add at the flush
            s = L[0]
            if s.kind != "id":
                nw = len(s.w_shapes)
                for need, shp, inv, R in zip(L[7][:nw], s.w_shapes, s.w_inv, s.w_R):
                    if need:
                        gathers.append((s.M * s.K * 9, inv, int(R), int(torch.Size(shp).numel())))
                for need, shp, inv, R in zip(L[7][nw:], s.b_shapes, s.b_inv, s.b_R):
                    if need:
                        gathers.append((s.M, inv, int(R), int(torch.Size(shp).numel())))
        seen["layers"], seen["gathers"] = layers, gathers
        return flush(self)

    wgradqueue.WgradQueue.flush = spy
    try:
        eng = Engine(DEFAULT_MODEL_ARGS, device="cuda", precision="bf16x3", graph=False, seed=1)
        batch = synthetic_batch(B, H, W)
        for _ in range(3):
            eng.train_step(*batch)
        torch.cuda.synchronize()
    finally:
        wgradqueue.WgradQueue.flush = flush
    return seen["layers"], seen["gathers"]


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rounds", type=int, default=20)
    ap.add_argument("--reps", type=int, default=10)
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    layers, gathers = record_step_work(8, 256, 256)
    lib = N.lib()
    dev = torch.device("cuda")
    torch.manual_seed(0)
    n = len(layers)
    xs = [torch.randn(B, Cin, H, W, device=dev) for B, Cin, H, W, Cout, hb in layers]
    gs = [torch.randn(B, Cout, H, W, device=dev) for B, Cin, H, W, Cout, hb in layers]
    gws = [torch.empty(Cout, Cin, 3, 3, device=dev) for B, Cin, H, W, Cout, hb in layers]
    gbs = [torch.empty(Cout, device=dev) if hb else None for B, Cin, H, W, Cout, hb in layers]
    slots = torch.zeros(2 * n, 64)
    slots[:, 0] = 1.0
    slots = slots.reshape(-1).to(dev)
    slot = lambda i: ctypes.c_void_p(slots.data_ptr() + 256 * i)
    srcs = [torch.randn(ns, device=dev) for ns, inv, R, no in gathers]
    outs = [torch.empty(no, device=dev) for ns, inv, R, no in gathers]
    needs = [int(lib.ebfi_conv2d_backward_weight_workspace(B, Cin, H, W, Cout, 3, 1, 1, N.EBFI_F32)) for B, Cin, H, W, Cout, hb in layers]
    wss = [torch.empty(max(v, 4), dtype=torch.uint8, device=dev) for v in needs]
    ints = lambda v: (ctypes.c_int * len(v))(*[int(q) for q in v])
    vps = lambda v: (ctypes.c_void_p * len(v))(*v)
    col = lambda i: ints([L[i] for L in layers])
    need_m = int(lib.ebfi_conv2d_backward_weight_f16g_multi_workspace(n, col(0), col(1), col(2), col(3), col(4)))
    ws_m = torch.empty(max(need_m, 4), dtype=torch.uint8, device=dev)

    def single():
        st = N.stream_ptr(dev)
        for k, (B, Cin, H, W, Cout, hb) in enumerate(layers):
            N.check(lib.ebfi_conv2d_backward_weight_f16g_ex(N.ptr(xs[k]), N.ptr(gs[k]), N.ptr(None), N.ptr(gws[k]), N.ptr(gbs[k]), N.ptr(None),
                                                            0, B, Cin, H, W, Cout, 3, 1, 1, 0, 0.0, slot(2 * k), slot(2 * k + 1),
                                                            N.ptr(wss[k]), needs[k], st), "ebfi_conv2d_backward_weight_f16g_ex")
        for (ns, inv, R, no), src, out in zip(gathers, srcs, outs):
            N.check(lib.ebfi_gather_sum(N.ptr(src), N.ptr(inv), N.ptr(out), no, R, st), "ebfi_gather_sum")

    def multi():
        st = N.stream_ptr(dev)
        N.check(lib.ebfi_conv2d_backward_weight_f16g_multi(
            n, vps([t.data_ptr() for t in xs]), vps([t.data_ptr() for t in gs]), vps([t.data_ptr() for t in gws]),
            vps([None if t is None else t.data_ptr() for t in gbs]), col(0), col(1), col(2), col(3), col(4), ints([3] * n), ints([1] * n),
            ints([1] * n), ints([1] * n), vps([slots.data_ptr() + 256 * 2 * k for k in range(n)]),
            vps([slots.data_ptr() + 256 * (2 * k + 1) for k in range(n)]), N.ptr(ws_m), need_m, st), "ebfi_conv2d_backward_weight_f16g_multi")
        m = len(gathers)
        N.check(lib.ebfi_gather_sum_multi(m, vps([t.data_ptr() for t in srcs]), vps([g[1].data_ptr() for g in gathers]),
                                          vps([t.data_ptr() for t in outs]), (ctypes.c_int64 * m)(*[g[3] for g in gathers]),
                                          ints([g[2] for g in gathers]), st), "ebfi_gather_sum_multi")

    rows = {}
    for name, fn in (("single", single), ("multi", multi)):
        fn()
        torch.cuda.synchronize()
        N.prof_reset()
        N.prof_enable(True)
        fn()
        torch.cuda.synchronize()
        N.prof_enable(False)
        rows[name] = {k: {"launches": v[0], "total_us": round(1e3 * v[1], 2)} for k, v in N.prof_collect().items() if v[0] > 0}
    graphs = {}
    for name, fn in (("single", single), ("multi", multi)):
        side = torch.cuda.Stream(dev)
        side.wait_stream(torch.cuda.current_stream(dev))
        with torch.cuda.stream(side):
            fn()
        torch.cuda.current_stream(dev).wait_stream(side)
        g = torch.cuda.CUDAGraph()
        with torch.cuda.graph(g):
            fn()
        graphs[name] = g
    times = {"single": [], "multi": []}
    for name in graphs:
        for _ in range(3):
            graphs[name].replay()
    torch.cuda.synchronize()
    for _ in range(a.rounds):
        for name in ("single", "multi"):
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record()
            for _ in range(a.reps):
                graphs[name].replay()
            e1.record()
            torch.cuda.synchronize()
            times[name].append(1e3 * e0.elapsed_time(e1) / a.reps)
    stat = lambda v: {"min_us": round(min(v), 2), "mean_us": round(sum(v) / len(v), 2), "max_us": round(max(v), 2)}
    res = {"layers": [list(L) for L in layers], "gathers": [[g[0], g[2], g[3]] for g in gathers],
           "launches": {"single": 2 * n + len(gathers), "multi": 2 * ((n + 15) // 16) + (len(gathers) + 47) // 48},
           "single": stat(times["single"]), "multi": stat(times["multi"]), "event_pair_rows": rows}
    res["gain_us"] = round(res["single"]["mean_us"] - res["multi"]["mean_us"], 2)
    res["single_spread_us"] = round(res["single"]["max_us"] - res["single"]["min_us"], 2)
    res["multi_is_faster_beyond_the_spread"] = bool(res["gain_us"] > res["single_spread_us"])
    txt = json.dumps(res)
    print(txt)
    if a.out:
        with open(a.out, "w") as f:
            f.write(txt + "\n")


if __name__ == "__main__":
    main()
