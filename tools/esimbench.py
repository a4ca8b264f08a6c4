#!/usr/bin/env python3
"""Throughput of the event simulator (csrc/esim.hip) at 720x1280: the count and the emit pass over a chunk of frame intervals,
timed with device events around the two launches (the state is restored between repetitions, outside the timed window), and
the whole `EventSimulator.generate` call (both passes, the prefix sum, the two stable sorts and the event-count read-back) with a
host clock that ends in a device synchronise.

    python tools/esimbench.py [--iters 400] [--chunk 16] [--out profiles/esim.md]

Prints one JSON line and writes it, with a short legend, to --out.  Algorithmic bytes per repetition: every frame byte once per
pass, 4 bytes of count and 8 of offset per pixel and interval, the 24-byte state read twice and written once, 13 bytes per
event; `frac_hbm` is that over the time, against 8 TB/s (MI355X_MICROARCH.md).  There is no earlier implementation to compare
with: the line is one box's measurement, not a bar.
"""
import argparse
import ctypes
import json
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "ebfi-be_amd"))

import torch  # noqa: E402

HBM_PEAK = 8000.0     # GB/s (MI355X_MICROARCH.md)
H, W = 720, 1280
PARAMS = dict(Cp=0.35, Cn=0.3, refractory_period=1e-4, log_eps=1e-3, use_log=True)

LEGEND = """# Event simulator (`csrc/esim.hip`): measurement

Command: `python tools/esimbench.py` (720x1280, a drifting sinusoid with sensor noise, 240 frames/s).  One JSON line:
`count_emit_ms` is the device time of the count and the emit launch over one chunk of `intervals` frame intervals (device events,
mean of `iters` repetitions), `frames_per_s` and `events_per_s` follow from it, `algorithmic_bytes` is what the two passes must
move (frames twice, counts, offsets, the state read twice and written once, 13 bytes per event), `GBps` and `frac_hbm` (of
8 TB/s) are that over the time; `kernel_ms` is the library's own event pair around each launch, from a separate loop.
`generate_ms` is the whole `EventSimulator.generate` call on the same chunk: both passes, the prefix sum, the two stable sorts
(by pixel, by t) and the read-back of the event count, host clock ending in a synchronise.

This is one box's number, taken once; there is no earlier implementation and no time bar.  At the default chunk of 16
intervals the two passes touch about 280 MB, the size of the 256 MB Infinity Cache, and every repetition walks the same chunk:
part of the traffic is served from that cache, so `GBps` is a rate of the algorithm's bytes, not of HBM traffic.

"""


def make_frames(n, device):
    """uint8 [n, H, W]: a sinusoid drifting four pixels a frame, plus noise of three gray levels."""
    g = torch.Generator(device=device).manual_seed(7)
    y = torch.arange(H, device=device, dtype=torch.float32)[None, :, None]
    x = torch.arange(W, device=device, dtype=torch.float32)[None, None, :]
    k = torch.arange(n, device=device, dtype=torch.float32)[:, None, None]
    v = 127.0 + 100.0 * torch.sin((x + 4.0 * k) / 37.0) * torch.cos((y + 2.0 * k) / 29.0)
    v = v + 3.0 * torch.randn((n, H, W), device=device, generator=g)
    return v.clamp(0, 255).to(torch.uint8)


def main(argv=None):
    ap = argparse.ArgumentParser(description=__doc__.split("\n")[0])
    ap.add_argument("--iters", type=int, default=400)
    ap.add_argument("--chunk", type=int, default=16, help="frame intervals per chunk (at most 128)")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "esim.md"))
    args = ap.parse_args(argv)
    if not torch.cuda.is_available():
        raise SystemExit("esimbench.py measures on an MI355X; no GPU is visible")
    from ebfi_amd import _native as N
    from ebfi_amd.esim import EventSimulator
    dev = torch.device("cuda", 0)
    n = args.chunk
    frames = make_frames(n + 1, dev)
    times = [k / 240.0 for k in range(n + 1)]

    sim = EventSimulator(**PARAMS)
    sim.generate(frames[:1], times[:1])
    state0 = sim._state.clone()
    state = sim._state
    h = N.lib()
    stream = N.stream_ptr(dev)
    t_c = (ctypes.c_double * (n + 1))(*times)
    strides = (ctypes.c_int64 * 2)(int(frames.stride(0)), int(frames.stride(1)))
    walk = (N.ptr(frames[1:]), strides, 0, n, H, W, t_c, sim._levels_c, sim.Cp, sim.Cn, sim.refractory_period)
    counts = torch.empty((n, H, W), dtype=torch.int32, device=dev)
    N.check(h.ebfi_esim_count(*walk, N.ptr(state), N.ptr(counts), stream), "ebfi_esim_count")
    ends = torch.cumsum(counts.view(-1), 0, dtype=torch.int64)
    total = int(ends[-1].item())
    offsets = ends - counts.view(-1)
    xs = torch.empty(total, dtype=torch.int16, device=dev)
    ys = torch.empty(total, dtype=torch.int16, device=dev)
    ts = torch.empty(total, dtype=torch.float64, device=dev)
    ps = torch.empty(total, dtype=torch.int8, device=dev)

    def both():
        N.check(h.ebfi_esim_count(*walk, N.ptr(state), N.ptr(counts), stream), "ebfi_esim_count")
        N.check(h.ebfi_esim_emit(*walk, N.ptr(state), N.ptr(offsets), total, N.ptr(xs), N.ptr(ys), N.ptr(ts), N.ptr(ps), stream),
                "ebfi_esim_emit")

    for _ in range(3):
        state.copy_(state0)
        both()
    pairs = []
    for _ in range(args.iters):
        state.copy_(state0)          # (outside the timed window: every repetition walks the same chunk from the same state)
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record()
        both()
        b.record()
        pairs.append((a, b))
    torch.cuda.synchronize()
    ms = sum(a.elapsed_time(b) for a, b in pairs) / args.iters

    # the library's own event pair around each launch, in a run of its own
    N.prof_reset()
    N.prof_enable(True)
    for _ in range(min(args.iters, 100)):
        state.copy_(state0)
        both()
    torch.cuda.synchronize()
    N.prof_enable(False)
    prof = N.prof_collect()
    kernel_ms = {k: round(v[1] / max(v[0], 1), 4) for k, v in prof.items() if k.startswith("esim_walk")}

    def generate():
        sim.reset()
        sim.generate(frames, times, chunk=n)

    for _ in range(2):
        generate()
    torch.cuda.synchronize()
    reps = max(3, args.iters // 4)
    t0 = time.perf_counter()
    for _ in range(reps):
        generate()
    torch.cuda.synchronize()
    gen_ms = (time.perf_counter() - t0) * 1e3 / reps

    hw = H * W
    nbytes = 2 * n * hw + 4 * n * hw + 8 * n * hw + 3 * 24 * hw + 13 * total
    line = {"op": "esim_count_emit", "H": H, "W": W, "intervals": n, "iters": args.iters, "events": total,
            "count_emit_ms": round(ms, 4), "frames_per_s": round(n / ms * 1e3, 1), "events_per_s": round(total / ms * 1e3, 1),
            "algorithmic_bytes": nbytes, "GBps": round(nbytes / ms * 1e-6, 1), "frac_hbm": round(nbytes / ms * 1e-6 / HBM_PEAK, 4),
            "kernel_ms": kernel_ms, "generate_ms": round(gen_ms, 3), "device": torch.cuda.get_device_name(0)}
    text = json.dumps(line)
    print(text)
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as f:
        f.write(LEGEND + "```\n" + text + "\n```\n")
    return 0


if __name__ == "__main__":
    sys.exit(main())
