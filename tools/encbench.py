#!/usr/bin/env python3
"""Times of the ordered event scatters (csrc/encodings.hip) at 720x1280 with B = 16: the temporal-bilinear voxel grid of a
uniform event list and of one with a hot pixel, the index build (keys, stable radix sort, run starts) and the accumulation
separately, and PyTorch eager on the same GPU running the same function's torch expressions.

    python tools/encbench.py [--events 1000000] [--hot 0.1] [--iters 50] [--out FILE]

Prints one JSON line per event list (profiles/encodings.md quotes them) and, with --out, writes them to a file.  `call_ms` is
the whole `events_to_voxel_torch` call (device events around it, workspace allocation included, mean over --iters after
warm-up); `index_ms` and `accumulate_ms` are the
library's own event pairs around its launches, from a separate loop (`kernel_ms` lists every launch label).  Bytes the kernels
must move, from the shapes: the index reads 8 bytes of coordinates and writes 4 of key per event, every 8-bit pass reads the
key twice and the permutation once and writes both (20 bytes; the first pass has no permutation to read, 16) plus its
[256][workgroups] table three times, the run starts write 4 bytes per pixel; the accumulation reads 8 bytes of run bounds and
writes 4 per pixel and plane and gathers 20 bytes (permutation entry, stamp, polarity, two coordinates) per event and plane.
`frac_hbm` is those over the time, against 8 TB/s.  The eager figure is OUR restatement of the reference's torch expressions
(one `index_put_(accumulate=True)` per bin: float atomics, so its low bits differ from run to run); `eager_max_abs_diff` is
its distance from the ordered result.  One box's numbers, taken once; there is no earlier implementation and no time bar.
"""
import argparse
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "ebfi-be_amd"))

import torch  # noqa: E402

HBM_PEAK = 8000.0     # GB/s (MI355X_MICROARCH.md)
H, W, B = 720, 1280, 16


def event_list(n, hot, device):
    """Sorted stamps in [0, 1), polarity +-1 scaled by a fractional contrast, uniform coordinates; a share `hot` of the events
    sits on one pixel."""
    g = torch.Generator(device=device).manual_seed(11)
    xs = torch.rand(n, device=device, generator=g) * W
    ys = torch.rand(n, device=device, generator=g) * H
    if hot > 0:
        pick = torch.rand(n, device=device, generator=g) < hot
        xs = torch.where(pick, torch.full_like(xs, 640.5), xs)
        ys = torch.where(pick, torch.full_like(ys, 360.5), ys)
    ts = torch.sort(torch.rand(n, device=device, generator=g)).values
    ps = (torch.randint(0, 2, (n,), device=device, generator=g).float() * 2 - 1) * (0.5 + torch.rand(n, device=device, generator=g))
    return xs, ys, ts, ps


def eager_voxel(xs, ys, ts, ps, bins):
    """The torch expressions of events_to_voxel_torch(temporal_bilinear=True), out-of-place."""
    oob = (xs >= W) | (xs < 0) | (ys >= H) | (ys < 0)
    x = torch.where(oob, torch.zeros_like(xs), xs).long()
    y = torch.where(oob, torch.zeros_like(ys), ys).long()
    dt = ts[-1] - ts[0] + 1e-6
    t_norm = (ts - ts[0]) / dt * (bins - 1)
    out = []
    for bi in range(bins):
        w = ps * torch.clamp(1.0 - torch.abs(t_norm - bi), min=0)
        if bi == 0:
            w = torch.where(oob, torch.zeros_like(w), w)
        img = torch.zeros((H, W), device=xs.device)
        img.index_put_((y, x), w, accumulate=True)
        out.append(img)
    return torch.stack(out)


def timed(fn, iters):
    for _ in range(3):
        fn()
    torch.cuda.synchronize()
    pairs = []
    for _ in range(iters):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record()
        fn()
        b.record()
        pairs.append((a, b))
    torch.cuda.synchronize()
    return sum(a.elapsed_time(b) for a, b in pairs) / iters


def algorithmic_bytes(n, planes):
    pixels = H * W
    passes = ((pixels).bit_length() + 7) // 8
    table = 256 * ((n + 255) // 256) * 4
    index = 12 * n + passes * (20 * n + 3 * table) - 4 * n + 4 * (pixels + 1)
    accumulate = planes * (12 * pixels + 20 * n)
    return index, accumulate


def main(argv=None):
    ap = argparse.ArgumentParser(description=__doc__.split("\n")[0])
    ap.add_argument("--events", type=int, default=1000000)
    ap.add_argument("--hot", type=float, default=0.1, help="share of the events on one pixel in the hot list")
    ap.add_argument("--iters", type=int, default=50)
    ap.add_argument("--out", default=None)
    args = ap.parse_args(argv)
    if not torch.cuda.is_available():
        raise SystemExit("encbench.py measures on an MI355X; no GPU is visible")
    from ebfi_amd import _native as N
    from ebfi_amd.encodings import events_to_voxel_torch
    dev = torch.device("cuda", 0)
    lines = []
    for name, hot in (("uniform", 0.0), ("hot_pixel", args.hot)):
        xs, ys, ts, ps = event_list(args.events, hot, dev)
        ours = lambda: events_to_voxel_torch(xs, ys, ts, ps, B, sensor_size=(H, W))
        iters = args.iters if hot == 0 else max(3, args.iters // 10)     # (the hot pixel's walk is serial: fewer repetitions)
        call_ms = timed(ours, iters)
        N.prof_reset()
        N.prof_enable(True)
        reps = min(iters, 20)
        for _ in range(reps):
            ours()
        torch.cuda.synchronize()
        N.prof_enable(False)
        prof = N.prof_collect()
        kernel_ms = {k: round(v[1] / reps, 4) for k, v in prof.items() if k.startswith("enc_")}
        acc_ms = kernel_ms.get("enc_grid_accumulate", 0.0)
        idx_ms = round(sum(v for k, v in kernel_ms.items() if k != "enc_grid_accumulate"), 4)
        eager_ms = timed(lambda: eager_voxel(xs, ys, ts, ps, B), args.iters)
        diff = float((eager_voxel(xs, ys, ts, ps, B) - ours()).abs().max())
        again = bool(torch.equal(ours(), ours()))
        ib, ab = algorithmic_bytes(args.events, B)
        line = {"op": "events_to_voxel_torch", "list": name, "H": H, "W": W, "B": B, "events": args.events, "hot_share": hot,
                "iters": iters, "call_ms": round(call_ms, 4), "index_ms": idx_ms, "accumulate_ms": acc_ms, "kernel_ms": kernel_ms,
                "index_bytes": ib, "accumulate_bytes": ab,
                "index_GBps": round(ib / idx_ms * 1e-6, 1) if idx_ms else None,
                "accumulate_GBps": round(ab / acc_ms * 1e-6, 1) if acc_ms else None,
                "index_frac_hbm": round(ib / idx_ms * 1e-6 / HBM_PEAK, 4) if idx_ms else None,
                "accumulate_frac_hbm": round(ab / acc_ms * 1e-6 / HBM_PEAK, 4) if acc_ms else None,
                "eager_ms": round(eager_ms, 4), "eager_max_abs_diff": diff, "bit_reproducible": again,
                "device": torch.cuda.get_device_name(0)}
        text = json.dumps(line)
        print(text)
        lines.append(text)
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            f.write("\n".join(lines) + "\n")
    return 0


if __name__ == "__main__":
    sys.exit(main())
