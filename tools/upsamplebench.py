#!/usr/bin/env python3
"""Cost of the frame-upsampling step (ebfi_amd.upsample) at 704x1280 -- 720p after the crop to multiples of 32 -- with seeded
weights: device time of one flow pass (flow network + flow maximum) and of one intermediate frame (assembly, interpolation
network, blend), per kernel from the library's own event pairs, and, in the same call and alternating with the native passes,
the same restated network (tests/upsample_ref.py in float32) in plain PyTorch-ROCm eager as the yardstick.

    python tools/upsamplebench.py [--iters 10] [--warmup 3] [--no-eager] [--height 704 --width 1280] [--out profiles/upsample.md]

Prints one JSON line and rewrites the part of --out between the `upsamplebench` markers (the rest of the file is kept).
Algorithmic FLOPs and bytes are what every launch records from its shapes (each operand once, results once).  `share` of a
kernel is the least time the hardware could take over the measured time: the larger of FLOPs over the matrix peak (157.3 TFLOP/s
for the exact-fp32 kernels; a third of 16 x 157.3 for the split-precision ones, which spend three bf16 products per product)
and bytes over 8 TB/s; `bound` says which of the two it was.  One box, one run: a measurement, not a bar.
"""
import argparse
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for p in (os.path.join(ROOT, "tests"), os.path.join(ROOT, "ebfi-be_amd"), ROOT):
    sys.path.insert(0, p)

import torch  # noqa: E402

HBM_PEAK = 8.0e12
F32_MFMA_PEAK = 157.3e12
X3_PEAK = 16 * F32_MFMA_PEAK / 3
BEGIN, END = "<!-- upsamplebench:begin -->", "<!-- upsamplebench:end -->"


def timed(fn, start, stop):
    start.record()
    fn()
    stop.record()


def mean_ms(pairs):
    return sum(a.elapsed_time(b) for a, b in pairs) / len(pairs)


def spread_ms(pairs):
    v = [a.elapsed_time(b) for a, b in pairs]
    return min(v), max(v)


def kernel_rows(prof, passes):
    rows = []
    for name, (n, ms, flops, nbytes) in sorted(prof.items(), key=lambda kv: -kv[1][1]):
        if name.startswith("__") or n == 0:
            continue
        peak = X3_PEAK if "bf16x3" in name else F32_MFMA_PEAK
        t_flops, t_bytes = flops / peak * 1e3, nbytes / HBM_PEAK * 1e3
        least = max(t_flops, t_bytes)
        rows.append(dict(kernel=name, launches_per_pass=n / passes, ms_per_pass=ms / passes, gflop_per_pass=flops / passes / 1e9,
                         mbyte_per_pass=nbytes / passes / 1e6, bound="matrix" if t_flops >= t_bytes else "hbm",
                         share=(least / ms) if ms > 0 else None))
    return rows


def table(rows):
    out = ["| kernel | launches | ms | GFLOP | MB | bound | share of bound |", "|---|---|---|---|---|---|---|"]
    for r in rows:
        out.append("| `%s` | %g | %.3f | %.2f | %.1f | %s | %s |" % (
            r["kernel"], r["launches_per_pass"], r["ms_per_pass"], r["gflop_per_pass"], r["mbyte_per_pass"], r["bound"],
            "%.1f %%" % (100 * r["share"]) if r["share"] is not None else "-"))
    return "\n".join(out)


def main(argv=None):
    ap = argparse.ArgumentParser(description=__doc__.split("\n")[0])
    ap.add_argument("--iters", type=int, default=10)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--height", type=int, default=704)
    ap.add_argument("--width", type=int, default=1280)
    ap.add_argument("--no-eager", action="store_true", help="skip the PyTorch eager yardstick")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "upsample.md"))
    args = ap.parse_args(argv)
    if not torch.cuda.is_available():
        raise SystemExit("upsamplebench.py measures on an MI355X; no GPU is visible")
    import upsample_ref as R
    from ebfi_amd import _native as N
    from ebfi_amd.upsample import Upsampler
    dev = torch.device("cuda", 0)
    H, W = args.height, args.width
    sd_fc, sd_at = R.flow_state_dict(), R.interp_state_dict()
    up = Upsampler.from_state_dicts(dev, sd_fc, sd_at)
    g = torch.Generator().manual_seed(3)
    I0 = (torch.rand((3, H, W), generator=g) * 1.03 - 0.43).to(dev)
    I1 = (torch.rand((3, H, W), generator=g) * 1.03 - 0.43).to(dev)
    b = up._bufs(H, W)
    b["x6"][:3].copy_(I0)
    b["x6"][3:].copy_(I1)
    lib, st, t = N.lib(), N.stream_ptr(dev), 0.5
    gray = torch.empty((H, W), dtype=torch.uint8, device=dev)

    def flow_pass():
        flow = up.flowComp(b["x6"])
        N.check(lib.ebfi_flow_max_magnitude(N.ptr(flow), H, W, N.ptr(b["max"]), st), "flow_max")
        return flow

    flow = flow_pass().clone()

    def frame_pass():
        N.check(lib.ebfi_slomo_assemble(N.ptr(b["x6"][:3]), N.ptr(b["x6"][3:]), N.ptr(flow), t, N.ptr(b["x20"]), H, W, st), "assemble")
        intrp = up.ArbTimeFlowIntrp(b["x20"])
        N.check(lib.ebfi_slomo_blend(N.ptr(intrp), N.ptr(b["x20"]), t, N.ptr(None), N.ptr(gray), H, W, st), "blend")

    eager = None
    if not args.no_eager:
        e_fc = {k: v.to(dev) for k, v in sd_fc.items()}
        e_at = {k: v.to(dev) for k, v in sd_at.items()}
        x6 = b["x6"][None].clone()

        def eager_flow():
            with torch.no_grad():
                fo = R.unet_forward(e_fc, x6, torch.float32)
                return fo, torch.max(fo[:, :2].pow(2).sum(1).pow(0.5).max(), fo[:, 2:].pow(2).sum(1).pow(0.5).max())

        e_flow = eager_flow()[0]

        def eager_frame():
            with torch.no_grad():
                x20 = R.assemble(x6[:, :3], x6[:, 3:], e_flow, t)
                return R.blend(R.unet_forward(e_at, x20, torch.float32), x20, t)

        eager = (eager_flow, eager_frame)
        print("eager yardstick built (its first passes choose and build library kernels)", flush=True)

    ev = lambda: torch.cuda.Event(enable_timing=True)
    series = {"flow_ms": [], "frame_ms": [], "eager_flow_ms": [], "eager_frame_ms": []}
    for i in range(args.warmup + args.iters):
        keep = i >= args.warmup
        todo = [("flow_ms", flow_pass), ("frame_ms", frame_pass)]
        if eager:
            todo = [todo[0], ("eager_flow_ms", eager[0]), todo[1], ("eager_frame_ms", eager[1])]       # alternating
        for key, fn in todo:
            a, z = ev(), ev()
            timed(fn, a, z)
            if keep:
                series[key].append((a, z))
        torch.cuda.synchronize()
        print("pass %d of %d done" % (i + 1, args.warmup + args.iters), flush=True)
    res = dict(H=H, W=W, iters=args.iters, warmup=args.warmup)
    for key, pairs in series.items():
        if pairs:
            lo, hi = spread_ms(pairs)
            res[key] = round(mean_ms(pairs), 4)
            res[key.replace("_ms", "_min_max_ms")] = [round(lo, 4), round(hi, 4)]

    # per kernel: the library's own event pair around every launch, in loops of their own
    per_kernel = {}
    for key, fn in (("flow", flow_pass), ("frame", frame_pass)):
        N.prof_reset()
        N.prof_enable(True)
        for _ in range(args.iters):
            fn()
            torch.cuda.synchronize()
            N.prof_fold()
        torch.cuda.synchronize()
        prof = N.prof_collect()
        N.prof_enable(False)
        per_kernel[key] = kernel_rows(prof, args.iters)
        res[key + "_gflop"] = round(sum(r["gflop_per_pass"] for r in per_kernel[key]), 2)
        res[key + "_algorithmic_mbyte"] = round(sum(r["mbyte_per_pass"] for r in per_kernel[key]), 1)
        res[key + "_kernel_ms_sum"] = round(sum(r["ms_per_pass"] for r in per_kernel[key]), 4)
    res["kernels"] = per_kernel
    line = json.dumps(res)
    print(line)

    head = {k: v for k, v in res.items() if k != "kernels"}
    text = [BEGIN, "", "Command: `python tools/upsamplebench.py%s` (%d x %d, seeded weights, t = 0.5; device events, mean of %d passes "
            "after %d warm-up passes; native and eager passes alternate inside one loop)." % (" --no-eager" if args.no_eager else "", H, W,
                                                                                           args.iters, args.warmup), "",
            "```json", json.dumps(head), "```", ""]
    for key, title in (("flow", "One flow pass (flow network + flow maximum)"), ("frame", "One intermediate frame (assembly, interpolation network, blend)")):
        text += ["### %s, per kernel" % title, "", table(per_kernel[key]), ""]
    text += [END]
    old = open(args.out).read() if os.path.exists(args.out) else "# Frame upsampling (`ebfi_amd/upsample.py`, `csrc/upsample.hip`): measurements\n\n%s\n%s\n" % (BEGIN, END)
    if BEGIN in old and END in old:
        new = old[:old.index(BEGIN)] + "\n".join(text) + old[old.index(END) + len(END):]
    else:
        new = old.rstrip("\n") + "\n\n" + "\n".join(text) + "\n"
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as f:
        f.write(new)
    return 0


if __name__ == "__main__":
    sys.exit(main())
