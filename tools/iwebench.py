#!/usr/bin/env python3
"""Times of the device warping losses (csrc/iwe.hip) at B = 8, 256 x 256: the fused EventWarping loss forward plus backward
and AveragedIWE, at 2^17 and 2^20 events per item with uniform source pixels, and one row with every event on one pixel.
The baseline is PyTorch eager on the same GPU running the torch restatement of tests/iwe_ref.py (scatter_add with float
atomics: its low bits change from run to run).

    python tools/iwebench.py [--iters 10] [--out FILE]

Prints one JSON line per row (profiles/iwe.md quotes them).  `*_ms`: device events around the whole call, workspace
allocation included, mean over --iters after warm-up.  `kernel_ms`: the library's own event pairs per launch label, from a
separate loop.  `eager_*_diff`: distance of the eager result from the ordered one; `bit_reproducible`: two calls of ours
compared bit for bit.  One box's numbers, taken once; there is no earlier implementation and no time bar.
"""
import argparse
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "ebfi-be_amd"))
sys.path.insert(0, os.path.join(ROOT, "tests"))

import torch  # noqa: E402

B, H, W = 8, 256, 256
WEIGHT = 0.001


def inputs(n, one_pixel, device):
    g = torch.Generator(device=device).manual_seed(7)
    ev = torch.empty((B, n, 4), device=device)
    ev[:, :, 0] = torch.rand((B, n), device=device, generator=g)
    if one_pixel:
        ev[:, :, 1], ev[:, :, 2] = 100.0, 57.0
    else:
        ev[:, :, 1] = torch.randint(0, H, (B, n), device=device, generator=g).float()
        ev[:, :, 2] = torch.randint(0, W, (B, n), device=device, generator=g).float()
    ev[:, :, 3] = torch.randint(0, 2, (B, n), device=device, generator=g).float() * 2 - 1
    pm = torch.stack([(ev[:, :, 3] > 0).float(), (ev[:, :, 3] < 0).float()], dim=2)
    flow = (torch.rand((B, 2, H, W), device=device, generator=g) - 0.5) * 0.02      # up to 2.5 pixels at scaling 256
    return ev, pm, flow


def timed(fn, iters):
    for _ in range(2):
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


def main(argv=None):
    ap = argparse.ArgumentParser(description=__doc__.split("\n")[0])
    ap.add_argument("--iters", type=int, default=10)
    ap.add_argument("--out", default=None)
    args = ap.parse_args(argv)
    if not torch.cuda.is_available():
        raise SystemExit("iwebench.py measures on an MI355X; no GPU is visible")
    import iwe_ref as R
    from ebfi_amd import _native as N
    from ebfi_amd.iwe import AveragedIWE, EventWarping
    dev = torch.device("cuda", 0)
    config = {"loss": {"flow_regul_weight": WEIGHT}, "loader": {"resolution": [H, W], "batch_size": B}}
    loss_fn, avg_fn = EventWarping(config, dev), AveragedIWE(config, dev)
    lines = []
    for name, n, one_pixel in (("uniform", 1 << 17, False), ("uniform", 1 << 20, False), ("one_pixel", 1 << 17, True)):
        ev, pm, flow = inputs(n, one_pixel, dev)
        flow.requires_grad_(True)

        def ours():
            loss = loss_fn([flow], ev, pm, (H, W))
            return loss.detach(), torch.autograd.grad(loss, flow)[0]

        def eager():
            loss = R.t_event_warping([flow], ev, pm, (H, W), WEIGHT)
            return loss.detach(), torch.autograd.grad(loss, flow)[0]

        ours_avg = lambda: avg_fn(flow.detach(), ev, pm)
        eager_avg = lambda: R.t_averaged_iwe(flow.detach(), ev, pm, (H, W))
        fwd_ms = timed(lambda: loss_fn([flow.detach()], ev, pm, (H, W)), args.iters)
        both_ms = timed(ours, args.iters)
        avg_ms = timed(ours_avg, args.iters)
        N.prof_reset()
        N.prof_enable(True)
        reps = min(args.iters, 5)
        for _ in range(reps):
            ours()
            ours_avg()
        torch.cuda.synchronize()
        N.prof_enable(False)
        kernel_ms = {k: round(v[1] / reps, 4) for k, v in N.prof_collect().items() if k.startswith("iwe_")}
        eager_ms = timed(eager, args.iters)
        eager_avg_ms = timed(eager_avg, args.iters)
        (l1, g1), (l2, g2), (le, ge) = ours(), ours(), eager()
        a1, a2, ae = ours_avg(), ours_avg(), eager_avg()
        line = {"op": "EventWarping fwd+bwd / AveragedIWE", "list": name, "B": B, "H": H, "W": W, "events_per_item": n,
                "iters": args.iters, "forward_ms": round(fwd_ms, 4), "forward_backward_ms": round(both_ms, 4),
                "averaged_ms": round(avg_ms, 4), "kernel_ms": kernel_ms, "eager_forward_backward_ms": round(eager_ms, 4),
                "eager_averaged_ms": round(eager_avg_ms, 4),
                "eager_loss_rel_diff": abs(float(le) - float(l1)) / abs(float(l1)),
                "eager_grad_diff_of_max": float((ge - g1).abs().max() / g1.abs().max()),
                "eager_averaged_max_abs_diff": float((ae - a1).abs().max()),
                "bit_reproducible": bool(torch.equal(l1, l2) and torch.equal(g1, g2) and torch.equal(a1, a2)),
                "device": torch.cuda.get_device_name(0)}
        text = json.dumps(line)
        print(text, flush=True)
        lines.append(text)
        del ev, pm, flow
        torch.cuda.empty_cache()
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            f.write("\n".join(lines) + "\n")
    return 0


if __name__ == "__main__":
    sys.exit(main())
