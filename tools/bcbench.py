#!/usr/bin/env python3
"""Times of the device reconstruction loss (csrc/bcloss.hip) at B = 8, 256 x 256, 2^17 events per item and flows within
+-0.01 (2.6 pixels): forward and forward plus backward of BrightnessConstancy's three terms, and one row with every pixel
sampling one 2 x 2 footprint (the ordered scatter's worst case).  The baseline is PyTorch eager on the same GPU running the
torch restatement of tests/bc_ref.py (grid_sample; its image gradient is a scatter with float atomics).

    python tools/bcbench.py [--iters 10] [--out FILE]

Prints one JSON line per row (profiles/bcloss.md quotes them).  `*_ms`: device events around the whole call, workspace
allocation included, mean over --iters after warm-up; both sides get the averaged image of warped events handed in, except
`generative_with_iwe_*`, which is the public method (masked flow, AveragedIWE, then the term).  `kernel_ms`: the library's own
event pairs per launch label, from a separate loop.  `*_bit_reproducible`: two calls compared bit for bit, per side.
`eager_*_diff`: distance of the eager result from the ordered one; `eager_*_grad_elements_off`: how many gradient elements
carry it.  One box's numbers, taken once; no time bar.
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
N_EVENTS = 1 << 17
WEIGHTS = [0.1, 0.5]


def inputs(pile, device):
    g = torch.Generator(device=device).manual_seed(7)
    rand = lambda *s: torch.rand(s, device=device, generator=g)
    ev = torch.empty((B, N_EVENTS, 4), device=device)
    ev[:, :, 0] = rand(B, N_EVENTS)
    ev[:, :, 1] = torch.randint(0, H, (B, N_EVENTS), device=device, generator=g).float()
    ev[:, :, 2] = torch.randint(0, W, (B, N_EVENTS), device=device, generator=g).float()
    ev[:, :, 3] = torch.randint(0, 2, (B, N_EVENTS), device=device, generator=g).float() * 2 - 1
    pm = torch.stack([(ev[:, :, 3] > 0).float(), (ev[:, :, 3] < 0).float()], dim=2)
    cnt = torch.randint(0, 3, (B, 2, H, W), device=device, generator=g).float()
    if pile:                                                   # every sample into the cell of (100.x, 57.x)
        cnt += 1
        ix, iy = 100.1 + 0.8 * rand(B, H, W), 57.1 + 0.8 * rand(B, H, W)
        col = torch.arange(W, device=device)[None, None, :].float()
        row = torch.arange(H, device=device)[None, :, None].float()
        flow = torch.stack([(col - (ix + 0.5) * (W - 1) / W) / max(H, W), (row - (iy + 0.5) * (H - 1) / H) / max(H, W)], dim=1)
    else:
        flow = (rand(B, 2, H, W) - 0.5) * 0.02
    return dict(flow=flow.contiguous(), img=rand(B, 1, H, W), prev=rand(B, 1, H, W), cnt=cnt, ev=ev, pm=pm)


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
    return round(sum(a.elapsed_time(b) for a, b in pairs) / iters, 4)


def same(a, b):
    return all(torch.equal(x, y) for x, y in zip(a, b))


def main(argv=None):
    ap = argparse.ArgumentParser(description=__doc__.split("\n")[0])
    ap.add_argument("--iters", type=int, default=10)
    ap.add_argument("--out", default=None)
    args = ap.parse_args(argv)
    if not torch.cuda.is_available():
        raise SystemExit("bcbench.py measures on an MI355X; no GPU is visible")
    import bc_ref as R
    from ebfi_amd import _native as N
    from ebfi_amd import bcloss
    dev = torch.device("cuda", 0)
    config = {"loss": {"reconstruction_regul_weight": WEIGHTS}, "loader": {"resolution": [H, W], "batch_size": B}}
    bc = bcloss.BrightnessConstancy(config, dev)
    lines = []
    for name, pile in (("uniform", False), ("pile", True)):
        t = inputs(pile, dev)
        leaf = {k: t[k].clone().requires_grad_(True) for k in ("flow", "img", "prev")}
        s = t["cnt"].sum(dim=1, keepdim=True)
        avg = bc.averaged_iwe(t["flow"] * torch.where(s > 0, torch.ones_like(s), s), t["ev"], t["pm"])
        dict_in = {"inp_cnt": t["cnt"], "inp_list": t["ev"], "inp_pol_mask": t["pm"]}
        gen_fn = lambda flow, img: bcloss._Generative.apply(flow, img, t["cnt"], avg, max(H, W))
        ours = {
            "generative": (lambda f, i, p: gen_fn(f, i), ("flow", "img")),
            "generative_with_iwe": (lambda f, i, p: bc.generative_model(f, i, dict_in), ("flow", "img")),
            "temporal": (lambda f, i, p: bc.temporal_consistency(f, p, i), ("flow", "prev", "img")),
            "regularization": (lambda f, i, p: bc.regularization(i), ("img",)),
        }
        eager = {
            "generative": (lambda f, i, p: R.t_generative(f, i, t["cnt"], avg, (H, W)), ("flow", "img")),
            "temporal": (lambda f, i, p: R.t_temporal(f, p, i, (H, W), WEIGHTS[1]), ("flow", "prev", "img")),
            "regularization": (lambda f, i, p: R.t_total_variation(i, WEIGHTS[0]), ("img",)),
        }

        def both(fn, wrt):
            loss = fn(leaf["flow"], leaf["img"], leaf["prev"])
            return (loss.detach(),) + tuple(torch.autograd.grad(loss, [leaf[k] for k in wrt]))

        line = {"op": "BrightnessConstancy", "flows": name, "B": B, "H": H, "W": W, "events_per_item": N_EVENTS, "iters": args.iters}
        for term, (fn, wrt) in ours.items():
            line[term + "_forward_ms"] = timed(lambda: fn(t["flow"], t["img"], t["prev"]), args.iters)
            line[term + "_forward_backward_ms"] = timed(lambda: both(fn, wrt), args.iters)
            line[term + "_bit_reproducible"] = same(both(fn, wrt), both(fn, wrt))
        N.prof_reset()
        N.prof_enable(True)
        reps = min(args.iters, 5)
        for _ in range(reps):
            for term in ("generative", "temporal", "regularization"):
                both(*ours[term])
        torch.cuda.synchronize()
        N.prof_enable(False)
        line["kernel_ms"] = {k: round(v[1] / reps, 4) for k, v in N.prof_collect().items() if k.startswith(("bc_", "sobel_"))}
        for term, (fn, wrt) in eager.items():
            line["eager_" + term + "_forward_ms"] = timed(lambda: fn(t["flow"], t["img"], t["prev"]), args.iters)
            line["eager_" + term + "_forward_backward_ms"] = timed(lambda: both(fn, wrt), args.iters)
            a, b, mine = both(fn, wrt), both(fn, wrt), both(*ours[term])
            line["eager_" + term + "_bit_reproducible"] = same(a, b)
            line["eager_" + term + "_loss_rel_diff"] = abs(float(a[0]) - float(mine[0])) / abs(float(mine[0]))
            line["eager_" + term + "_grad_diff_of_max"] = max(float((x - y).abs().max() / y.abs().max()) for x, y in zip(a[1:], mine[1:]))
            # elements further than 1e-3 of the largest from ours: the pixels at a kink (a sample coordinate at an integer, an
            # L1 argument at 0), where float32 arithmetic and the float64 coordinates here take different branches
            line["eager_" + term + "_grad_elements_off"] = sum(int(((x - y).abs() > 1e-3 * y.abs().max()).sum()) for x, y in zip(a[1:], mine[1:]))
            line["eager_" + term + "_grad_elements"] = sum(x.numel() for x in a[1:])
        line["device"] = torch.cuda.get_device_name(0)
        text = json.dumps(line)
        print(text, flush=True)
        lines.append(text)
        del t, leaf, avg
        torch.cuda.empty_cache()
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            f.write("\n".join(lines) + "\n")
    return 0


if __name__ == "__main__":
    sys.exit(main())
