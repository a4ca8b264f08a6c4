#!/usr/bin/env python3
"""Cost of the deformable PS-ROI pooling (ebfi_amd.dcn.dcn_v2_pooling_forward / _backward, csrc/dcnpool.hip) at two detection-head
shapes, with, in the same call and alternating with the native passes, a PyTorch-ROCm eager restatement of the same law
(written below with index and gather ops; its backward is autograd's) as the yardstick.

    python tools/poolbench.py [--iters 20] [--warmup 3] [--no-eager] [--out profiles/dcn_pooling.md]

Shapes: input [2, C, 50, 68], 300 seeded ROIs, pooled_size = part_size = 7, sample_per_part = 4, scale 1/16, trans_std 0.1;
  roi_align  deformable RoI-align: output_dim 256, group_size 1 (C = 256), one class
  ps         position-sensitive:   output_dim 10, group_size 7 (C = 490), one class
and `roi_align` once more with output_dim halved: the geometry is computed once per (ROI, class), so the forward's time should
follow the channel count.

Prints one JSON line and rewrites the part of --out between the `poolbench` markers (the rest of the file is kept).  Times are
device events around one call, mean of --iters calls after --warmup.  Algorithmic bytes count every tensor of a call once
(grad_input once, although it is zeroed and then accumulated); `hbm_share` is those bytes over 8 TB/s over the measured time.
One box, one run: a measurement, not a bar.
"""
import argparse
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for p in (os.path.join(ROOT, "ebfi-be_amd"), ROOT):
    sys.path.insert(0, p)

import torch  # noqa: E402

HBM_PEAK = 8.0e12
BEGIN, END = "<!-- poolbench:begin -->", "<!-- poolbench:end -->"
SHAPES = {
    # name: (B, D, G, H, W, R, P, part, spp, scale, trans_std)
    "roi_align": (2, 256, 1, 50, 68, 300, 7, 7, 4, 1.0 / 16, 0.1),
    "ps": (2, 10, 7, 50, 68, 300, 7, 7, 4, 1.0 / 16, 0.1),
    "roi_align_half_D": (2, 128, 1, 50, 68, 300, 7, 7, 4, 1.0 / 16, 0.1),
}


def c_round(v):
    t = torch.trunc(v)
    return t + torch.where((v - t).abs() >= 0.5, torch.copysign(torch.ones_like(v), v), torch.zeros_like(v))


def eager_forward(inp, rois, trans, scale, P, D, G, part, spp, trans_std):
    """The law of include/ebfi_hip.h in float32 tensor ops, one class.  The divisors are 0-dim device tensors: a tensor divided
    by a Python number is multiplied by its reciprocal on the GPU, which moves a sample that sits next to an integer
    coordinate across it -- and with it one cell of the offset gradient by a visible amount."""
    B, C, H, W = inp.shape
    R = rois.shape[0]
    f = inp.dtype
    dev = inp.device
    P_, spp_ = torch.tensor(float(P), device=dev, dtype=f), torch.tensor(float(spp), device=dev, dtype=f)
    bi = rois[:, 0]
    valid = (bi >= 0) & (bi < B) & (bi == torch.floor(bi))
    batch = torch.where(valid, bi, torch.zeros_like(bi)).long()
    sw, sh = c_round(rois[:, 1]) * scale - 0.5, c_round(rois[:, 2]) * scale - 0.5
    ew, eh = (c_round(rois[:, 3]) + 1) * scale - 0.5, (c_round(rois[:, 4]) + 1) * scale - 0.5
    rw, rh = torch.clamp_min(ew - sw, 0.1), torch.clamp_min(eh - sh, 0.1)
    bw, bh = rw / P_, rh / P_
    sbw, sbh = bw / spp_, bh / spp_
    p = torch.arange(P, device=dev, dtype=f)
    part_of = torch.floor(p / P_ * part).long()
    g_of = torch.floor(p * G / P_).long().clamp(0, G - 1)
    tx = trans[:R, 0][:, part_of[:, None], part_of[None, :]] * trans_std            # [R, ph, pw]
    ty = trans[:R, 1][:, part_of[:, None], part_of[None, :]] * trans_std
    r3 = lambda v: v[:, None, None]
    w0 = p[None, None, :] * r3(bw) + r3(sw) + tx * r3(rw)
    h0 = p[None, :, None] * r3(bh) + r3(sh) + ty * r3(rh)
    i = torch.arange(spp, device=dev, dtype=f)
    r5 = lambda v: v[:, None, None, None, None]
    w = (w0[..., None, None] + i[None, None, None, None, :] * r5(sbw)).expand(R, P, P, spp, spp)
    h = (h0[..., None, None] + i[None, None, None, :, None] * r5(sbh)).expand(R, P, P, spp, spp)
    inc = ~((w < -0.5) | (w > W - 0.5) | (h < -0.5) | (h > H - 0.5)) & r5(valid)
    wc, hc = w.clamp(0, W - 1), h.clamp(0, H - 1)
    fw, fh = torch.floor(wc), torch.floor(hc)
    dx, dy = (wc - fw)[:, None], (hc - fh)[:, None]                                  # [R, 1, ph, pw, ih, iw]
    x0, x1, y0, y1 = (v.long()[:, None] for v in (fw, torch.ceil(wc), fh, torch.ceil(hc)))
    chan = ((torch.arange(D, device=dev)[:, None, None] * G + g_of[None, :, None]) * G + g_of[None, None, :])
    chan = chan[None, :, :, :, None, None]                                           # [1, D, ph, pw, 1, 1]
    b = batch[:, None, None, None, None, None]
    val = ((1 - dx) * (1 - dy) * inp[b, chan, y0, x0] + (1 - dx) * dy * inp[b, chan, y1, x0] +
           dx * (1 - dy) * inp[b, chan, y0, x1] + dx * dy * inp[b, chan, y1, x1])
    m = inc[:, None]
    total = torch.where(m, val, torch.zeros_like(val)).sum(dim=(4, 5))
    count = inc.sum(dim=(3, 4)).to(f)[:, None].expand(R, D, P, P)
    return torch.where(count > 0, total / count.clamp_min(1), torch.zeros_like(total)), count


def algorithmic_bytes(B, D, G, H, W, R, P, part):
    inp, out, tr = B * D * G * G * H * W, R * D * P * P, R * 2 * part * part
    fwd = 4 * (inp + 5 * R + tr + 2 * out)                   # input, rois, trans; output and count
    bwd = 4 * (2 * out + inp + 5 * R + tr + inp + tr)        # grad_output, count, input, rois, trans; grad_input, grad_trans
    return fwd, bwd


def main(argv=None):
    ap = argparse.ArgumentParser(description=__doc__.split("\n")[0])
    ap.add_argument("--iters", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--no-eager", action="store_true", help="skip the PyTorch eager yardstick")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "dcn_pooling.md"))
    args = ap.parse_args(argv)
    if not torch.cuda.is_available():
        raise SystemExit("poolbench.py measures on an MI355X; no GPU is visible")
    from ebfi_amd import dcn
    dev = torch.device("cuda", 0)
    ev = lambda: torch.cuda.Event(enable_timing=True)
    res = dict(iters=args.iters, warmup=args.warmup, shapes={})
    for name, (B, D, G, H, W, R, P, part, spp, scale, tstd) in SHAPES.items():
        g = torch.Generator().manual_seed(7)
        inp = torch.randn((B, D * G * G, H, W), generator=g).to(dev)
        ext_w, ext_h = W / scale, H / scale
        xy = torch.rand((R, 2), generator=g) * torch.tensor([0.8 * ext_w, 0.8 * ext_h])
        wh = torch.rand((R, 2), generator=g) * torch.tensor([0.4 * ext_w, 0.4 * ext_h]) + 16
        rois = torch.cat([torch.randint(0, B, (R, 1), generator=g).float(), xy, xy + wh], dim=1).to(dev)
        trans = torch.randn((R, 2, part, part), generator=g).to(dev)
        go = torch.randn((R, D, P, P), generator=g).to(dev)
        tail = (False, scale, D, G, P, part, spp, tstd)
        out, count = dcn.dcn_v2_pooling_forward(inp, rois, trans, *tail)

        def native_fwd():
            return dcn.dcn_v2_pooling_forward(inp, rois, trans, *tail)

        def native_bwd():
            return dcn.dcn_v2_pooling_backward(go, inp, rois, trans, count, *tail)

        todo = [("forward_ms", native_fwd), ("backward_ms", native_bwd)]
        entry = dict(B=B, D=D, G=G, H=H, W=W, R=R, P=P, part=part, spp=spp)
        if not args.no_eager:
            e_inp, e_trans = inp.clone().requires_grad_(True), trans.clone().requires_grad_(True)
            state = {}

            def eager_fwd():
                state["out"] = eager_forward(e_inp, rois, e_trans, scale, P, D, G, part, spp, tstd)[0]

            def eager_bwd():
                return torch.autograd.grad(state["out"], (e_inp, e_trans), go)

            eager_fwd()
            with torch.no_grad():
                entry["eager_count_equals_native"] = bool(torch.equal(
                    eager_forward(inp, rois, trans, scale, P, D, G, part, spp, tstd)[1], count))
            e_gi, e_gt = eager_bwd()
            gi, gt = native_bwd()
            rel = lambda a, b: ((a - b).abs().max() / b.abs().max()).item()
            entry["eager_vs_native_rel"] = dict(forward=rel(out, state["out"].detach()), grad_input=rel(gi, e_gi),
                                                grad_trans=rel(gt, e_gt))
            todo = [todo[0], ("eager_forward_ms", eager_fwd), todo[1], ("eager_backward_ms", eager_bwd)]     # alternating
        series = {k: [] for k, _ in todo}
        for it in range(args.warmup + args.iters):
            for key, fn in todo:
                a, z = ev(), ev()
                a.record()
                fn()
                z.record()
                if it >= args.warmup:
                    series[key].append((a, z))
            torch.cuda.synchronize()
        for key, pairs in series.items():
            v = [a.elapsed_time(z) for a, z in pairs]
            entry[key] = round(sum(v) / len(v), 4)
            entry[key.replace("_ms", "_min_max_ms")] = [round(min(v), 4), round(max(v), 4)]
        fb, bb = algorithmic_bytes(B, D, G, H, W, R, P, part)
        entry["forward_mbyte"], entry["backward_mbyte"] = round(fb / 1e6, 2), round(bb / 1e6, 2)
        entry["forward_hbm_share"] = fb / HBM_PEAK / (entry["forward_ms"] * 1e-3)
        entry["backward_hbm_share"] = bb / HBM_PEAK / (entry["backward_ms"] * 1e-3)
        if "eager_forward_ms" in entry:
            entry["forward_speedup"] = round(entry["eager_forward_ms"] / entry["forward_ms"], 2)
            entry["backward_speedup"] = round(entry["eager_backward_ms"] / entry["backward_ms"], 2)
        res["shapes"][name] = entry
        print("%s done" % name, flush=True)
    res["forward_half_D_over_full"] = round(res["shapes"]["roi_align_half_D"]["forward_ms"] / res["shapes"]["roi_align"]["forward_ms"], 3)
    print(json.dumps(res))

    rows = ["| shape | pass | native ms (min .. max) | eager ms | eager / native | MB | share of 8 TB/s |", "|---|---|---|---|---|---|---|"]
    for name, e in res["shapes"].items():
        for ps in ("forward", "backward"):
            lo, hi = e[ps + "_min_max_ms"]
            eager = e.get("eager_%s_ms" % ps)
            rows.append("| %s | %s | %.4f (%.4f .. %.4f) | %s | %s | %.2f | %.2f %% |" % (
                name, ps, e[ps + "_ms"], lo, hi, "%.3f" % eager if eager is not None else "not measured",
                "%.1f" % e[ps + "_speedup"] if eager is not None else "-", e[ps + "_mbyte"], 100 * e[ps + "_hbm_share"]))
    text = [BEGIN, "", "Command: `python tools/poolbench.py%s` (device events around one call, mean of %d calls after %d warm-up calls; "
            "native and eager calls alternate inside one loop)." % (" --no-eager" if args.no_eager else "", args.iters, args.warmup), "",
            "\n".join(rows), "",
            "Forward at half the output channels over the full forward (`roi_align_half_D` / `roi_align`): %.3f." % res["forward_half_D_over_full"],
            "", "```json", json.dumps(res), "```", "", END]
    old = open(args.out).read() if os.path.exists(args.out) else \
        "# Deformable PS-ROI pooling (`ebfi_amd/dcn.py`, `csrc/dcnpool.hip`): measurements\n\n%s\n%s\n" % (BEGIN, END)
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
