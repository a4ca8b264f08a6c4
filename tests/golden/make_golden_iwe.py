#!/usr/bin/env python3
"""Golden fixture for ebfi_amd.iwe: RUNS THE REFERENCE'S OWN myutils/iwe.py and loss/flow.py on the CPU and stores what they
returned.  Only data is written.

    python tests/golden/make_golden_iwe.py <reference checkout>      # rewrites iwe_small.npz and loss_names.txt

The functions add fractional float32 weights with scatter_add_; with one thread that loop walks the list in order, which is
the law the device kernels implement, so this script runs under torch.set_num_threads(1).

Per case `<c>` the file holds the inputs (`<c>__events` [B, N, 4] = (ts, y, x, p), `<c>__pol_mask` [B, N, 2], `<c>__flows`
[K, B, 2, H, W], `<c>__H`, `<c>__W`, `<c>__weight`) and the float32 outputs of
get_interpolation (`gi_{bil,rnd}_{t1,t0}_{idx,w}`), interpolate (`interp`: bilinear, tref = 1, positive mask; `interp_plain`:
no mask), deblur_events (`deblur`), compute_pol_iwe (`pol_rnd`, `pol_bil`), AveragedIWE (`avg`) and EventWarping (`loss32`,
`grad32` [K, B, 2, H, W]); `loss64` / `grad64` are the same call with float64 inputs under
torch.set_default_dtype(torch.float64) (the reference builds its buffers with the default dtype).  `dev_loss` / `dev_grad`: the
largest deviation of the float32 run from the float64 run over the cases -- relative for the loss, largest absolute error
over largest absolute gradient for the gradient; the tests' bar is 8 times that.

For the cases compared under a tolerance an event is resampled while the float64 warped coordinate (either tref, any flow)
lies within 1e-3 of an integer: there float32 and float64 pick different corners.  The script asserts none remains.

loss_names.txt: `loss <name>` for every class or function defined in the reference's loss/flow.py and loss/restore.py and
every name loss/__init__.py imports explicitly, `myutils.iwe <name>` for every function of myutils/iwe.py.  loss/reconstruction.py
(BrightnessConstancy) is not listed: it has no counterpart.
"""
import ast
import importlib.util
import os
import sys

import numpy as np
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.dirname(HERE))
import iwe_ref as R  # noqa: E402

F = np.float32


def load_reference(root):
    sys.path.insert(0, root)                        # loss/flow.py imports myutils.iwe from its own checkout
    mods = []
    for name, rel in (("reference_iwe", ("myutils", "iwe.py")), ("reference_flow", ("loss", "flow.py"))):
        spec = importlib.util.spec_from_file_location(name, os.path.join(root, *rel))
        mod = importlib.util.module_from_spec(spec)
        spec.loader.exec_module(mod)
        mods.append(mod)
    return mods


def t(a, dtype=torch.float32):
    return torch.from_numpy(np.array(a)).to(dtype)          # a fresh copy every time


def masks(p):
    return np.stack([(p > 0), (p < 0)], axis=2).astype(F)


def random_events(rng, B, N, H, W):
    ev = np.zeros((B, N, 4), F)
    ev[:, :, 0] = rng.uniform(0.02, 0.98, (B, N))
    ev[:, :, 1] = rng.integers(0, H, (B, N))
    ev[:, :, 2] = rng.integers(0, W, (B, N))
    ev[:, :, 3] = rng.choice([-1.0, 1.0], (B, N))
    return ev


def random_flows(rng, shape, bound):
    """Uniform in +-bound, pushed away from 0 (an event on a pixel without flow warps to an integer whatever its stamp)."""
    f = rng.uniform(-bound, bound, shape).astype(F)
    return np.where(np.abs(f) < F(0.01), np.copysign(F(0.01), f), f).astype(F)


def resample(rng, flows, ev, pm, res):
    """Redraw the stamp of every live event that warps to within 1e-3 of an integer; the pixel is never redrawn."""
    for _ in range(200):
        bad = R.near_integer(flows, ev, pm, res)
        if not bad.any():
            return ev
        ev[bad, 0] = rng.uniform(0.02, 0.98, int(bad.sum())).astype(F)
    raise AssertionError("could not move every event away from the integers")


def case_general(rng):
    B, H, W, N = 2, 12, 20, 600
    flows = random_flows(rng, (2, B, 2, H, W), 0.15)
    ev = random_events(rng, B, N, H, W)
    pm = masks(ev[:, :, 3])
    return dict(events=resample(rng, flows, ev, pm, (H, W)), pol_mask=pm, flows=flows, H=H, W=W, weight=0.001)


def case_pile(rng):
    B, H, W, N = 1, 8, 10, 360
    flows = random_flows(rng, (1, B, 2, H, W), 0.1)
    flows[0, 0, 1, 3, 4], flows[0, 0, 0, 3, 4] = F(0.03), F(0.02)      # 0.3 and 0.2 pixels at most: one 2 x 2 footprint
    ev = random_events(rng, B, N, H, W)
    pile = rng.permutation(N)[:300]
    ev[0, pile, 1], ev[0, pile, 2] = 3, 4
    ev[0, pile, 3] = 1
    pm = masks(ev[:, :, 3])
    return dict(events=resample(rng, flows, ev, pm, (H, W)), pol_mask=pm, flows=flows, H=H, W=W, weight=0.001)


def case_boundaries(rng):
    B, H, W, N = 3, 6, 7, 257
    flows = random_flows(rng, (1, B, 2, H, W), 0.12)
    ev = random_events(rng, B, N, H, W)
    ev[:, 0:6, 1], ev[:, 0:6, 2] = 0, 0                                  # pixel 0 and pixel H * W - 1 of every item,
    ev[:, N - 6:, 1], ev[:, N - 6:, 2] = H - 1, W - 1                    # at both ends of the list
    flows[0, :, :, 0, 0] = F(0.05)
    flows[0, :, :, H - 1, W - 1] = F(-0.05)
    flows[0, 1, :, 0, 0] = F(-0.05)                                      # item 1 pushes both outwards: nothing may wrap
    flows[0, 1, :, H - 1, W - 1] = F(0.05)
    pm = masks(ev[:, :, 3])
    return dict(events=resample(rng, flows, ev, pm, (H, W)), pol_mask=pm, flows=flows, H=H, W=W, weight=0.01)


def case_ties(rng):
    B, H, W, N = 1, 5, 6, 40
    flows = np.zeros((1, B, 2, H, W), F)
    ev = random_events(rng, B, N, H, W)
    ev[0, :, 0] = rng.choice([0.0, 1.0, 0.5, 0.25], N)
    ev[0, 0, 0], ev[0, 1, 0] = 0.0, 1.0
    return dict(events=ev, pol_mask=masks(ev[:, :, 3]), flows=flows, H=H, W=W, weight=0.001)


def case_empty(rng):
    B, H, W = 2, 4, 5
    flows = random_flows(rng, (1, B, 2, H, W), 0.15)
    return dict(events=np.zeros((B, 0, 4), F), pol_mask=np.zeros((B, 0, 2), F), flows=flows, H=H, W=W, weight=0.5)


def case_padding(rng):
    B, H, W, N = 2, 6, 8, 90
    flows = random_flows(rng, (1, B, 2, H, W), 0.15)
    ev = random_events(rng, B, N, H, W)
    ev[0, 60:], ev[1, 45:] = 0, 0                                        # padding rows: all zeros, masked out
    pm = masks(ev[:, :, 3])
    return dict(events=resample(rng, flows, ev, pm, (H, W)), pol_mask=pm, flows=flows, H=H, W=W, weight=0.001)


def case_average(rng):
    """AveragedIWE by hand, 5 x 6 (flow_scaling 6, stamps 0: the warp adds 6 * flow exactly)."""
    B, H, W = 1, 5, 6
    flows = np.zeros((1, B, 2, H, W), F)
    flows[0, 0, 1, 1, 1] = F(0.25)      # y 1 -> 2.5 -> 2 (half to even)
    flows[0, 0, 1, 2, 2] = F(0.25)      # y 2 -> 3.5 -> 4
    flows[0, 0, 1, 4, 3] = F(0.125)     # y 4 -> 4.75 -> 5 = H: unfeasible
    flows[0, 0, 0, 0, 4] = F(0.25)      # x 4 -> 5.5 -> 6 = W: unfeasible
    rows = [
        (0.0, 1, 1, 1), (0.0, 1, 1, 1),          # the same source, destination and polarity: one contribution
        (0.0, 2, 1, 1),                          # a second source into (2, 1): two contributions
        (0.0, 1, 1, -1),                         # the other polarity of the first mapping
        (0.0, 2, 2, 1), (0.0, 4, 2, 1), (0.0, 4, 2, 1), (0.0, 4, 2, 0),      # 3.5 -> 4 joins the events that rest at (4, 2)
        (0.0, 4, 3, 1), (0.0, 0, 4, -1),         # leave the image
        (1.0, 1, 1, 1),                          # stamp 1: stays at (1, 1)
    ]
    ev = np.array(rows, F)[None]
    return dict(events=ev, pol_mask=masks(ev[:, :, 3]), flows=flows, H=H, W=W, weight=0.001)


CASES = (("general", case_general), ("pile", case_pile), ("bounds", case_boundaries), ("ties", case_ties), ("empty", case_empty),
         ("padding", case_padding), ("average", case_average))
TOLERANCE_CASES = ("general", "pile", "bounds", "padding")


def run_case(iwe, flow_mod, c):
    ev, pm, flows, H, W, weight = c["events"], c["pol_mask"], c["flows"], c["H"], c["W"], c["weight"]
    res, scaling = (H, W), max(H, W)
    B = ev.shape[0]
    out = {}
    fe = R.event_flow(flows[0], ev, res)
    for branch, rnd in (("bil", False), ("rnd", True)):
        for tref in (1, 0):
            idx, w = iwe.get_interpolation(t(ev), t(fe), tref, res, scaling, round_idx=rnd)
            out["gi_%s_t%d_idx" % (branch, tref)], out["gi_%s_t%d_w" % (branch, tref)] = idx.numpy(), w.numpy()
    idx, w = iwe.get_interpolation(t(ev), t(fe), 1, res, scaling)
    pm4 = torch.cat([t(pm)] * 4, dim=1)
    out["interp"] = iwe.interpolate(idx.long(), w, res, polarity_mask=pm4[:, :, 0:1]).numpy()
    out["interp_plain"] = iwe.interpolate(idx.long(), w, res).numpy()
    out["deblur"] = iwe.deblur_events(t(flows[0]), t(ev), res, flow_scaling=scaling).numpy()
    for key, rnd in (("pol_rnd", True), ("pol_bil", False)):
        out[key] = iwe.compute_pol_iwe(t(flows[0]), t(ev), res, t(pm[:, :, 0:1]), t(pm[:, :, 1:2]), flow_scaling=scaling,
                                       round_idx=rnd).numpy()
    config = {"loader": {"resolution": [H, W], "batch_size": B}, "loss": {"flow_regul_weight": weight}}
    out["avg"] = flow_mod.AveragedIWE(config, "cpu")(t(flows[0]), t(ev), t(pm)).numpy()
    for name, dtype in (("32", torch.float32), ("64", torch.float64)):
        torch.set_default_dtype(dtype)
        try:
            leaves = [t(f, dtype).requires_grad_(True) for f in flows]
            loss = flow_mod.EventWarping(config, "cpu")(leaves, t(ev, dtype), t(pm, dtype), res)
            loss.backward()
        finally:
            torch.set_default_dtype(torch.float32)
        out["loss" + name] = loss.detach().numpy()
        out["grad" + name] = np.stack([leaf.grad.numpy() for leaf in leaves])
    assert out["loss32"].dtype == np.float32 and out["grad64"].dtype == np.float64
    return out


def loss_names(root):
    def defined(*rel):
        tree = ast.parse(open(os.path.join(root, *rel)).read())
        return [n.name for n in tree.body if isinstance(n, (ast.ClassDef, ast.FunctionDef)) and not n.name.startswith("_")]
    names = ["loss " + n for n in defined("loss", "flow.py") + defined("loss", "restore.py")]
    for node in ast.parse(open(os.path.join(root, "loss", "__init__.py")).read()).body:
        if isinstance(node, ast.ImportFrom):
            names += ["loss " + a.name for a in node.names if a.name != "*"]
    names += ["myutils.iwe " + n for n in defined("myutils", "iwe.py")]
    return names


def main():
    if len(sys.argv) != 2:
        sys.exit(__doc__)
    torch.set_num_threads(1)
    iwe, flow_mod = load_reference(sys.argv[1])
    rng = np.random.default_rng(20261021)
    store = {}
    dev_loss = dev_grad = 0.0
    for name, make in CASES:
        c = make(rng)
        res = (c["H"], c["W"])
        if name in TOLERANCE_CASES:
            assert not R.near_integer(c["flows"], c["events"], c["pol_mask"], res).any(), name
        out = run_case(iwe, flow_mod, c)
        l32, l64 = float(out["loss32"]), float(out["loss64"])
        dev_loss = max(dev_loss, abs(l32 - l64) / abs(l64))
        for g32, g64 in zip(out["grad32"], out["grad64"]):
            if np.abs(g64).max() > 0:
                dev_grad = max(dev_grad, float(np.abs(g32 - g64).max() / np.abs(g64).max()))
        for k, v in list(c.items()) + list(out.items()):
            store["%s__%s" % (name, k)] = np.asarray(v)
        print("%-8s loss32 %.9g loss64 %.17g" % (name, l32, l64))
    store["dev_loss"], store["dev_grad"] = np.float64(dev_loss), np.float64(dev_grad)
    print("dev_loss %.3g dev_grad %.3g" % (dev_loss, dev_grad))
    np.savez_compressed(os.path.join(HERE, "iwe_small.npz"), **store)
    with open(os.path.join(HERE, "loss_names.txt"), "w") as f:
        f.write("\n".join(loss_names(sys.argv[1])) + "\n")


if __name__ == "__main__":
    main()
