#!/usr/bin/env python3
"""The training loss (Laplacian difference pyramid + census, two predictions) forward and backward in isolation at the
benchmark's shape, library event pairs per kernel; then every pyramid kernel per level (a 2-level pyramid at the level's
size runs exactly that level's reduce / level / bwd_reduce / bwd_expand launches).  Prints sha1 digests of the loss
gradients so that two builds can be compared bit for bit (EBFI_DEV=1 EBFI_LIB_PATH=<other build> for the other arm).
usage: python tools/lossbench.py [B H W]"""
import hashlib
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "ebfi-be_amd"))
import torch  # noqa: E402

from ebfi_amd import _native as N  # noqa: E402
from ebfi_amd.loss import TrainLoss  # noqa: E402

B, H, W = (int(v) for v in sys.argv[1:4]) if len(sys.argv) >= 4 else (8, 256, 256)
torch.manual_seed(0)
target = torch.rand(B, 3, H, W).cuda()
sharp = (target + 0.05 * torch.randn(B, 3, H, W).cuda()).requires_grad_()
sharp_pre = (target + 0.1 * torch.randn(B, 3, H, W).cuda()).requires_grad_()
loss = TrainLoss().cuda()
lib = N.lib()


def timed(fn, iters=20):
    for _ in range(3):
        fn()
    torch.cuda.synchronize()
    N.prof_reset()
    N.prof_enable(True)
    for _ in range(iters):
        fn()
    torch.cuda.synchronize()
    N.prof_enable(False)
    return {k: (v[0] / iters, 1e3 * v[1] / v[0]) for k, v in N.prof_collect().items() if v[0]}


def step():
    sharp.grad = sharp_pre.grad = None
    out = loss(sharp_pre, sharp, target)
    out.backward()
    return out


out = step()
torch.cuda.synchronize()
sha = lambda t: hashlib.sha1(t.detach().cpu().numpy().tobytes()).hexdigest()[:16]
print("library %s" % N.LIB_PATH)
print("loss %.9g  grad(sharp) %s  grad(sharp_pre) %s" % (out.item(), sha(sharp.grad), sha(sharp_pre.grad)))
t = timed(step)
total = 0.0
print("whole loss, B=%d 3x%dx%d, two predictions (launches per step x average):" % (B, H, W))
for name in sorted(t):
    n, us = t[name]
    if name.startswith(("lap_", "census_")):
        total += n * us
    print("  %-16s %4.1f x %7.1f us" % (name, n, us))
print("  lap_* + census_* per step: %.1f us" % total)

planes = 2 * B * 3
g = torch.ones(1, device="cuda")
st = N.stream_ptr(target.device)
for l in range(4):
    h, w = H >> l, W >> l
    a, b, tt = (torch.rand(B, 3, h, w).cuda() for _ in range(3))
    ws = torch.empty(int(lib.ebfi_laploss_workspace_floats(planes, h, w, 2)), device="cuda")
    part = torch.empty(int(lib.ebfi_laploss_partials(planes, h, w, 2)), device="cuda")
    gp = torch.empty(planes * h * w, device="cuda")

    def level():
        N.check(lib.ebfi_laploss_forward(N.ptr(a), N.ptr(b), N.ptr(tt), 0.1, 1.0, N.ptr(ws), N.ptr(part), B * 3, h, w, 2, st), "fwd")
        N.check(lib.ebfi_laploss_backward(N.ptr(g), N.ptr(ws), N.ptr(gp), planes, h, w, 2, st), "bwd")

    t = timed(level)
    # (lap_level runs twice here: this level and the elementwise coarsest one, a quarter of its size; level 0 of the old
    # form has lap_diff as a launch of its own)
    print("level %d (%dx%d): %s" % (l, h, w, "  ".join("%s %.1fx%.1f us" % (k, v[0], v[1]) for k, v in sorted(t.items()))), flush=True)
