"""Device time of ebfi_optim_step on ONE flat float32 buffer of the default model's 5 693 543 parameters, every variant, beside
the existing ebfi_adam_step_guarded launch and torch's own fused step of the same class on that single flat tensor.  Device
events around a burst of 10 launches enqueued behind a long matrix product (the events then bracket device work alone), median
of 60 bursts after 10 warm-up bursts; the variants alternate inside every repetition.  Bytes per
launch = maps x 4 x n (what the algorithm must move).  The working set (68 - 205 MB) fits the 256 MiB Infinity Cache: the rates
are cache-assisted, not fractions of HBM bandwidth.  Numbers: profiles/optim.md.
A second table holds what clipping and the weight average add: the two launches of ebfi_grad_norm on the same gradient (against the
floor of reading it once from HBM at 8 TB/s) and ebfi_optim_step_ex with a scale and an average beside the same configuration
without them (two more maps).

    python tools/optimbench.py [--n 5693543] [--reps 60]"""
import argparse
import os
import statistics
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "ebfi-be_amd"))
import torch  # noqa: E402
from ebfi_amd import _native as N  # noqa: E402
from ebfi_amd.dp import FlatOptimizer  # noqa: E402

# (label, torch class, arguments, maps moved per element)
VARIANTS = [
    ("adam (existing kernel)", "Adam", {}, 7),
    ("adam l2", "Adam", {"weight_decay": 1e-2}, 7),
    ("adam amsgrad", "Adam", {"amsgrad": True}, 9),
    ("adam l2 amsgrad", "Adam", {"weight_decay": 1e-2, "amsgrad": True}, 9),
    ("adamw", "AdamW", {"weight_decay": 1e-2}, 7),
    ("adamw amsgrad", "AdamW", {"weight_decay": 1e-2, "amsgrad": True}, 9),
    ("sgd", "SGD", {}, 3),
    ("sgd l2", "SGD", {"weight_decay": 1e-3}, 3),
    ("sgd momentum", "SGD", {"momentum": 0.9, "dampening": 0.1}, 5),
    ("sgd l2 momentum", "SGD", {"momentum": 0.9, "weight_decay": 1e-3}, 5),
    ("sgd nesterov", "SGD", {"momentum": 0.9, "nesterov": True}, 5),
    ("sgd l2 nesterov", "SGD", {"momentum": 0.9, "nesterov": True, "weight_decay": 1e-3}, 5),
]


BURST = 10          # launches per timing


def timed(fn, blocker):
    """Device milliseconds per call of `fn`: BURST calls are enqueued while a long matrix product keeps the device busy, so
    they run back to back and the events bracket device work alone, not the host's enqueue."""
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    blocker()
    a.record()
    for _ in range(BURST):
        fn()
    b.record()
    b.synchronize()
    return a.elapsed_time(b) / BURST


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--n", type=int, default=5693543)
    ap.add_argument("--reps", type=int, default=60)
    ap.add_argument("--warmup", type=int, default=10)
    args = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("optimbench.py measures on the GPU; none is visible")
    n, dev = args.n, torch.device("cuda")
    gen = torch.Generator(device=dev).manual_seed(0)
    grad = torch.randn(n, device=dev, generator=gen) * 1e-3
    start = torch.randn(n, device=dev, generator=gen) * 0.1
    guard = torch.zeros(2, dtype=torch.int32, device=dev)
    flag = torch.zeros(1, device=dev)
    runs = []
    for label, name, oargs, maps in VARIANTS:
        ours = FlatOptimizer([torch.nn.Parameter(start.clone())], name, lr=1e-4, **oargs)
        p = torch.nn.Parameter(start.clone())
        p.grad = grad
        theirs = getattr(torch.optim, name)([p], lr=1e-4, fused=True, **oargs)
        runs.append((label, maps, (lambda o=ours: o.step(grad, guard=guard, flag=flag)), theirs.step))
    # the existing launch, called directly
    p, m, v, step = start.clone(), torch.zeros(n, device=dev), torch.zeros(n, device=dev), torch.zeros((), device=dev)

    def old():
        step.add_(1)
        N.check(N.lib().ebfi_adam_step_guarded(N.ptr(p), N.ptr(grad), N.ptr(m), N.ptr(v), N.ptr(step), n, 1e-4, 0.9, 0.999, 1e-8,
                                               N.ptr(guard), N.ptr(flag), N.stream_ptr(dev)), "ebfi_adam_step_guarded")
    runs.append(("ebfi_adam_step_guarded, direct", 7, old, None))
    # clipping / average: the norm launches alone, and the update with and without scale + average (direct calls, same hyper-
    # parameters; plain Adam without them forwards to the existing kernel)
    first = len(runs)
    ws = torch.empty(max(1, N.lib().ebfi_grad_norm_workspace(n) // 8), dtype=torch.float64, device=dev)
    norm_out = torch.zeros(2, device=dev)
    for label, kind in (("grad norm L2 (2 launches)", N.CONSTANTS["EBFI_NORM_L2"]), ("grad norm inf (2 launches)", N.CONSTANTS["EBFI_NORM_INF"])):
        runs.append((label, 1, (lambda k=kind: N.check(N.lib().ebfi_grad_norm(N.ptr(grad), n, k, 1.0, N.ptr(norm_out), N.ptr(ws), ws.numel() * 8,
                                                                               N.stream_ptr(dev)), "ebfi_grad_norm")), None))
    scale = torch.full((1,), 0.5, device=dev)
    for label, kind, flags, wd, mom, maps in (("adam", 0, 0, 0.0, 0.0, 7), ("adamw", 0, 1, 1e-2, 0.0, 7), ("adamw amsgrad", 0, 3, 1e-2, 0.0, 9),
                                              ("sgd l2 nesterov", 1, 4, 1e-3, 0.9, 5)):
        for extra in (False, True):
            bufs = [start.clone()] + [torch.zeros(n, device=dev) for _ in range(4)]
            words = [torch.zeros((), device=dev), torch.zeros((), device=dev)]

            def ex(kind=kind, flags=flags, wd=wd, mom=mom, extra=extra, bufs=bufs, words=words):
                words[0].add_(1)
                if extra:
                    words[1].add_(1)
                N.check(N.lib().ebfi_optim_step_ex(kind, flags, N.ptr(bufs[0]), N.ptr(grad), N.ptr(bufs[1]), N.ptr(bufs[2]),
                                                   N.ptr(bufs[3] if flags & 2 and kind == 0 else None), N.ptr(words[0]), n, 1e-4, 0.9, 0.999,
                                                   1e-8, wd, mom, 0.0, N.ptr(guard), N.ptr(flag), N.ptr(scale if extra else None),
                                                   N.ptr(bufs[4] if extra else None), N.ptr(words[1] if extra else None), 0.999, 1,
                                                   N.stream_ptr(dev)), "ebfi_optim_step_ex")
            runs.append(("step_ex %s%s" % (label, " + scale + ema" if extra else ""), maps + (2 if extra else 0), ex, None))
    big = torch.randn(8192, 8192, device=dev, generator=gen)
    blocker = lambda: torch.mm(big, big)
    times = {(label, who): [] for label, _, _, t in runs for who in ("ours", "torch")}
    for rep in range(args.warmup + args.reps):
        for label, _, ours, theirs in runs:
            for who, fn in (("ours", ours), ("torch", theirs)):
                if fn is None:
                    continue
                t = timed(fn, blocker)
                if rep >= args.warmup:
                    times[(label, who)].append(t)
    print("n = %d elements, %d timed bursts of %d launches each (the step-word increment, one tiny launch, is inside every figure "
          "but plain SGD's)" % (n, args.reps, BURST))
    print("| variant | maps | MB per launch | this launch, us (min - max) | TB/s | torch fused step, us | ours / torch |")
    print("|---|---|---|---|---|---|---|")
    for label, maps, _, theirs in runs:
        t = times[(label, "ours")]
        med = statistics.median(t)
        mb = maps * 4.0 * n / 1e6
        if theirs is None:
            ref, ratio = "-", "-"
        else:
            tm = statistics.median(times[(label, "torch")])
            ref, ratio = "%.1f" % (tm * 1e3), "%.2f" % (med / tm)
        print("| %s | %d | %.1f | %.1f (%.1f - %.1f) | %.2f | %s | %s |"
              % (label, maps, mb, med * 1e3, min(t) * 1e3, max(t) * 1e3, mb / med / 1e3, ref, ratio))
    floor = 4.0 * n / 8e12 * 1e6
    print("clipping / average (rows from 'grad norm' on): reading the gradient once from HBM at 8 TB/s takes %.2f us" % floor)
    for label, _, _, _ in runs[first:first + 2]:
        med = statistics.median(times[(label, "ours")]) * 1e3
        print("%s: %.1f us = %.2f of that floor" % (label, med, floor / med))


if __name__ == "__main__":
    main()
