"""ResidualControl (ebfi_amd.model.ResidualControl, scheduled by ebfi_amd/rc_fused.py ResidualControlFn) as a module against a
plain float64 restatement on the CPU, in every route the node takes: output, the gradients of data / Ex / T and of every parameter,
Conv1 / Conv2 included.  Each pass asserts the route it took from the profile labels of that pass, the scale book's guard, and one
bound per tensor.

CASES is also read by tests/test_residual_control_host.py, which rebuilds every reference on the CPU, checks the restatement
against oracle/model_ref.residual_control and against the module's own CPU forward in double, and asserts the kink condition and
the batch predicate the GPU tests rely on: importing this module needs no GPU.

Tier A (default slope 0.01, every mode).  A LeakyReLU pre-activation that the device rounds to the other side of zero gives a
different, equally valid subgradient, and at these sizes one flipped element moves a weight gradient by percents.  A Tier-A case
is valid only if, in float64, every pre-activation z of every layer has |z| >= KINK * max|z| (1e-4); each case records a seed found
among 0..255 on the CPU for which this holds.
Tier B (tile geometry, slope 1.0 on every layer, Conv1 / Conv2 included).  Batched weight gradients need 40 tiles of 4 x 32 pixels:
hundreds of thousands of pre-activations, no seed is kink-free.  With slope 1.0 the activation is the identity, flips cannot
matter, and every copy, scale, slot, slice sum and pixel split still runs at real tile counts.  Each Tier-B case runs once more at
slope 0.01, where only the output (which does not feel kinks) is compared; gradients must be finite and the guard clear.

Modes (ALL_MODES) and the passes each makes:
  fp32           exact kernels, layer by layer + fused.scale_residual_cat
  bf16x3         split precision without a bank: layer by layer, weights packed per call
  bank           the fused node on the bank's images, fp32 stage (..._forward_ex / ..._backward_ex), split-precision gradients
  book           one bank + one ScaleBook through five passes on the same inputs:
                   1         fused node; fp16 weight / data gradients from fp32 tensors; every slot calibrated
                   2, 3      fp16 operand images; the round's tail in the grouped convolution's epilogue (packed_x3_rc with images,
                             ..._backward_c16a); the three weight gradients of a round batched exactly when `batched(...)`
                   restored  the (site, "a") slots dropped from book.calibrated: images WITHOUT the epilogue tail (..._forward_c16 /
                             ..._backward_c16), which re-measures `a`
                   after     the tail again
                 (rows that do not split into quads, W % 4 != 0: no images, every pass takes the route of pass 1)
  book-all       build_for(fwd16="all") + book.forward_f16 = "all": pass 1 calibrates, pass 2 runs fp16-operand forward convolutions
  nograd         torch.no_grad() under a bank: packed_x3_rc without images when W % 4 == 0, the three-launch form otherwise
A shape the node refuses (H * W % 4 != 0, C % 64 != 0) runs the module's layer-by-layer form under the bank: the fallback cases.

Bounds (error of a tensor: max|got - ref| / max|ref| against float64).  Per layer the (output, gradient) bounds of
tests/test_gpu_detail_stages.py PER_LAYER, times 3 * step + 1: three convolutions per round on the longest chain, one for the stage.
book-all is outside the parity bar by the project's own word: its output gets the 5e-3 of test_forward_f16_levels, its gradients
the per-parameter 5e-2 of test_benchmarked_step_vs_oracle.  Ceilings taken from the project, not fitted to what was measured.

Measured on an MI355X with the seeds below, output error / worst gradient error per mode and pass (book/3 and book/after repeat
book/2 to every digit shown; nograd's output equals bank's), and the largest error / bound over every compared tensor, mode and
pass of the row.  No bound was raised; the closest tensor (grad T of b-64-s1-b1-37x100, book/2) uses half of its bound.
  case                    slope fp32            bf16x3          bank            book/1          book/2          book/restored   book-all/all-2  worst/bound
  a-64-s1-b1-1x4          0.01  3.5e-07/7.2e-07 3.7e-06/1.4e-05 3.7e-06/1.4e-05 3.7e-06/1.2e-03 3.7e-06/1.2e-03 3.7e-06/1.2e-03 2.1e-04/1.2e-03 0.29
  a-64-s2-b1-2x4          0.01  6.2e-07/1.2e-06 4.7e-06/1.2e-05 4.7e-06/1.2e-05 4.7e-06/1.4e-03 4.7e-06/1.3e-03 4.7e-06/1.4e-03 3.0e-04/1.2e-03 0.20
  a-64-s2-b2-2x4          0.01  8.2e-07/1.6e-06 6.2e-06/3.6e-05 6.2e-06/3.6e-05 6.2e-06/7.9e-04 6.2e-06/8.0e-04 6.2e-06/8.0e-04 4.3e-04/1.2e-03 0.12
  a-128-s1-b1-2x4         0.01  1.6e-06/1.0e-06 6.2e-06/1.1e-05 6.2e-06/1.1e-05 6.2e-06/7.3e-04 6.2e-06/1.1e-03 6.2e-06/7.3e-04 4.3e-04/8.3e-04 0.29
  a-64-s2-b1-2x6          0.01  1.1e-06/1.2e-05 6.7e-06/2.8e-05 6.7e-06/2.6e-05 6.7e-06/6.1e-04 -               -               -               0.09
  a-64-s1-b2-4x4          0.01  1.0e-06/2.5e-06 5.6e-06/1.6e-05 5.6e-06/1.6e-05 5.6e-06/5.8e-04 5.6e-06/8.6e-04 5.6e-06/5.8e-04 2.8e-04/1.1e-03 0.21
  a-64-s1-b1-3x3-fallback 0.01  1.2e-06/8.2e-07 5.7e-06/1.9e-05 5.7e-06/1.9e-05 -               -               -               -               0.07
  a-32-s1-b1-2x4-fallback 0.01  4.3e-07/5.4e-06 6.0e-06/3.9e-05 6.0e-06/3.9e-05 -               -               -               -               0.07
  b-64-s2-b2-40x64        1     -               -               1.0e-05/1.2e-05 1.0e-05/1.4e-03 1.0e-05/1.4e-03 1.0e-05/1.4e-03 -               0.20
  b-64-s2-b2-40x64        0.01  -               -               7.8e-06/-       7.8e-06/-       7.8e-06/-       7.8e-06/-       -               0.06
  b-64-s2-b2-36x64        1     -               -               1.1e-05/2.0e-05 1.1e-05/8.6e-04 1.1e-05/8.9e-04 1.1e-05/8.9e-04 -               0.13
  b-64-s2-b2-36x64        0.01  -               -               6.8e-06/-       6.8e-06/-       6.8e-06/-       6.8e-06/-       -               0.05
  b-64-s1-b1-37x100       1     -               -               6.7e-06/6.2e-05 6.7e-06/1.4e-03 6.7e-06/2.0e-03 6.7e-06/1.4e-03 -               0.51
  b-64-s1-b1-37x100       0.01  -               -               4.7e-06/-       4.7e-06/-       4.7e-06/-       4.7e-06/-       -               0.06
  b-128-s1-b1-13x36       1     -               -               6.0e-06/9.4e-06 6.0e-06/5.8e-04 6.0e-06/7.9e-04 6.0e-06/7.9e-04 -               0.20
  b-128-s1-b1-13x36       0.01  -               -               4.5e-06/-       4.5e-06/-       4.5e-06/-       4.5e-06/-       -               0.06
  b-64-s1-b2-10x34        1     -               -               5.6e-06/1.2e-05 5.6e-06/3.0e-04 -               -               -               0.07
  b-64-s1-b2-10x34        0.01  -               -               4.9e-06/-       4.9e-06/-       -               -               -               0.06
(Tier B at slope 0.01: the uncompared weight gradients differ from float64 by 1e-2 .. 4e-2 in every mode, bank included -- the
flipped subgradients the kink condition keeps out of Tier A.)
"""
import collections
import contextlib
import math

import pytest
import torch
import torch.nn.functional as F

KINK = 1e-4
#                   output, gradients
PER_LAYER = {"fp32": (2e-5, 5e-5), "bf16x3": (2e-5, 2e-4), "bank": (2e-5, 2e-4), "nograd": (2e-5, 2e-4), "book": (1e-4, 1e-3)}
BOOK_ALL = (5e-3, 5e-2)
ALL_MODES = ("fp32", "bf16x3", "bank", "book", "book-all", "nograd")
TILE_MODES = ("bank", "book", "nograd")
FALLBACK_MODES = ("fp32", "bf16x3", "bank", "nograd")
BOOK_PASSES = ("1", "2", "3", "restored", "after")

Case = collections.namedtuple("Case", "id tier C step B H W seed modes")
CASES = [
    # Tier A: the smallest maps each route still runs on; seeds found on the CPU (tests/test_residual_control_host.py re-checks them)
    Case("a-64-s1-b1-1x4", "A", 64, 1, 1, 1, 4, 96, ALL_MODES),            # one row, one quad per row
    Case("a-64-s2-b1-2x4", "A", 64, 2, 1, 2, 4, 163, ALL_MODES),            # two rounds: the image handed from round to round
    Case("a-64-s2-b2-2x4", "A", 64, 2, 2, 2, 4, 181, ALL_MODES),            # ... and two samples: [step, B, C] scales
    Case("a-128-s1-b1-2x4", "A", 128, 1, 1, 2, 4, 185, ALL_MODES),          # C != 64: two channel blocks per group, never batched
    Case("a-64-s2-b1-2x6", "A", 64, 2, 1, 2, 6, 105, ALL_MODES),            # W % 4 != 0: no images even with a book
    Case("a-64-s1-b2-4x4", "A", 64, 1, 2, 4, 4, 153, ALL_MODES),            # a whole 4-row tile per sample
    Case("a-64-s1-b1-3x3-fallback", "A", 64, 1, 1, 3, 3, 250, FALLBACK_MODES),     # H * W % 4 != 0: not even the fused stage
    Case("a-32-s1-b1-2x4-fallback", "A", 32, 1, 1, 2, 4, 25, FALLBACK_MODES),     # C % 64 != 0
    # Tier B: tile geometry at slope 1.0 (and the output alone at slope 0.01)
    Case("b-64-s2-b2-40x64", "B", 64, 2, 2, 40, 64, 0, TILE_MODES),          # exactly 40 tiles: batched
    Case("b-64-s2-b2-36x64", "B", 64, 2, 2, 36, 64, 1, TILE_MODES),          # 36 tiles: not batched
    Case("b-64-s1-b1-37x100", "B", 64, 1, 1, 37, 100, 2, TILE_MODES),        # ragged rows and segments, 40 tiles
    Case("b-128-s1-b1-13x36", "B", 128, 1, 1, 13, 36, 3, TILE_MODES),
    Case("b-64-s1-b2-10x34", "B", 64, 1, 2, 10, 34, 4, TILE_MODES),          # W % 4 != 0
]
BY_ID = {c.id: c for c in CASES}
SLOPES = {"A": (0.01,), "B": (1.0, 0.01)}


def batched(C, B, H, W):
    """rc_fused.ResidualControlFn.backward: the three weight gradients of a round leave as one launch."""
    return C == 64 and B * math.ceil(H / 4) * math.ceil(W / 32) >= 40


def node_usable(case):
    """rc_fused.usable as far as the shape decides it."""
    return (case.H * case.W) % 4 == 0 and case.C % 64 == 0


def make_module(case, slope):
    from ebfi_amd.model import ResidualControl
    rc = ResidualControl(BLinch=1, Tinch=1, Basech=case.C, step=case.step)
    for bank in (rc.Conv1, rc.Conv2, rc.Conv3, rc.Conv4, rc.Conv5):
        for seq in bank:
            for layer in seq:
                layer.activation.negative_slope = slope
    return rc


def _init(rc):
    """O(1) activations at any depth, as the detail-stage test: weights randn * sqrt(1.5 / fan_in), biases 0.1 * randn."""
    with torch.no_grad():
        for p in rc.parameters():
            p.copy_(torch.randn_like(p) * (0.1 if p.dim() == 1 else (1.5 / p[0].numel()) ** 0.5))


def restatement(sd, data, ex, t, step, slope):
    """ResidualControl from a state_dict: per round x <- Conv5(cat(Conv1(ex) * Conv3(x) + x, Conv2(t) * Conv4(x) + x)), every layer
    conv + bias + LeakyReLU(slope)."""
    def layer(name, x, pad):
        return F.leaky_relu(F.conv2d(x, sd[name + ".conv2d.weight"], sd[name + ".conv2d.bias"], 1, pad), slope)
    ex, t, x = ex[:, :, None, None], t[:, :, None, None], data
    for i in range(step):
        a = layer("Conv3.%d.1" % i, layer("Conv3.%d.0" % i, x, 1), 1)
        b = layer("Conv4.%d.1" % i, layer("Conv4.%d.0" % i, x, 1), 1)
        x = layer("Conv5.%d.0" % i, torch.cat([layer("Conv1.%d.0" % i, ex, 0) * a + x, layer("Conv2.%d.0" % i, t, 0) * b + x], 1), 1)
    return x


@contextlib.contextmanager
def _recorded_kinks(out):
    """Every LeakyReLU evaluated inside appends min|z| / max|z| of its pre-activation to `out`."""
    leaky = F.leaky_relu

    def leaky_(z, *a, **k):
        m = z.detach().abs()
        out.append((m.min() / m.max()).item())
        return leaky(z, *a, **k)

    F.leaky_relu = leaky_
    try:
        yield out
    finally:
        F.leaky_relu = leaky


Reference = collections.namedtuple("Reference", "sd data ex t out g kink n_act")


def build_reference(case, slope, seed=None, backward=True):
    """The float64 CPU statement of `case` from its recorded seed (or `seed`): parameters, inputs, output, upstream gradient
    (gradients on the leaves' .grad when `backward`), and the smallest min|z| / max|z| over its activations."""
    gen_state = torch.random.get_rng_state()
    try:
        torch.manual_seed(case.seed if seed is None else seed)
        rc = make_module(case, slope)
        _init(rc)
        sd = {k: v.detach().double().clone().requires_grad_() for k, v in rc.state_dict().items()}
        data = torch.randn(case.B, case.C, case.H, case.W).double().requires_grad_()
        ex = torch.rand(case.B, 1).double().requires_grad_()
        t = torch.rand(case.B, 1).double().requires_grad_()
        kinks = []
        with _recorded_kinks(kinks):
            out = restatement(sd, data, ex, t, case.step, slope)
        g = torch.randn(out.shape).double()
        if backward:
            out.backward(g)
    finally:
        torch.random.set_rng_state(gen_state)
    return Reference(sd, data, ex, t, out.detach(), g, min(kinks), len(kinks))


_REFS = {}


def reference(case, slope):
    """Computed once per (case, slope), shared by every mode and the mutation test, never written to."""
    if (case.id, slope) not in _REFS:
        _REFS[(case.id, slope)] = build_reference(case, slope)
    return _REFS[(case.id, slope)]


def bounds(case, mode):
    if mode == "book-all":
        return BOOK_ALL
    n = 3 * case.step + 1
    return n * PER_LAYER[mode][0], n * PER_LAYER[mode][1]


def _rel(got, ref):
    return ((got.detach().cpu().double() - ref).abs().max() / ref.abs().max()).item()


# ------------------------------------------------------------------------------------------------------- the route of a pass
WATCHED = ("conv_fwd", "conv_wgrad", "scale_residual_cat", "to_c16")
X3 = "conv_fwd_bf16x3/"


def route_of(prof):
    """The watched launches of a pass, {label: launches}.  The split-precision convolution has two kernels behind one role (the
    wave-specialised _ws and, on few tiles, _db): both count under conv_fwd_bf16x3/<role>; likewise conv_wgrad_x3[_ws]."""
    r = collections.Counter()
    for k, n in prof.items():
        k = k.replace("conv_fwd_bf16x3_db/", X3).replace("conv_fwd_bf16x3_ws/", X3)
        k = "conv_wgrad_x3" if k == "conv_wgrad_x3_ws" else k
        if k.startswith(WATCHED) and k != "conv_wgrad_reduce_f32":
            r[k] += n
    return dict(r)


def expected_route(case, mode, what):
    """{label: launches} of pass `what` of `mode`.  what: "train" (fp32, bf16x3, bank), "nograd", or one of BOOK_PASSES /
    "all-1", "all-2"."""
    s, quads = case.step, case.W % 4 == 0
    stage = (case.H * case.W) % 4 == 0              # fused.scale_residual_cat takes planes of whole 16-byte vectors
    if what == "nograd":
        if not node_usable(case):                   # layer by layer, nothing kept
            r = {X3 + "fwd": 5 * s} if mode != "fp32" else {"conv_fwd_f32/fwd": 5 * s}
            return dict(r, scale_residual_cat_fwd=s) if stage else r
        if quads:
            return {X3 + "fwd": 2 * s, X3 + "fwd_rc": s}
        return {X3 + "fwd": 3 * s, "scale_residual_cat_fwd": s}
    both = {"scale_residual_cat_fwd": s, "scale_residual_cat_bwd": s}
    if mode == "fp32" or mode == "bf16x3" or not node_usable(case):
        if mode == "fp32":
            r = {"conv_fwd_f32/fwd": 5 * s, "conv_fwd_f32/dgrad": 5 * s, "conv_wgrad_f32": 5 * s}
        else:
            r = {X3 + "fwd": 5 * s, X3 + "dgrad": 5 * s, "conv_wgrad_x3": 5 * s}
        return dict(r, **both) if stage else r
    # the node's split-precision data gradients are forward launches on the transposed images: they count under .../fwd
    if mode == "bank":
        return dict({X3 + "fwd": 6 * s, "conv_wgrad_x3": 3 * s}, **both)
    if what in ("1", "all-1") or not quads:         # fp16 gradient kernels on fp32 tensors
        if quads:
            return dict({X3 + "fwd": 3 * s, "conv_fwd_f16_ws/f32_f32": 3 * s, "conv_wgrad_f16_tr/f32": 3 * s}, **both)
        return dict({X3 + "fwd": 6 * s, "conv_wgrad_f16_ws": 3 * s}, **both)
    # images: x and the upstream gradient converted once; per round the data gradients of Conv5 (fp32 out), of the grouped layer
    # (image out) and of the merged first layers (image out, fp32 in the first round)
    r = {"to_c16": 2, "scale_residual_cat_bwd": s, "conv_fwd_f16_ws/img_f32": s + 1, "conv_fwd_f16_ws/img_img": 2 * s - 1}
    if batched(case.C, case.B, case.H, case.W):
        r["conv_wgrad_f16_tr/img_batch"] = s
    else:
        r["conv_wgrad_f16_tr/img"] = 3 * s
    if what == "all-2":                             # fp16-operand forward: every convolution reads an image
        r["conv_fwd_f16_ws/img_both"] = 2 * s - 1
        r["conv_fwd_f16_ws/img_f32"] += s + 1
        r["scale_residual_cat_fwd"] = s
        return r
    r[X3 + "fwd_img"] = 2 * s - 1                   # (the last round's Conv5 writes no image)
    if what == "restored":
        r[X3 + "fwd"] = s + 1
        r["scale_residual_cat_fwd"] = s
    else:
        r[X3 + "fwd"] = 1
        r[X3 + "fwd_rc"] = s
    return r


# ------------------------------------------------------------------------------------------------------------ the device runs
Pass = collections.namedtuple("Pass", "what errs route packs guard finite")


class Device:
    """`case` on the GPU in `mode`: the module, its bank and scale book live across the passes of one mode."""

    def __init__(self, case, mode, slope):
        from ebfi_amd import conv, f16scale, weightbank
        self.case, self.mode, self.slope = case, mode, slope
        self.ref = reference(case, slope)
        rc = make_module(case, slope)
        rc.load_state_dict({k: v.detach().float() for k, v in self.ref.sd.items()})
        self.rc = rc.cuda().train()
        self.g = self.ref.g.float().cuda()
        self.bank = self.book = None
        conv.set_compute_dtype("fp32" if mode == "fp32" else "bf16x3")
        if mode not in ("fp32", "bf16x3"):
            self.bank = weightbank.build_for(self.rc, fwd16="all" if mode == "book-all" else None)
            if mode in ("book", "book-all"):
                self.book = f16scale.ScaleBook("cuda")
                if mode == "book-all":
                    self.book.forward_f16 = "all"
                self.bank.attach_scale_book(self.book)

    def drop_a_slots(self):
        """As slots restored from an earlier state: the image of `a` was never measured."""
        from ebfi_amd import rc_fused
        with self.bank.active():
            sites = rc_fused.sites_of(self.rc)
        for _, sb, _ in sites:
            self.book.calibrated.discard(self.book.index[(sb.key, "a")])

    def all_calibrated(self):
        return len(self.book.index) > 0 and self.book.calibrated == set(self.book.index.values())

    def run(self, what, grad=True):
        from ebfi_amd import _native as N
        case, ref, rc = self.case, self.ref, self.rc
        rc.zero_grad(set_to_none=True)
        data, ex, t = (v.detach().float().cuda().requires_grad_(grad) for v in (ref.data, ref.ex, ref.t))
        N.prof_reset()
        N.prof_enable(True)
        try:
            with contextlib.ExitStack() as ctx:
                if self.bank is not None:
                    self.bank.ensure_fresh()
                    ctx.enter_context(self.bank.active())
                if self.book is not None:
                    self.book.begin_step()
                    ctx.enter_context(self.book.active())
                if not grad:
                    ctx.enter_context(torch.no_grad())
                out = rc(data, ex, t)
                if grad:
                    out.backward(self.g)
                if self.book is not None:
                    self.book.finish()
            torch.cuda.synchronize()
        finally:
            N.prof_enable(False)
        prof = {k: v[0] for k, v in N.prof_collect().items() if v[0] > 0}
        b_out, b_grad = bounds(case, "nograd" if not grad else self.mode)
        assert out.shape == ref.out.shape
        errs = {"out": (_rel(out, ref.out), b_out)}
        finite = bool(torch.isfinite(out).all())
        if grad:
            named = dict(rc.named_parameters())
            assert set(named) == set(ref.sd)
            got = [("grad data", data.grad, ref.data.grad), ("grad Ex", ex.grad, ref.ex.grad), ("grad T", t.grad, ref.t.grad)]
            got += [("grad " + n, named[n].grad, q.grad) for n, q in ref.sd.items()]
            for name, a, b in got:
                assert a is not None and b is not None and a.shape == b.shape, name
                errs[name] = (_rel(a, b), b_grad)
                finite = finite and bool(torch.isfinite(a).all())
        guard = int(self.book.guard[0].item()) if self.book is not None else None
        return Pass(what, errs, route_of(prof), prof.get("conv_pack_w_bf16", 0), guard, finite)


def passes_of(case, mode, slope):
    """Every pass of `mode`, in order (a generator: the test checks each pass before the next one runs)."""
    from ebfi_amd import conv
    try:
        dev = Device(case, mode, slope)
        if mode == "nograd":
            yield dev.run("nograd", grad=False)
        elif mode == "book" and node_usable(case):
            for what in BOOK_PASSES:
                if what == "restored":
                    dev.drop_a_slots()
                    assert not dev.all_calibrated()
                yield dev.run(what)
                assert dev.all_calibrated(), what       # pass 1 measures every slot, the restored pass re-measures `a`
        elif mode == "book-all" and node_usable(case):
            yield dev.run("all-1")
            yield dev.run("all-2")
        else:
            yield dev.run("train")
    finally:
        conv.set_compute_dtype("fp32")


def compared(case, slope, p):
    """Tier B at slope 0.01 compares the output alone (the forward does not feel kinks)."""
    return p.errs if slope == SLOPES[case.tier][0] else {"out": p.errs["out"]}


def _report(case, mode, slope, p):
    tag = "%s %s/%s slope %g" % (case.id, mode, p.what, slope)
    held = compared(case, slope, p)
    for name, (e, b) in p.errs.items():
        note = "" if name in held else "  (not compared)"
        print("residual-control %-52s %-30s %.3e  bound %.1e  ratio %.3f%s" % (tag, name, e, b, e / b, note))
    worst = max(held, key=lambda n: held[n][0] / held[n][1])
    print("residual-control-worst %-52s out %.3e  grad %.3e  worst/bound %.3f (%s)  guard %s" % (
        tag, p.errs["out"][0], max([e for n, (e, _) in p.errs.items() if n != "out"] or [0.0]),
        held[worst][0] / held[worst][1], worst, p.guard))
    print("residual-control-route %-52s %s packs %d" % (tag, sorted(p.route.items()), p.packs))


def check_pass(case, mode, slope, p):
    """Route from the profile, guard, and the bound of every compared tensor."""
    assert p.route == expected_route(case, mode, p.what), (p.what, p.route, expected_route(case, mode, p.what))
    if mode == "fp32":
        assert p.packs == 0
    elif mode == "bf16x3":
        assert p.packs > 0                                      # weights packed per call
    else:
        assert p.packs == 0                                     # images from the bank
    if mode in ("book", "book-all"):
        assert p.guard == 0                                     # calibrated scales: nothing left fp16's range
    assert p.finite
    bad = {n: v for n, v in compared(case, slope, p).items() if not v[0] < v[1]}
    assert not bad, (p.what, bad)


PARAMS = [(c, m, s) for c in CASES for s in SLOPES[c.tier] for m in c.modes]


@pytest.mark.gpu
@pytest.mark.parametrize("case,mode,slope", PARAMS, ids=["%s-%s-slope%g" % (c.id, m, s) for c, m, s in PARAMS])
def test_residual_control_vs_float64(case, mode, slope):
    with contextlib.closing(passes_of(case, mode, slope)) as passes:     # (closed on a failure too: the compute mode is put back)
        for p in passes:
            _report(case, mode, slope, p)
            check_pass(case, mode, slope, p)


@pytest.mark.gpu
def test_the_checks_notice_exchanged_scales(monkeypatch):
    """The comparison bites: with the two scale tensors handed to ResidualControlFn.apply exchanged (same shapes, same addresses,
    wrong numbers) the output and the gradients of Conv1 / Conv2 each miss their bounds by at least 100 times, on the fp32 stage
    (bank) and on the epilogue tail (book pass 2)."""
    from ebfi_amd import rc_fused
    case = BY_ID["a-64-s2-b2-2x4"]
    real = rc_fused.ResidualControlFn.apply

    def exchanged(data, s_ex, s_t, *rest):
        return real(data, s_t, s_ex, *rest)

    monkeypatch.setattr(rc_fused.ResidualControlFn, "apply", staticmethod(exchanged))
    for mode, what in (("bank", "train"), ("book", "2")):
        with contextlib.closing(passes_of(case, mode, 0.01)) as passes:
            p = next(q for q in passes if q.what == what)
        assert p.route == expected_route(case, mode, what)
        for name in ["out"] + [n for n in p.errs if n.startswith(("grad Conv1.", "grad Conv2."))]:
            e, b = p.errs[name]
            print("residual-control-mutant %-8s %-30s error / bound %.1f" % (mode, name, e / b))
            assert e >= 100 * b, (mode, name, e, b)
