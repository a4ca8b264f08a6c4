"""Every stage of the detail branch (ebfi_amd.model.UNet3d_18: ebfi_amd/fold3d.py on the 2-D convolution kernels, csrc/segate.hip
for the gates) against the stage's own module in float64 on the CPU, where fold3d.usable is false and the module IS torch's
Conv3d / ConvTranspose3d / AdaptiveAvgPool3d / Sigmoid.  Output, input gradients and every parameter gradient, in the four ways a
convolution of the branch can be routed: exact fp32 kernels, split precision packing per call, split precision from the weight
bank, and the bank with a scale book (fp16 weight / data gradients where the folded shape qualifies).

CASES is also read by tests/test_detail_folds_host.py, which rebuilds every float64 reference on the CPU and asserts the kink
condition below for the recorded seed: importing this module needs no GPU.

Kink condition.  A ReLU / LeakyReLU pre-activation that the device rounds to the other side of zero gives a different, equally
valid subgradient, and at these sizes one flipped element moves a weight gradient by percents.  A case is therefore valid only
if, in the float64 reference, every activation's pre-activation z has |z| >= KINK * max|z| (1e-4: 5 times the per-layer forward
bound).  Each case records a seed (found among 0..255 on the CPU) for which this holds.

Bounds (error of a tensor: max|got - ref| / max|ref| against float64).  Per convolution layer they are the ones
tests/test_gpu_conv.py holds these kernels to (PER_LAYER); a stage whose longest chain has L convolutions gets (L + 1) times
those -- first-order error sum, the extra one for the gate.  The whole branch gets the TOL of
test_gpu_model.py::test_gradients_vs_reference_fixture (1e-3) without a scale book and the packed-gradient bound (5e-3) with one,
now per tensor against float64.  They are ceilings taken from the project, not fitted to what was measured.
"""
import collections
import contextlib
import re

import pytest
import torch
import torch.nn as nn
import torch.nn.functional as F

KINK = 1e-4
MODES = ("fp32", "bf16x3", "bank", "book")
#                   output, gradients
PER_LAYER = {"fp32": (2e-5, 5e-5), "bf16x3": (2e-5, 2e-4), "bank": (2e-5, 2e-4), "book": (1e-4, 1e-3)}
WHOLE = {"fp32": 1e-3, "bf16x3": 1e-3, "bank": 1e-3, "book": 5e-3}
# Measured on an MI355X with the seeds below: the output's error / the worst gradient's error per mode, and the largest
# error / bound over all tensors and modes of the stage (every bound holds with a factor of 5 or more to spare; none was raised):
#   stage                    fp32 out / grad      bf16x3 out / grad    bank out / grad      book out / grad      worst / bound
#   stem-16-9x7              3.8e-07 / 2.8e-07  3.8e-07 / 5.1e-06  3.8e-07 / 5.1e-06  3.8e-07 / 5.1e-06    0.01
#   block-16-8x12            1.7e-07 / 4.0e-07  2.4e-06 / 8.2e-06  2.4e-06 / 8.2e-06  2.4e-06 / 4.4e-04    0.15
#   block-24-4x8             2.0e-07 / 5.6e-07  2.8e-06 / 7.6e-06  2.8e-06 / 7.6e-06  2.8e-06 / 4.7e-04    0.16
#   block-32-2x2             1.2e-07 / 6.6e-07  1.1e-06 / 1.3e-05  1.1e-06 / 1.3e-05  1.1e-06 / 5.5e-04    0.18
#   block-48-5x6             3.9e-07 / 6.3e-07  2.7e-06 / 9.4e-06  2.7e-06 / 9.4e-06  2.7e-06 / 9.4e-06    0.04
#   block-16to24-s2-9x7      1.1e-07 / 4.1e-07  6.0e-06 / 6.8e-06  6.0e-06 / 6.8e-06  6.0e-06 / 4.2e-04    0.14
#   block-24to32-s2-8x12     1.9e-07 / 5.3e-07  1.1e-05 / 7.1e-06  1.1e-05 / 7.1e-06  1.1e-05 / 3.4e-04    0.18
#   block-32to48-4x8         2.1e-07 / 8.2e-07  6.2e-06 / 9.3e-06  6.2e-06 / 9.3e-06  6.2e-06 / 4.3e-04    0.14
#   conv3d-96to32-4x8        2.1e-06 / 6.8e-07  3.8e-06 / 5.7e-06  3.8e-06 / 5.7e-06  3.8e-06 / 3.1e-04    0.15
#   conv3d-24to16-5x6        5.6e-07 / 4.3e-07  3.6e-06 / 7.1e-06  3.6e-06 / 7.1e-06  3.6e-06 / 7.1e-06    0.09
#   up-32to16-4x8            4.9e-07 / 5.7e-07  6.0e-06 / 6.8e-06  6.0e-06 / 6.8e-06  6.0e-06 / 3.3e-04    0.16
#   up-24to16-9x7            5.6e-07 / 6.1e-07  5.0e-06 / 5.5e-06  5.0e-06 / 5.5e-06  5.0e-06 / 5.5e-06    0.13
#   tail-16-4x8              9.8e-07 / 5.6e-07  7.7e-06 / 1.0e-05  7.7e-06 / 1.0e-05  7.7e-06 / 2.9e-04    0.10
#   tail-24-5x6              8.6e-07 / 8.4e-07  8.1e-06 / 9.2e-06  8.1e-06 / 9.2e-06  8.1e-06 / 9.2e-06    0.10
#   unet-16x16               4.8e-07 / 1.0e-06  9.7e-06 / 2.9e-05  9.7e-06 / 2.9e-05  9.7e-06 / 2.9e-05    0.03
#   unet-16x24               5.1e-07 / 1.9e-06  1.0e-05 / 2.6e-05  1.0e-05 / 2.6e-05  1.0e-05 / 2.6e-05    0.03

# kind, args: what make_stage builds.  L: convolutions on the longest chain.  f16: how many (weight gradients, data gradients)
# conv._site_backward must run on the fp16 kernels with a scale book -- counted by hand from its rules over the stage's 3x3
# stride-1 layers, by their folded input channels 2C and the row length W they see:
#   weight gradient: 2C % 64 == 0, or 2C >= 32 and W % 4 == 0        data gradient: 2C >= 48 and W % 4 == 0
#   2C = 32: weight gradient only     2C = 48: the data-gradient threshold     2C = 64: a whole 64-channel block, weight gradient
#   at any W     2C = 96: a whole block + a partial one, nothing without quad rows     (strided and 1x1 layers: never)
Case = collections.namedtuple("Case", "id kind args B H W L f16 seed")
CASES = [
    Case("stem-16-9x7", "stem", (16,), 2, 9, 7, 1, (0, 0), 11),                    # 3x7x7 stride (1,2,2) from an odd size
    Case("block-16-8x12", "block", (16, 16, 1), 2, 8, 12, 2, (2, 0), 249),        # folded 32
    Case("block-24-4x8", "block", (24, 24, 1), 1, 4, 8, 2, (2, 2), 11),          # folded 48
    Case("block-32-2x2", "block", (32, 32, 1), 1, 2, 2, 2, (2, 0), 25),           # folded 64 on the deepest plane of a 16x16 input
    Case("block-48-5x6", "block", (48, 48, 1), 2, 5, 6, 2, (0, 0), 25),            # folded 96, rows without quads
    Case("block-16to24-s2-9x7", "block", (16, 24, 2), 1, 9, 7, 2, (1, 1), 4),    # stride 2 from an odd size to 5x4, 1x1 strided shortcut
    Case("block-24to32-s2-8x12", "block", (24, 32, 2), 2, 8, 12, 2, (1, 0), 2),   # ... to 4x6: folded 64 without quads
    Case("block-32to48-4x8", "block", (32, 48, 1), 1, 4, 8, 2, (2, 2), 10),      # layer4's first block: unstrided 1x1 shortcut; 64, 96
    Case("conv3d-96to32-4x8", "conv3d", (96, 32), 1, 4, 8, 1, (1, 1), 6),        # concatenated input of 2 * 48 channels: folded 192
    Case("conv3d-24to16-5x6", "conv3d", (24, 16), 2, 5, 6, 1, (0, 0), 15),
    Case("up-32to16-4x8", "up", (32, 16), 2, 4, 8, 1, (1, 1), 82),               # even W: the gate reads through the pixel shuffle
    Case("up-24to16-9x7", "up", (24, 16), 1, 9, 7, 1, (0, 0), 49),                 # odd W: pixel_shuffle, then the plain gate
    Case("tail-16-4x8", "tail", (16,), 2, 4, 8, 3, (1, 1), 218),                 # decoder stage 4 -> fuse 1x1 -> reflect pad -> 7x7
    Case("tail-24-5x6", "tail", (24,), 1, 5, 6, 3, (0, 0), 228),
    Case("unet-16x16", "unet", ((4, 6, 8, 10),), 1, 16, 16, None, (0, 0), 254),    # the wiring: skip order, concatenations, fuse permutation
    Case("unet-16x24", "unet", ((4, 6, 8, 10),), 1, 16, 24, None, (0, 0), 136),
]
BY_ID = {c.id: c for c in CASES}


class _Pass(nn.Module):
    """Stands in for decoder stages 0..3 of a UNet3d_18 whose tail alone is under test."""

    def forward(self, y, post_act=None):
        return y


class _NoEncoder(nn.Module):
    """Stands in for the encoder: the stacked input is the decoder's input, the four skips have no channels."""

    def forward(self, x):
        e = x[:, :0]
        return e, e, e, e, x


def make_stage(case):
    from ebfi_amd.model import BasicBlock, Conv_3d, UNet3d_18, identity, r3d_18, upConv3D
    up = dict(kernel_size=(3, 4, 4), stride=(1, 2, 2), padding=(1, 1, 1), upmode="transpose", bn=False)
    if case.kind == "stem":
        return r3d_18(bn=False, channels=[case.args[0]] * 4).stem
    if case.kind == "block":
        cin, planes, s = case.args
        ds, stride = None, 1
        if s != 1 or cin != planes:                      # as VideoResNet builds the first block of a layer
            stride = (1, s, s)
            ds = nn.Sequential(nn.Conv3d(cin, planes, kernel_size=1, stride=stride, bias=False), identity(planes))
        return BasicBlock(cin, planes, stride, ds, False)
    if case.kind == "conv3d":
        return Conv_3d(case.args[0], case.args[1], kernel_size=3, padding=1, bias=True, bn=False)
    if case.kind == "up":
        return upConv3D(case.args[0], case.args[1], **up)
    if case.kind == "tail":
        c0 = case.args[0]
        net = UNet3d_18(channels=[c0, c0, c0, c0], bn=False)
        net.encoder = _NoEncoder()
        for i in range(4):
            net.decoder[i] = _Pass()
        return net
    if case.kind == "unet":
        return UNet3d_18(channels=list(case.args[0]), bn=False)
    raise ValueError(case.kind)


def _init(stage):
    """O(1) activations at any depth: randn * sqrt(1.5 / fan_in); gates as in test_gpu_model.py's gate tests."""
    with torch.no_grad():
        for name, p in stage.named_parameters():
            if "attn_layer" in name:
                p.copy_(torch.randn_like(p) * (0.5 if p.dim() > 1 else 0.3))
            elif p.dim() == 1:
                p.copy_(torch.randn_like(p) * 0.1)
            else:
                fan_in = p[0].numel()
                if p.dim() == 5 and p.shape[2:] == (3, 4, 4):        # ConvTranspose3d [Ci, Co, 3, 4, 4]: 2x2 of the 4x4 taps per output
                    fan_in = p.shape[0] * 3 * 4
                p.copy_(torch.randn_like(p) * (1.5 / fan_in) ** 0.5)


def _inputs(case):
    B, H, W = case.B, case.H, case.W
    if case.kind == "stem":
        return [torch.randn(B, 3, 2, H, W)]
    if case.kind == "unet":
        return [torch.rand(B, 3, H, W), torch.rand(B, 3, H, W)]        # two frames in [0, 1)
    cin = 2 * case.args[0] if case.kind == "tail" else case.args[0]
    return [torch.randn(B, cin, 2, H, W)]


def forward(case, stage, xs):
    """The stage as UNet3d_18 / VideoResNet run it: on CPU tensors this is torch's own 3-D modules."""
    x = xs[0]
    if case.kind == "stem":
        if x.is_cuda:                                    # VideoResNet.forward's line for a stem without a norm
            from ebfi_amd import conv, fold3d
            assert fold3d.usable(x)
            return fold3d.conv3d_d2(x, stage[0], conv.ACT_LEAKY, 0.0)
        return stage(x)
    if case.kind == "block":
        return stage(x)
    if case.kind in ("conv3d", "up"):
        return stage(x, 0.2)
    if case.kind == "tail":
        if x.is_cuda:                                    # UNet3d_18.forward itself, from decoder stage 4 on
            return stage(x[:, :, 0], x[:, :, 1])
        y = F.leaky_relu(stage.decoder[4].upconv(x), 0.2)
        y = torch.cat(torch.unbind(y, 2), 1)
        y = F.leaky_relu(stage.feature_fuse[0](y), 0.2)
        return stage.outconv[1](nn.ReflectionPad2d(3)(y))
    return stage(xs[0], xs[1])


@contextlib.contextmanager
def _recorded_kinks(out):
    """Every ReLU / LeakyReLU evaluated inside appends min|z| / max|z| of its pre-activation to `out`."""
    relu, leaky = F.relu, F.leaky_relu

    def note(z):
        a = z.detach().abs()
        out.append((a.min() / a.max()).item())

    def relu_(z, *a, **k):
        note(z)
        return relu(z, *a, **k)

    def leaky_(z, *a, **k):
        note(z)
        return leaky(z, *a, **k)

    F.relu, F.leaky_relu = relu_, leaky_
    try:
        yield out
    finally:
        F.relu, F.leaky_relu = relu, leaky


Reference = collections.namedtuple("Reference", "stage xs out g kink n_act")


def build_reference(case, seed=None, backward=True):
    """The float64 CPU statement of `case` from its recorded seed (or `seed`): module, inputs, output, upstream gradient
    (gradients on the inputs' and parameters' .grad when `backward`), and the smallest min|z| / max|z| over its activations."""
    gen_state = torch.random.get_rng_state()
    try:
        torch.manual_seed(case.seed if seed is None else seed)
        stage = make_stage(case)
        _init(stage)
        stage = stage.double()
        xs = [x.double().requires_grad_() for x in _inputs(case)]
        kinks = []
        with _recorded_kinks(kinks):
            out = forward(case, stage, xs)
        g = torch.randn(out.shape).double()
        if backward:
            out.backward(g)
    finally:
        torch.random.set_rng_state(gen_state)
    return Reference(stage, xs, out.detach(), g, min(kinks), len(kinks))


_REFS = {}


def reference(case):
    """Computed once per case, shared by the four modes and the sensitivity test, never written to."""
    if case.id not in _REFS:
        _REFS[case.id] = build_reference(case)
    return _REFS[case.id]


def bounds(case, mode):
    if case.kind == "unet":
        return WHOLE[mode], WHOLE[mode]
    return (case.L + 1) * PER_LAYER[mode][0], (case.L + 1) * PER_LAYER[mode][1]


def _rel(got, ref):
    return ((got.detach().cpu().double() - ref).abs().max() / ref.abs().max()).item()


def run_device(case, mode):
    """`case` on the GPU in `mode`: ({tensor name: (error, bound)}, {kernel label: launches}, the scale book's guard flag or None,
    the kinds of weight-bank site the stage's convolutions found)."""
    from ebfi_amd import _native as N
    from ebfi_amd import conv, f16scale, weightbank
    ref = reference(case)
    stage = make_stage(case)
    stage.load_state_dict(ref.stage.state_dict())
    stage = stage.float().cuda()
    xs = [x.detach().float().cuda().requires_grad_() for x in ref.xs]
    g = ref.g.float().cuda()
    bank = book = None
    hits, lookup = set(), weightbank.lookup

    def noted_lookup(param, kind="id"):                  # which kinds of bank site the stage found
        site = lookup(param, kind)
        if site is not None:
            hits.add(kind)
        return site

    conv.set_compute_dtype("fp32" if mode == "fp32" else "bf16x3")
    weightbank.lookup = noted_lookup
    try:
        if mode in ("bank", "book"):
            bank = weightbank.build_for(stage)
            if mode == "book":
                book = f16scale.ScaleBook("cuda")
                bank.attach_scale_book(book)
        N.prof_reset()
        N.prof_enable(True)
        with contextlib.ExitStack() as ctx:
            if bank is not None:
                bank.ensure_fresh()
                ctx.enter_context(bank.active())
            if book is not None:
                ctx.enter_context(book.active())
            out = forward(case, stage, xs)
            out.backward(g)
            if book is not None:
                book.finish()
        torch.cuda.synchronize()
        N.prof_enable(False)
        prof = {k: v[0] for k, v in N.prof_collect().items() if v[0] > 0}
    finally:
        N.prof_enable(False)
        weightbank.lookup = lookup
        conv.set_compute_dtype("fp32")
    b_out, b_grad = bounds(case, mode)
    assert out.shape == ref.out.shape
    errs = {"out": (_rel(out, ref.out), b_out)}
    for i, (xd, xr) in enumerate(zip(xs, ref.xs)):
        errs["grad_in%d" % i] = (_rel(xd.grad, xr.grad), b_grad)
    named = dict(stage.named_parameters())
    assert set(named) == set(dict(ref.stage.named_parameters()))
    for n, q in ref.stage.named_parameters():
        assert q.grad is not None and named[n].grad is not None, n
        errs["grad " + n] = (_rel(named[n].grad, q.grad), b_grad)
    guard = int(book.guard[0].item()) if book is not None else None
    return errs, prof, guard, hits


def _count(prof, prefix):
    return sum(v for k, v in prof.items() if k == prefix or k.startswith(prefix + "/") or k.startswith(prefix + "_"))


SITES = {"stem": set(), "block": {"conv3d"}, "conv3d": {"conv3d"}, "up": {"convT3d"},
         "tail": {"convT3d", "fuse_d2"},                 # (the fuse through "fuse_d2", never through its plain 1x1 "id" site)
         "unet": {"conv3d", "convT3d", "fuse_d2"}}


def check_route(case, mode, prof, hits):
    """Each mode ran on the kernels it names."""
    packs, table = prof.get("conv_pack_w_bf16", 0), prof.get("pack_table_bf16", 0)
    f16 = {k for k in prof if re.search(r"(?<!b)f16", k)}
    split = {k for k in prof if "bf16" in k or "_x3" in k}
    if mode == "fp32":                                          # exact kernels alone
        assert not f16 and not split and not hits, prof
    elif mode == "bf16x3":                                      # a folded weight packed per call, forward and transposed
        assert table == 0 and not f16 and not hits, prof
        assert (packs > 0 and "conv_fwd_bf16x3_db/fwd" in prof) or case.kind == "stem", prof    # (the strided stem stays exact)
    else:                                                       # images from the bank's one pack launch
        assert hits == SITES[case.kind], hits
        assert packs == 0 and table == (1 if hits else 0), prof
        assert "conv_fwd_bf16x3_db/fwd" in prof or case.kind == "stem", prof
    if mode == "book":
        assert (_count(prof, "conv_wgrad_f16"), _count(prof, "conv_fwd_f16_ws")) == case.f16, prof
    else:
        assert not f16, prof
    if case.kind == "up":                                       # the gate through the shuffle needs an even W
        shuffled, plain = prof.get("se_gate_fwd/shuffle", 0), prof.get("se_gate_fwd", 0)
        assert (shuffled, plain) == ((1, 0) if case.W % 2 == 0 else (0, 1)), prof
        assert prof.get("se_gate_bwd/shuffle" if case.W % 2 == 0 else "se_gate_bwd", 0) == 1, prof
    elif case.kind != "stem":
        assert _count(prof, "se_gate_fwd") > 0 and _count(prof, "se_gate_bwd") > 0, prof


def _report(case, mode, errs):
    for name, (e, b) in errs.items():
        print("detail-stage %-22s %-7s %-44s %.3e  bound %.1e  ratio %.3f" % (case.id, mode, name, e, b, e / b))
    worst = max(errs, key=lambda n: errs[n][0] / errs[n][1])
    print("detail-stage-worst %-22s %-7s out %.3e  grad %.3e  worst/bound %.3f (%s)" % (
        case.id, mode, errs["out"][0], max(e for n, (e, _) in errs.items() if n != "out"), errs[worst][0] / errs[worst][1], worst))


@pytest.mark.gpu
@pytest.mark.parametrize("mode", MODES)
@pytest.mark.parametrize("case", CASES, ids=[c.id for c in CASES])
def test_stage_vs_float64_module(case, mode):
    errs, prof, guard, hits = run_device(case, mode)
    _report(case, mode, errs)
    print("detail-stage-prof %-22s %-7s %s" % (case.id, mode, sorted(prof.items())))
    check_route(case, mode, prof, hits)
    if mode == "book":
        assert guard == 0                                       # calibrated scales: nothing left fp16's range
    bad = {n: v for n, v in errs.items() if not v[0] < v[1]}
    assert not bad, bad


@pytest.mark.gpu
def test_the_checks_notice_a_wrong_fold(monkeypatch):
    """The comparison bites: a Conv3d fold with its two output-depth slices exchanged, and a bias repeated as (b, b) instead of
    depth-minor (b0, b0, b1, b1, ...), each miss a bound by at least 100 times.  Both mutations keep every shape: wrong
    numbers, never another address."""
    from ebfi_amd import fold3d
    real = fold3d.fold_conv3d_weight

    def swapped_depth(w):
        w2 = real(w)
        return w2.view(w.shape[0], 2, *w2.shape[1:]).flip(1).reshape(w2.shape)

    fold3d._MAPS.clear()
    try:
        for cid, name, mutant in (("block-24-4x8", "fold_conv3d_weight", swapped_depth),
                                  ("conv3d-24to16-5x6", "_rep2", lambda b: b.repeat(2))):
            with monkeypatch.context() as mp:
                mp.setattr(fold3d, name, mutant)
                fold3d._MAPS.clear()
                for mode in ("fp32", "bf16x3"):
                    errs, _, _, _ = run_device(BY_ID[cid], mode)
                    miss = max(e / b for e, b in errs.values())
                    print("detail-stage-mutant %-22s %-7s %-20s worst/bound %.1f" % (cid, mode, name, miss))
                    assert miss >= 100, (cid, mode, errs)
            fold3d._MAPS.clear()
    finally:
        fold3d._MAPS.clear()
