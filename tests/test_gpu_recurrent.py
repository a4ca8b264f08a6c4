"""The recurrent U-Nets on the device (csrc/recurrent.hip, ebfi_amd.recurrent, ebfi_amd.unet): the cell and up-sampling kernels
through the C ABI, the whole nets against tests/unet_ref.py in float64, reproducibility, the strict-native switch, a graph
capture and UNetFlow under the event-warping loss.

Accuracy bars are MEASURED, not fixed (the rule of tests/test_gpu_stgan.py): for every output, e = max |x - x64| / max |x64|
against the float64 law; the yardstick e32 is the same law evaluated by torch on the CPU in float32 (for the whole nets:
tests/unet_ref.py in float32); pass when e <= max(4 e32, 4 * 2^-23).  Here only libm's last-ulp differences separate the two,
and for the up-sampling only contraction and summation order.  In bf16x3 compute mode the bar is the project's whole-model one
for that mode, 1e-3 of each tensor's scale.  Every figure is printed (`recurrent-accuracy ...`); profiles/recurrent.md keeps a run.
"""
import os
import sys

import numpy as np
import pytest
import torch
import torch.nn.functional as F

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import unet_ref as R  # noqa: E402

from ebfi_amd import _native as N  # noqa: E402
from ebfi_amd import conv  # noqa: E402

pytestmark = pytest.mark.gpu

FACTOR, ULP = 4.0, 2.0 ** -23
CELL_SHAPES = [(1, 1, 1, 1), (2, 3, 5, 7), (1, 8, 2, 2), (2, 16, 33, 4)]
UP_SHAPES = [(1, 1, 1, 1), (2, 3, 5, 7), (1, 2, 9, 33)]


def _rel(x, x64):
    x, x64 = np.asarray(x, dtype=np.float64), np.asarray(x64, dtype=np.float64)
    scale = float(np.abs(x64).max())
    return float(np.abs(x - x64).max()) / scale if scale > 0 else float(np.abs(x).max())


def _measure(tag, key, got, want64, yard32, failures, fixed=None):
    """fixed=None: the measured bar; else that fraction of the tensor's scale."""
    got = got.detach().cpu().numpy() if torch.is_tensor(got) else got
    e, e32 = _rel(got, want64.detach().numpy()), _rel(yard32.detach().numpy(), want64.detach().numpy())
    bar = max(FACTOR * e32, FACTOR * ULP) if fixed is None else fixed
    print("recurrent-accuracy %-34s %-44s e=%.3e e32=%.3e bar=%.3e" % (tag, key, e, e32, bar))
    if not e <= bar:
        failures.append((tag, key, e, e32, bar))


def _draw(rs, shape, spread=1.0):
    return torch.from_numpy((spread * rs.standard_normal(shape)).astype(np.float32))


def _dev(t):
    return None if t is None else t.cuda().contiguous()


def _grads(outs, cots, leaves):
    """d sum(cot * out) / d leaves, None leaves skipped; a None cotangent drops its output."""
    loss = sum((c.to(o.dtype) * o).sum() for o, c in zip(outs, cots) if c is not None)
    present = [l for l in leaves if l is not None]
    got = iter(torch.autograd.grad(loss, present, allow_unused=True))
    return [None if l is None else next(got) for l in leaves]


def _sig(v):
    return 1 / (1 + torch.exp(-v))


# ------------------------------------------------------------------------------------------------------------ the laws
def lstm_law(gates, prev_cell):
    gi, gf, go, gc = gates.chunk(4, 1)
    cell = _sig(gi) * torch.tanh(gc)
    if prev_cell is not None:
        cell = _sig(gf) * prev_cell + cell
    return _sig(go) * torch.tanh(cell), cell


def gru_reset_law(reset_pre, x, h):
    return torch.cat([x, h * _sig(reset_pre) if h is not None else torch.zeros_like(reset_pre)], 1)


def gru_update_law(update_pre, out_pre, h):
    u = _sig(update_pre)
    new = torch.tanh(out_pre) * u
    return new if h is None else h * (1 - u) + new


def _law(fn, inputs, cots, dtype):
    """outputs and input gradients of `fn` on CPU copies of `inputs` in `dtype`."""
    leaves = [None if t is None else t.detach().to(dtype).clone().requires_grad_(True) for t in inputs]
    outs = fn(*leaves)
    outs = outs if isinstance(outs, tuple) else (outs,)
    return [o.detach() for o in outs], _grads(outs, cots, leaves)


# ------------------------------------------------------------------------------------------------------------ cells, C ABI
@pytest.mark.parametrize("spread", [1.0, 8.0])
@pytest.mark.parametrize("shape", CELL_SHAPES)
def test_lstm_cell_kernels_against_float64(shape, spread):
    B, C, H, W = shape
    rs = np.random.RandomState(B * 1000 + C * 100 + H + int(spread))
    lib, st, failures = N.lib(), N.stream_ptr(), []
    gates, prev = _draw(rs, (B, 4 * C, H, W), spread), _draw(rs, shape)
    gh, gc = _draw(rs, shape), _draw(rs, shape)
    for with_prev in (True, False):
        pc = prev if with_prev else None
        for cots in ((gh, gc), (gh, None), (None, gc)):
            tag = "lstm %s s=%g prev=%d gh=%d gc=%d" % ("x".join(map(str, shape)), spread, with_prev, cots[0] is not None, cots[1] is not None)
            (h64, c64), (dg64, dp64) = _law(lstm_law, (gates, pc), cots, torch.float64)
            (h32, c32), (dg32, dp32) = _law(lstm_law, (gates, pc), cots, torch.float32)
            d = dict(gates=_dev(gates), prev=_dev(pc), gh=_dev(cots[0]), gc=_dev(cots[1]))
            hidden, cell = torch.empty(shape, device="cuda"), torch.empty(shape, device="cuda")
            N.check(lib.ebfi_lstm_cell_forward(N.ptr(d["gates"]), N.ptr(d["prev"]), N.ptr(hidden), N.ptr(cell), B, C, H * W, st), tag)
            dgates = torch.full((B, 4 * C, H, W), float("nan"), device="cuda")
            dprev = torch.full(shape, float("nan"), device="cuda") if with_prev else None
            N.check(lib.ebfi_lstm_cell_backward(N.ptr(d["gates"]), N.ptr(d["prev"]), N.ptr(cell), N.ptr(d["gh"]), N.ptr(d["gc"]),
                                                N.ptr(dgates), N.ptr(dprev), B, C, H * W, st), tag)
            _measure(tag, "hidden", hidden, h64, h32, failures)
            _measure(tag, "cell", cell, c64, c32, failures)
            _measure(tag, "grad_gates", dgates, dg64, dg32, failures)
            if with_prev:
                _measure(tag, "grad_prev_cell", dprev, dp64, dp32, failures)
            assert torch.equal(d["gates"].cpu(), gates)
    assert not failures, failures


@pytest.mark.parametrize("spread", [1.0, 8.0])
@pytest.mark.parametrize("shape", CELL_SHAPES)
def test_gru_kernels_against_float64(shape, spread):
    B, C, H, W = shape
    Cx = C + 1                                                  # (the nets have Cx == C; the kernel does not rely on it)
    rs = np.random.RandomState(B * 1000 + C * 100 + H + int(spread) + 7)
    lib, st, failures = N.lib(), N.stream_ptr(), []
    rp, up, op = (_draw(rs, shape, spread) for _ in range(3))
    x, hs = _draw(rs, (B, Cx, H, W)), _draw(rs, shape)
    g_cat, g_new, g_acc = _draw(rs, (B, Cx + C, H, W)), _draw(rs, shape), _draw(rs, shape)
    for with_h in (True, False):
        h = hs if with_h else None
        tag = "gru %s s=%g h=%d" % ("x".join(map(str, shape)), spread, with_h)
        # first half: cat(x, h * sigmoid(reset))
        (o64,), (dr64, dx64, dh64) = _law(gru_reset_law, (rp, x, h), (g_cat,), torch.float64)
        (o32,), (dr32, dx32, dh32) = _law(gru_reset_law, (rp, x, h), (g_cat,), torch.float32)
        d = dict(rp=_dev(rp), up=_dev(up), op=_dev(op), x=_dev(x), h=_dev(h), g_cat=_dev(g_cat), g_new=_dev(g_new), g_acc=_dev(g_acc))
        out = torch.full((B, Cx + C, H, W), float("nan"), device="cuda")
        N.check(lib.ebfi_gru_reset_forward(N.ptr(d["rp"]), N.ptr(d["x"]), N.ptr(d["h"]), N.ptr(out), B, Cx, C, H * W, st), tag)
        _measure(tag, "cat(x, h*r)", out, o64, o32, failures)
        assert torch.equal(out[:, :Cx].cpu(), x)                # the copied half is the input's bits
        for acc in (False, True):
            for want_x in (True, False):
                dx = torch.full((B, Cx, H, W), float("nan"), device="cuda") if want_x else None
                dr = torch.full(shape, float("nan"), device="cuda")
                dh = torch.full(shape, float("nan"), device="cuda") if with_h else None
                N.check(lib.ebfi_gru_reset_backward(N.ptr(d["g_cat"]), N.ptr(d["rp"]), N.ptr(d["h"]), N.ptr(d["g_acc"] if acc else None),
                                                    N.ptr(dx), N.ptr(dr), N.ptr(dh), B, Cx, C, H * W, st), tag)
                sub = "%s acc=%d" % (tag, acc)
                if with_h:
                    _measure(sub, "grad_reset_pre", dr, dr64, dr32, failures)
                    _measure(sub, "grad_h (reset)", dh, dh64 + (g_acc.double() if acc else 0), dh32 + (g_acc if acc else 0), failures)
                else:
                    assert not dr.any()                         # no state: the reset gate has no effect
                if want_x:
                    assert torch.equal(dx.cpu(), g_cat[:, :Cx])
        # second half
        (n64,), (du64, do64, dh64) = _law(gru_update_law, (up, op, h), (g_new,), torch.float64)
        (n32,), (du32, do32, dh32) = _law(gru_update_law, (up, op, h), (g_new,), torch.float32)
        new = torch.full(shape, float("nan"), device="cuda")
        N.check(lib.ebfi_gru_update_forward(N.ptr(d["up"]), N.ptr(d["op"]), N.ptr(d["h"]), N.ptr(new), B, C, H * W, st), tag)
        _measure(tag, "new_state", new, n64, n32, failures)
        for want_h in ((True, False) if with_h else (False,)):
            du, do = torch.full(shape, float("nan"), device="cuda"), torch.full(shape, float("nan"), device="cuda")
            dh = torch.full(shape, float("nan"), device="cuda") if want_h else None
            N.check(lib.ebfi_gru_update_backward(N.ptr(d["up"]), N.ptr(d["op"]), N.ptr(d["h"]), N.ptr(d["g_new"]), N.ptr(du), N.ptr(do),
                                                 N.ptr(dh), B, C, H * W, st), tag)
            _measure(tag, "grad_update_pre", du, du64, du32, failures)
            _measure(tag, "grad_out_pre", do, do64, do32, failures)
            if want_h:
                _measure(tag, "grad_h (update)", dh, dh64, dh32, failures)
    assert not failures, failures


# ------------------------------------------------------------------------------------------------------------ up-sampling
def _up_law(scale):
    return lambda x: F.interpolate(x, scale_factor=scale, mode="bilinear", align_corners=False)


@pytest.mark.parametrize("scale", [2, 4])
@pytest.mark.parametrize("shape", UP_SHAPES)
def test_bilinear_up_against_float64(shape, scale):
    B, C, H, W = shape
    rs = np.random.RandomState(B * 100 + C * 10 + H + scale)
    lib, st, failures = N.lib(), N.stream_ptr(), []
    x, g = _draw(rs, shape), _draw(rs, (B, C, scale * H, scale * W))
    tag = "bilinear x%d %s" % (scale, "x".join(map(str, shape)))
    (o64,), (dx64,) = _law(_up_law(scale), (x,), (g,), torch.float64)
    (o32,), (dx32,) = _law(_up_law(scale), (x,), (g,), torch.float32)
    out = torch.full(g.shape, float("nan"), device="cuda")
    N.check(lib.ebfi_bilinear_up_forward(N.ptr(_dev(x)), N.ptr(out), B * C, H, W, scale, st), tag)
    _measure(tag, "out", out, o64, o32, failures)
    gd = _dev(g)
    runs = []
    for _ in range(2):
        dx = torch.full(shape, float("nan"), device="cuda")
        N.check(lib.ebfi_bilinear_up_backward(N.ptr(gd), N.ptr(dx), B * C, H, W, scale, st), tag)
        runs.append(dx)
    _measure(tag, "grad_x", runs[0], dx64, dx32, failures)
    assert runs[0].cpu().numpy().tobytes() == runs[1].cpu().numpy().tobytes()        # a gather in a fixed order
    # the adjoint identity in float64 of the device's float32 results: <up(x), g> == <x, up^T(g)> to float32 rounding
    lhs, rhs = float((out.double().cpu() * g.double()).sum()), float((x.double() * runs[0].double().cpu()).sum())
    assert abs(lhs - rhs) <= 1e-5 * max(float((out.double().cpu() * g.double()).abs().sum()), 1e-30)
    # through the module function, with autograd
    from ebfi_amd.recurrent import bilinear_up
    xd = _dev(x).requires_grad_(True)
    y = bilinear_up(xd, scale)
    (gx,) = torch.autograd.grad(y, xd, gd)
    assert torch.equal(y, out) and torch.equal(gx, runs[0])
    assert not failures, failures


# ------------------------------------------------------------------------------------------------------------ whole nets
@pytest.fixture(scope="module")
def cases():
    """case -> (seed, xs, cots, float64 run, float32 run) of the restatement on the fixture's seeds: computed once, shared."""
    fixture = np.load(os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "unet_small.npz"))
    out = {}
    for i, case in enumerate(R.CASES):
        seed = int(fixture["seeds"][i])
        xs, cots = R.make_inputs(seed + 1000, case)
        state = R.fill_state(seed, case)
        out[case] = (seed, xs, cots, R.run(case, state, xs, cots), R.run(case, state, xs, cots, dtype=torch.float32))
    return out


def _net(case, seed):
    from models.model_misc import unet
    net = getattr(unet, R.CASES[case]["net"])(R.unet_kwargs(case))
    net.load_state_dict({k: v.float() for k, v in R.fill_state(seed, case).items()})
    return net.cuda()


def _two_calls(net, xs, cots, names):
    """Two consecutive calls from a fresh state, one backward -> (outs, final states, gradients in `names` order)."""
    net.states = [None] * net.num_encoders
    outs = [R.module_outputs(net(x)) for x in xs]
    loss = sum((c * o).sum() for c, o in zip(cots, outs))
    params = dict(net.named_parameters())
    grads = torch.autograd.grad(loss, [params[n] for n in names])
    return [o.detach() for o in outs], [s.detach() for s in R.flat_states(net.states)], list(grads)


def _device_run(case, seed, xs, cots):
    names = [n for n, _ in R.names_and_shapes(case)]
    net = _net(case, seed)
    return names, _two_calls(net, [x.float().cuda() for x in xs], [c.float().cuda() for c in cots], names)


def _compare(tag, names, got, ref64, ref32, fixed=None):
    failures = []
    outs, states, grads = got
    for c, o in enumerate(outs):
        _measure(tag, "out[%d]" % c, o, ref64["outs"][c], ref32["outs"][c], failures, fixed)
    assert len(states) == len(ref64["states"])
    for k, s in enumerate(states):
        _measure(tag, "state[%d]" % k, s, ref64["states"][k], ref32["states"][k], failures, fixed)
    for n, g in zip(names, grads):
        _measure(tag, "grad " + n, g, ref64["grads"][n], ref32["grads"][n], failures, fixed)
    return failures


@pytest.mark.parametrize("case", list(R.CASES))
def test_whole_net_fp32_against_float64(cases, case):
    seed, xs, cots, ref64, ref32 = cases[case]
    assert conv.get_compute_dtype() == "fp32"
    names, got = _device_run(case, seed, xs, cots)
    failures = _compare("net %s fp32" % case, names, got, ref64, ref32)
    assert not failures, failures


@pytest.mark.parametrize("case", list(R.CASES))
def test_whole_net_bf16x3_against_float64(cases, case):
    seed, xs, cots, ref64, ref32 = cases[case]
    before = conv.get_compute_dtype()
    conv.set_compute_dtype("bf16x3")
    try:
        names, got = _device_run(case, seed, xs, cots)
    finally:
        conv.set_compute_dtype(before)
    failures = _compare("net %s bf16x3" % case, names, got, ref64, ref32, fixed=1e-3)
    assert not failures, failures


def _bits(run):
    outs, states, grads = run
    return [t.cpu().numpy().tobytes() for t in outs + states + grads]


def test_two_runs_give_the_same_bits(cases):
    seed, xs, cots, _, _ = cases["A"]
    names = [n for n, _ in R.names_and_shapes("A")]
    net = _net("A", seed)
    xd, cd = [x.float().cuda() for x in xs], [c.float().cuda() for c in cots]
    first, second = _bits(_two_calls(net, xd, cd, names)), _bits(_two_calls(net, xd, cd, names))
    assert first == second and len(first) == 2 + 4 + len(names)


@pytest.mark.parametrize("case", ["A", "B", "D"])
def test_strict_native_forward_and_backward(cases, case, monkeypatch):
    """kernel_size=3, norm=None, use_upsample_conv=True: no convolution leaves the native kernels."""
    monkeypatch.setenv("EBFI_STRICT_NATIVE", "1")
    seed, xs, cots, _, _ = cases[case]
    _, (outs, states, grads) = _device_run(case, seed, xs, cots)
    assert all(torch.isfinite(t).all() for t in outs + states + grads)
    # the switch is live: a layer outside the kernels does raise under it
    from ebfi_amd.recurrent import TransposedConvLayer
    with pytest.raises(N.EbfiNativeError, match="EBFI_STRICT_NATIVE"):
        TransposedConvLayer(4, 4, kernel_size=3, padding=1).cuda()(torch.zeros(1, 4, 4, 4, device="cuda"))


def test_captured_two_call_step_replays_the_eager_bits(cases):
    seed, xs, cots, _, _ = cases["A"]
    names = [n for n, _ in R.names_and_shapes("A")]
    net = _net("A", seed)
    xd, cd = [x.float().cuda() for x in xs], [c.float().cuda() for c in cots]
    eager = _bits(_two_calls(net, xd, cd, names))
    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):
        _two_calls(net, xd, cd, names)                          # (the eager pass a capture runs first)
    torch.cuda.current_stream().wait_stream(side)
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        captured = _two_calls(net, xd, cd, names)
    for _ in range(2):
        for t in captured[0] + captured[1] + captured[2]:
            t.fill_(float("nan"))
        graph.replay()
        torch.cuda.synchronize()
        assert _bits(captured) == eager


def test_unetflow_under_the_event_warping_loss(cases):
    """The producer the flow losses were missing: UNetFlow (case A's configuration) -> ebfi_amd.iwe.EventWarping -> backward.
    No accuracy claim here (the warp has floor boundaries): finite gradients everywhere, non-zero ones where the flow reaches,
    and the same bits twice."""
    from ebfi_amd.iwe import EventWarping
    seed, xs, _, _, _ = cases["A"]
    B, _, H, W = R.CASES["A"]["shape"]
    rs = np.random.RandomState(5)
    n = 64
    ev = np.stack([rs.uniform(0, 1, (B, n)), rs.randint(0, H, (B, n)), rs.randint(0, W, (B, n)), rs.choice([-1.0, 1.0], (B, n))], -1)
    events = torch.from_numpy(ev.astype(np.float32)).cuda()
    pol_mask = torch.stack([events[..., 3] > 0, events[..., 3] < 0], -1).float().contiguous()
    loss_fn = EventWarping({"loss": {"flow_regul_weight": 0.001}}, "cuda")
    net = _net("A", seed)
    x = xs[0].float().cuda()

    def run():
        net.states = [None] * net.num_encoders
        net.zero_grad(set_to_none=True)
        loss = loss_fn([net(x)["flow"]], events, pol_mask, (H, W))
        loss.backward()
        return loss.detach().clone(), {k: p.grad.clone() for k, p in net.named_parameters() if p.grad is not None}

    loss, grads = run()
    assert torch.isfinite(loss) and set(grads) == {k for k, _ in net.named_parameters()}
    assert all(torch.isfinite(g).all() for g in grads.values())
    for key in ("pred.conv2d.weight", "decoders.0.conv2d.weight", "decoders.1.conv2d.weight",
                "encoders.0.recurrent_block.Gates.weight", "encoders.1.recurrent_block.Gates.weight"):
        assert float(grads[key].abs().max()) > 0, key
    loss2, grads2 = run()
    assert loss.cpu().numpy().tobytes() == loss2.cpu().numpy().tobytes()
    assert all(grads[k].cpu().numpy().tobytes() == grads2[k].cpu().numpy().tobytes() for k in grads)
