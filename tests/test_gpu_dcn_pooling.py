"""Deformable PS-ROI pooling on the device (ebfi_amd.dcn: dcn_v2_pooling_forward / _backward, _DCNv2Pooling, DCNv2Pooling,
DCNPooling) against tests/psroi_ref.py: its float32 run is the position law (count must match exactly), its float64 run
the oracle of the values.  Fixtures: tests/psroi_cases.py; tests/test_psroi_ref.py asserts that the two precisions agree on
every sample's inclusion and corners there, which is what makes the float64 comparison meaningful.

Bars: 2e-5 (forward) and 5e-5 (gradients) in the relative max norm, the bars of tests/test_gpu_dcn.py."""
import functools

import numpy as np
import pytest
import torch

import psroi_cases as K
import psroi_ref as R
from ebfi_amd import dcn

pytestmark = pytest.mark.gpu

F32, F64 = np.float32, np.float64
FWD_BAR, GRAD_BAR = 2e-5, 5e-5


def _rel(a, b):
    return ((a - b).abs().max() / b.abs().max().clamp_min(1e-30)).item()


def _relnp(dev, want):
    return _rel(dev.detach().cpu().double(), torch.from_numpy(np.array(want)).double())


def _cuda(a):
    return torch.from_numpy(np.array(a)).cuda()              # (a copy: the fixtures are read-only)


def _grad_out(c):
    return np.random.RandomState(99).randn(c.R, c.D, c.P, c.P).astype(F32)


@functools.lru_cache(maxsize=None)
def oracle(name, dtype):
    """(out, count, grad_input, grad_trans) of a fixture in `dtype`, computed once."""
    c = K.case(name)
    out, count = R.forward(c.inp, c.rois, c.trans, *K.law_args(c), no_trans=c.no_trans, dtype=dtype)
    gi, gt = R.backward(_grad_out(c), c.inp, c.rois, c.trans, *K.law_args(c), no_trans=c.no_trans, dtype=dtype)
    for a in (out, count, gi, gt):
        a.setflags(write=False)
    return out, count, gi, gt


def _op_args(c):
    """The tail of dcn_v2_pooling_forward / _backward after the tensors."""
    return (c.no_trans, c.scale, c.D, c.G, c.P, c.part, c.spp, c.trans_std)


def run_device(c, rois=None, trans=None, go=None):
    inp, rois = _cuda(c.inp), _cuda(c.rois if rois is None else rois)
    trans = inp.new() if c.no_trans else _cuda(c.trans if trans is None else trans)
    out, count = dcn.dcn_v2_pooling_forward(inp, rois, trans, *_op_args(c))
    go = _cuda(_grad_out(c) if go is None else go)
    gi, gt = dcn.dcn_v2_pooling_backward(go, inp, rois, trans, count, *_op_args(c))
    torch.cuda.synchronize()
    return out, count, gi, gt


@functools.lru_cache(maxsize=None)
def device(name):
    return run_device(K.case(name))


@pytest.mark.parametrize("name", K.NAMES)
def test_count_is_the_float32_law_exactly(name):
    c = K.case(name)
    out, count, _, _ = device(name)
    assert tuple(out.shape) == tuple(count.shape) == (c.R, c.D, c.P, c.P) and count.dtype == torch.float32
    want = oracle(name, F32)[1]
    assert np.array_equal(count.cpu().numpy(), want)
    full = c.spp * c.spp
    assert (want == 0).any() and (want == full).any() and ((want > 0) & (want < full)).any()
    assert (out.cpu().numpy()[want == 0] == 0).all()


@pytest.mark.parametrize("name", K.NAMES)
def test_forward_matches_the_float64_oracle(name):
    out = device(name)[0]
    err = _relnp(out, oracle(name, F64)[0])
    print("forward %s: %.3e" % (name, err))
    assert err < FWD_BAR


@pytest.mark.parametrize("name", K.NAMES)
def test_gradients_match_the_float64_oracle(name):
    c = K.case(name)
    _, _, gi, gt = device(name)
    _, _, want_gi, want_gt = oracle(name, F64)
    e_in = _relnp(gi, want_gi)
    assert np.abs(want_gi).max() > 0
    if c.no_trans:
        print("backward %s: grad_input %.3e" % (name, e_in))
        assert gt.numel() == 0
    else:
        e_tr = _relnp(gt, want_gt)
        print("backward %s: grad_input %.3e, grad_trans %.3e" % (name, e_in, e_tr))
        assert tuple(gt.shape) == c.trans.shape and np.abs(want_gt).max() > 0
        assert e_tr < GRAD_BAR
    assert e_in < GRAD_BAR


@pytest.mark.parametrize("name", ["A", "B", "C", "D"])
def test_grad_trans_is_bit_reproducible_and_zero_past_the_rois(name):
    c = K.case(name)
    first, second = run_device(c)[3], run_device(c)[3]
    assert torch.equal(first, second) and torch.equal(first, device(name)[3])
    assert first[:c.R].abs().max() > 0
    if name == "B":
        assert first.shape[0] == c.R + 3
    assert not first[c.R:].any()


@pytest.mark.parametrize("name", ["A", "B", "C", "D"])
def test_zero_trans_is_no_trans_bit_for_bit(name):
    c = K.case(name)
    out0, count0, gi0, gt0 = run_device(c, trans=np.zeros_like(c.trans))
    plain = c._replace(no_trans=True, nc=1, trans=None)
    out1, count1, gi1, _ = run_device(plain)
    assert torch.equal(out0, out1) and torch.equal(count0, count1) and out0.abs().max() > 0
    # (grad_input is summed with atomics: the order of the adds, hence the last bits, differ from launch to launch)
    assert _rel(gi0.double(), gi1.double()) < GRAD_BAR


def test_rois_outside_the_batch_pool_nothing_and_disturb_nothing():
    c = K.case("B")
    bad, good = [0, 2, 4, 5], [1, 3]
    rois = c.rois.copy()
    rois[bad, 0] = [c.B, -1, 0.5, np.nan]
    out, count, gi, gt = run_device(c, rois=rois)
    ref = device("B")
    assert not out[bad].any() and not count[bad].any() and not gt[bad].any() and not gt[c.R:].any()
    for got, want in zip((out, count, gt), (ref[0], ref[1], ref[3])):
        assert torch.equal(got[good], want[good]) and want[good].abs().max() > 0
    # the gradient of the input comes from the two good ROIs alone
    go = _grad_out(c)
    want_gi, _ = R.backward(go, c.inp, rois, c.trans, *K.law_args(c), dtype=F64)
    only, _ = R.backward(go[good], c.inp, c.rois[good], c.trans[good], *K.law_args(c), dtype=F64)
    assert np.allclose(want_gi, only, rtol=1e-12, atol=0) and np.abs(only).max() > 0      # (summed in another order)
    assert _relnp(gi, want_gi) < GRAD_BAR
    # all four at once: every ROI refused
    rois[:, 0] = np.nan
    out, count, gi, gt = run_device(c, rois=rois)
    assert not out.any() and not count.any() and not gi.any() and not gt.any()


def test_nan_and_infinite_offsets():
    """A NaN offset makes its samples' coordinate NaN, which no comparison skips and fmax / fmin turn into pixel 0: counted.
    An infinite one is skipped.  Output and count are the float32 restatement's, bit for bit."""
    c = K.case("B")
    trans = c.trans.copy()
    trans[2, 0, 3, 3] = np.nan              # ROI 2 (half-integer corners), class 0, x
    trans[2, 3, 1, 5] = np.nan              # class 1, y
    trans[3, 1, 2, 2] = np.inf              # ROI 3 (partly outside), class 0, y
    trans[4, 2, 1, 1] = -np.inf             # class 1, x
    out, count, gi, gt = run_device(c, trans=trans)
    want_out, want_count = R.forward(c.inp, c.rois, trans, *K.law_args(c), dtype=F32)
    assert want_count[2, 0, 3, 3] == 16 and want_count[2, 4, 1, 5] == 16          # NaN: all 16 samples, on column / row 0
    assert want_count[3, 0, 2, 2] == 0 and want_count[4, 4, 1, 1] == 0            # Inf: none
    assert np.array_equal(count.cpu().numpy(), want_count)
    assert torch.isfinite(out).all()
    assert np.array_equal(out.cpu().numpy(), want_out)
    assert torch.isfinite(gi).all()


class _OraclePool(torch.autograd.Function):
    """The float64 restatement as an autograd node on CPU tensors."""

    @staticmethod
    def forward(ctx, inp, rois, trans, no_trans, args):
        t = None if no_trans else trans.detach().numpy()
        out, _ = R.forward(inp.detach().numpy(), rois.numpy(), t, *args, no_trans=no_trans, dtype=F64)
        ctx.save_for_backward(inp, rois, trans)
        ctx.no_trans, ctx.args = no_trans, args
        return torch.from_numpy(out)

    @staticmethod
    def backward(ctx, go):
        inp, rois, trans = ctx.saved_tensors
        t = None if ctx.no_trans else trans.detach().numpy()
        gi, gt = R.backward(go.numpy(), inp.detach().numpy(), rois.numpy(), t, *ctx.args, no_trans=ctx.no_trans, dtype=F64)
        return torch.from_numpy(gi), None, (None if ctx.no_trans else torch.from_numpy(gt)), None, None


def test_dcnv2pooling_through_autograd():
    c = K.case("D")
    inp, trans = _cuda(c.inp).requires_grad_(True), _cuda(c.trans).requires_grad_(True)
    mod = dcn.DCNv2Pooling(c.scale, c.P, c.D, False, c.G, c.part, c.spp, c.trans_std).cuda()
    out = mod(inp, _cuda(c.rois), trans)
    go = _cuda(_grad_out(c))
    out.backward(go)
    want = oracle("D", F64)
    assert _relnp(out, want[0]) < FWD_BAR
    assert _relnp(inp.grad, want[2]) < GRAD_BAR and _relnp(trans.grad, want[3]) < GRAD_BAR
    # no_trans through the module, on fixture E (without offsets D's samples sit on boundaries that float32 and float64 place
    # differently: no oracle there): the offset argument is ignored and gets no gradient
    e = K.case("E")
    plain = dcn.DCNv2Pooling(e.scale, e.P, e.D, True, e.G, e.part, e.spp, e.trans_std).cuda()
    x, ignored = _cuda(e.inp).requires_grad_(True), _cuda(K.case("B").trans).requires_grad_(True)
    o = plain(x, _cuda(e.rois), ignored)
    o.backward(_cuda(_grad_out(e)))
    want = oracle("E", F64)
    assert _relnp(o, want[0]) < FWD_BAR and _relnp(x.grad, want[2]) < GRAD_BAR and ignored.grad is None


def test_dcnpooling_through_autograd():
    """B's map and ROIs, one class (the module's offsets have two channels).  The last layer is given weights, so the
    offsets move; the same module is assembled from the float64 restatement and copies of the weights on the CPU."""
    c = K.case("B")
    torch.manual_seed(5)
    mod = dcn.DCNPooling(c.scale, c.P, c.D, False, c.G, c.part, c.spp, c.trans_std, deform_fc_dim=48)
    with torch.no_grad():
        mod.offset_mask_fc[4].weight.normal_(0, 0.3)
        mod.offset_mask_fc[4].bias.normal_(0, 0.5)
    fc64 = torch.nn.Sequential(torch.nn.Linear(c.P * c.P * c.D, 48), torch.nn.ReLU(), torch.nn.Linear(48, 48), torch.nn.ReLU(),
                               torch.nn.Linear(48, c.P * c.P * 3)).double()
    fc64.load_state_dict({k: v.double() for k, v in mod.offset_mask_fc.state_dict().items()})
    mod = mod.cuda()
    go = _grad_out(c)

    inp = _cuda(c.inp).requires_grad_(True)
    out = mod(inp, _cuda(c.rois))
    out.backward(_cuda(go))

    args = K.law_args(c)
    x64, rois = torch.from_numpy(c.inp.astype(F64)).requires_grad_(True), torch.from_numpy(c.rois.copy())
    roi = _OraclePool.apply(x64, rois, x64.new(), True, args)
    o1, o2, mask = torch.chunk(fc64(roi.view(c.R, -1)).view(c.R, 3, c.P, c.P), 3, dim=1)
    offset = torch.cat((o1, o2), dim=1)
    want = _OraclePool.apply(x64, rois, offset, False, args) * torch.sigmoid(mask)
    want.backward(torch.from_numpy(go.astype(F64)))

    assert offset.abs().max() > 0.1
    e_out, e_in = _rel(out.detach().cpu().double(), want.detach()), _rel(inp.grad.cpu().double(), x64.grad)
    print("DCNPooling: forward %.3e, grad_input %.3e" % (e_out, e_in))
    assert e_out < FWD_BAR and e_in < GRAD_BAR
    for (k, p), q in zip(mod.offset_mask_fc.named_parameters(), fc64.parameters()):
        assert q.grad.abs().max() > 0, k
        e = _rel(p.grad.cpu().double(), q.grad)
        print("DCNPooling: grad %s %.3e" % (k, e))
        assert e < GRAD_BAR, k
    # as constructed (zeroed last layer) the offsets are 0 and the mask 1/2
    fresh = dcn.DCNPooling(c.scale, c.P, c.D, False, c.G, c.part, c.spp, c.trans_std, deform_fc_dim=48).cuda()
    with torch.no_grad():
        half = fresh(_cuda(c.inp), _cuda(c.rois))
        plain = dcn.DCNPooling(c.scale, c.P, c.D, True, c.G, c.part, c.spp, c.trans_std).cuda()(_cuda(c.inp), _cuda(c.rois))
    assert torch.equal(half, plain * 0.5)


def test_side_stream_and_graph_capture():
    c = K.case("B")
    inp, rois, trans, go = _cuda(c.inp), _cuda(c.rois), _cuda(c.trans), _cuda(_grad_out(c))
    ref = device("B")

    def step():
        out, count = dcn.dcn_v2_pooling_forward(inp, rois, trans, *_op_args(c))
        gi, gt = dcn.dcn_v2_pooling_backward(go, inp, rois, trans, count, *_op_args(c))
        return out, count, gi, gt

    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):
        eager = step()
    torch.cuda.current_stream().wait_stream(side)
    torch.cuda.synchronize()
    for got, want in zip(eager, ref):
        assert got.abs().max() > 0
    assert all(torch.equal(eager[i], ref[i]) for i in (0, 1, 3)) and _rel(eager[2].double(), ref[2].double()) < GRAD_BAR

    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        captured = step()
    for t in captured:
        t.fill_(7.0)
    graph.replay()
    torch.cuda.synchronize()
    assert all(torch.equal(captured[i], ref[i]) for i in (0, 1, 3))
    assert _rel(captured[2].double(), ref[2].double()) < GRAD_BAR
