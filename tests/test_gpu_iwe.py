"""GPU checks of the device warping losses (ebfi_amd.iwe, csrc/iwe.hip).  Images and indices are compared with torch.equal
against what the reference itself returned (tests/golden/iwe_small.npz) or against the serial numpy restatement that
tests/test_iwe_host.py holds against that fixture (tests/iwe_ref.py): the law is a serial fp32 sum per pixel in list order, so
there is no tolerance to choose.  The loss and its gradient are held against the reference's float64 run; the bar per quantity
is 8 times the deviation of the reference's own float32 run from it (stored in the fixture), floor 4 float32 ulps."""
import os

import numpy as np
import pytest
import torch

from ebfi_amd import iwe as _iwe  # noqa: F401  (every test here is about this module: without it none may pass)

import iwe_ref as R

pytestmark = pytest.mark.gpu
F = np.float32
CASES = ("general", "pile", "bounds", "ties", "empty", "padding", "average")
TOLERANCE_CASES = ("general", "pile", "bounds", "padding")


@pytest.fixture(scope="module")
def golden(golden_dir):
    return np.load(os.path.join(golden_dir, "iwe_small.npz"))


@pytest.fixture(scope="module")
def I():
    from ebfi_amd import iwe
    return iwe


def dev(a):
    return torch.from_numpy(np.ascontiguousarray(a)).cuda()


def case(golden, name):
    v = {k: golden["%s__%s" % (name, k)] for k in ("events", "pol_mask", "flows")}
    v.update(res=(int(golden[name + "__H"]), int(golden[name + "__W"])), weight=float(golden[name + "__weight"]))
    v["flow_ev"] = R.event_flow(v["flows"][0], v["events"], v["res"])      # the first flow at every event's source pixel
    return v


def config(v, batch=None):
    return {"loss": {"flow_regul_weight": v["weight"]},
            "loader": {"resolution": list(v["res"]), "batch_size": v["events"].shape[0] if batch is None else batch}}


def bars(golden):
    floor = 4 * 2.0 ** -23
    return max(8 * float(golden["dev_loss"]), floor), max(8 * float(golden["dev_grad"]), floor)


def twice(call, keep, t):
    """The call made twice: the same bits, float32 on the device, and every input bit-unchanged afterwards."""
    a, b = call(), call()
    for x, y in zip(a if isinstance(a, tuple) else (a,), b if isinstance(b, tuple) else (b,)):
        assert x.is_cuda and x.dtype == torch.float32 and x.cpu().numpy().tobytes() == y.cpu().numpy().tobytes()
    for k, orig in keep.items():
        assert torch.equal(t[k], orig) and t[k].cpu().numpy().tobytes() == orig.cpu().numpy().tobytes(), k
    return a


@pytest.mark.parametrize("name", CASES)
def test_images_and_indices_are_the_reference_bits(golden, I, name):
    v = case(golden, name)
    res, scaling = v["res"], max(v["res"])
    t = dict(ev=dev(v["events"]), pm=dev(v["pol_mask"]), flow=dev(v["flows"][0]), fe=dev(v["flow_ev"]))
    t["pos"], t["neg"] = t["pm"][:, :, 0:1], t["pm"][:, :, 1:2]
    keep = {k: a.clone() for k, a in t.items()}
    g = lambda k: dev(golden["%s__%s" % (name, k)])
    for branch, rnd in (("bil", False), ("rnd", True)):
        for tref in (1, 0):
            idx, w = twice(lambda: I.get_interpolation(t["ev"], t["fe"], tref, res, scaling, round_idx=rnd), keep, t)
            assert torch.equal(idx, g("gi_%s_t%d_idx" % (branch, tref))), (branch, tref)      # (-0.0 == 0.0)
            assert torch.equal(w, g("gi_%s_t%d_w" % (branch, tref))), (branch, tref)
    idx, w = I.get_interpolation(t["ev"], t["fe"], 1, res, scaling)
    pm4 = torch.cat([t["pos"]] * 4, dim=1)
    assert torch.equal(twice(lambda: I.interpolate(idx.long(), w, res, polarity_mask=pm4), keep, t), g("interp"))
    assert torch.equal(twice(lambda: I.interpolate(idx.long(), w, res), keep, t), g("interp_plain"))
    assert torch.equal(I.interpolate(idx, w, res), g("interp_plain"))                        # a float32 index is truncated
    assert torch.equal(twice(lambda: I.deblur_events(t["flow"], t["ev"], res, flow_scaling=scaling), keep, t), g("deblur"))
    for key, rnd in (("pol_rnd", True), ("pol_bil", False)):
        got = twice(lambda: I.compute_pol_iwe(t["flow"], t["ev"], res, t["pos"], t["neg"], flow_scaling=scaling, round_idx=rnd),
                    keep, t)
        assert torch.equal(got, g(key)), key
        if not rnd:
            one = I.deblur_events(t["flow"], t["ev"], res, flow_scaling=scaling, round_idx=False, polarity_mask=t["neg"])
            assert torch.equal(one, got[:, 1:2])
    avg = twice(lambda: I.AveragedIWE(config(v), "cuda")(t["flow"], t["ev"], t["pm"]), keep, t)
    assert tuple(avg.shape) == golden[name + "__avg"].shape and torch.equal(avg, g("avg"))


def warping(I, v, flows, upstream=None):
    """(loss, [gradients]) of EventWarping on device tensors; the flows are used as given."""
    loss = I.EventWarping(config(v), "cuda")(flows, v["t_ev"], v["t_pm"], v["res"])
    out = loss if upstream is None else loss * upstream
    leaves = [f if f.is_leaf else f.root for f in flows]
    grads = torch.autograd.grad(out, leaves)
    return loss.detach(), [g_.detach() for g_ in grads]


def uploaded(golden, name):
    v = case(golden, name)
    v["t_ev"], v["t_pm"] = dev(v["events"]), dev(v["pol_mask"])
    return v


def check_against_float64(golden, name, loss, grads, scale=1.0):
    bar_loss, bar_grad = bars(golden)
    want = float(golden[name + "__loss64"])
    err = abs(float(loss) - want) / abs(want)
    print("%s: loss %.9g, float64 %.17g, relative error %.3g (bar %.3g)" % (name, float(loss), want, err, bar_loss))
    assert err <= bar_loss
    for k, (g_, g64) in enumerate(zip(grads, golden[name + "__grad64"])):
        g64 = g64 * scale
        err = np.abs(g_.cpu().numpy().astype(np.float64) - g64).max() / max(np.abs(g64).max(), 1e-300)
        print("%s: flow %d gradient error %.3g of the largest element (bar %.3g)" % (name, k, err, bar_grad))
        assert err <= bar_grad


@pytest.mark.parametrize("name", CASES)
def test_event_warping_against_the_float64_reference(golden, I, name):
    """Every case, `general` with its flow_list of two.  The ties case (flow 0, stamps 0 and 1: every warp lands on an integer)
    is exact by construction, so the float32 reference is the same function there: it must meet the same bar against it."""
    v = uploaded(golden, name)
    flows = [dev(f).requires_grad_(True) for f in v["flows"]]
    keep = {"ev": v["t_ev"].clone(), "pm": v["t_pm"].clone()}
    keep.update({"flow%d" % k: f.detach().clone() for k, f in enumerate(flows)})
    loss, grads = warping(I, v, flows)
    assert loss.dtype == torch.float32 and loss.dim() == 0 and loss.is_cuda
    again, grads2 = warping(I, v, flows)
    assert loss.cpu().numpy().tobytes() == again.cpu().numpy().tobytes()
    for a, b in zip(grads, grads2):
        assert a.cpu().numpy().tobytes() == b.cpu().numpy().tobytes()
    t = dict(ev=v["t_ev"], pm=v["t_pm"], **{"flow%d" % k: f.detach() for k, f in enumerate(flows)})
    for k, orig in keep.items():
        assert t[k].cpu().numpy().tobytes() == orig.cpu().numpy().tobytes(), k
    check_against_float64(golden, name, loss, grads)
    if name == "ties":
        bar_loss, bar_grad = bars(golden)
        l32, g32 = float(golden["ties__loss32"]), golden["ties__grad32"][0].astype(np.float64)
        assert abs(float(loss) - l32) <= bar_loss * abs(l32)
        assert np.abs(grads[0].cpu().numpy() - g32).max() <= bar_grad * np.abs(g32).max()
    if name == "empty":                                       # N = 0: only the smoothness term
        f = v["flows"][0].astype(np.float64)
        smooth = np.sqrt((f[:, :, :-1] - f[:, :, 1:]) ** 2 + 1e-6).sum() + np.sqrt((f[:, :, :, :-1] - f[:, :, :, 1:]) ** 2 + 1e-6).sum()
        assert abs(float(loss) - v["weight"] * smooth) <= 4 * 2.0 ** -23 * v["weight"] * smooth


def test_flow_variants(golden, I):
    """The general case's two flows: handed over non-contiguous and as non-leaf tensors they give the bits of the plain call;
    an upstream gradient other than 1 scales the gradient."""
    v = uploaded(golden, "general")
    plain = [dev(f).requires_grad_(True) for f in v["flows"]]
    loss, grads = warping(I, v, plain)
    B, _, H, W = v["flows"][0].shape
    strided = []
    for f in v["flows"]:
        wide = torch.zeros((B, H, W + 3, 2), device="cuda")
        wide[:, :, 1:W + 1, :] = dev(f).permute(0, 2, 3, 1)
        leaf = wide.requires_grad_(True)
        view = leaf[:, :, 1:W + 1, :].permute(0, 3, 1, 2)                 # [B, 2, H, W], no stride in order
        assert not view.is_contiguous() and not view.is_leaf
        view.root = leaf
        strided.append(view)
    loss_s, grads_s = warping(I, v, strided)
    assert loss_s.cpu().numpy().tobytes() == loss.cpu().numpy().tobytes()
    for g_, gs in zip(grads, grads_s):
        inner = gs[:, :, 1:W + 1, :].permute(0, 3, 1, 2)
        assert inner.contiguous().cpu().numpy().tobytes() == g_.cpu().numpy().tobytes()
        assert not gs[:, :, 0, :].any() and not gs[:, :, W + 1:, :].any()
    loss_u, grads_u = warping(I, v, plain, upstream=2.5)
    assert loss_u.cpu().numpy().tobytes() == loss.cpu().numpy().tobytes()
    check_against_float64(golden, "general", loss_u, grads_u, scale=2.5)
    one = warping(I, v, plain[:1])[1][0]                                   # a flow's gradient does not depend on its list
    assert one.cpu().numpy().tobytes() == grads[0].cpu().numpy().tobytes()


@pytest.mark.parametrize("name", ["general", "pile"])
def test_forward_and_backward_replay_from_a_graph(golden, I, name):
    v = uploaded(golden, name)
    flows = [dev(f).requires_grad_(True) for f in v["flows"]]
    eager_loss, eager_grads = warping(I, v, flows)
    torch.cuda.synchronize()
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        main = torch.cuda.current_stream()
        loss, grads = warping(I, v, flows)
        assert torch.cuda.current_stream() == main and torch.cuda.is_current_stream_capturing()
    for _ in range(2):
        loss.zero_()
        for g_ in grads:
            g_.zero_()
        graph.replay()
        torch.cuda.synchronize()
        assert loss.cpu().numpy().tobytes() == eager_loss.cpu().numpy().tobytes()
        for a, b in zip(grads, eager_grads):
            assert a.cpu().numpy().tobytes() == b.cpu().numpy().tobytes()


def test_masked_rows_are_not_counted_and_draw_no_gradient(golden, I):
    """The padding case's rows with pol_mask == 0 hold zeros; with arbitrary events in their place every image, the loss and
    the gradient keep their bits."""
    v = uploaded(golden, "padding")
    H, W = v["res"]
    dead = v["pol_mask"].sum(axis=2) == 0
    rng = np.random.default_rng(6)
    noisy = np.array(v["events"])
    noisy[dead] = np.stack([rng.uniform(0, 1, dead.sum()), rng.integers(0, H, dead.sum()), rng.integers(0, W, dead.sum()),
                            rng.choice([-1.0, 1.0], dead.sum())], axis=1).astype(F)
    flow = dev(v["flows"][0]).requires_grad_(True)
    loss, grads = warping(I, v, [flow])
    w = dict(v, t_ev=dev(noisy))
    loss_n, grads_n = warping(I, w, [flow])
    assert loss_n.cpu().numpy().tobytes() == loss.cpu().numpy().tobytes()
    assert grads_n[0].cpu().numpy().tobytes() == grads[0].cpu().numpy().tobytes()
    pos, neg = v["t_pm"][:, :, 0:1], v["t_pm"][:, :, 1:2]
    for rnd in (True, False):
        a = I.compute_pol_iwe(flow.detach(), v["t_ev"], v["res"], pos, neg, flow_scaling=max(H, W), round_idx=rnd)
        b = I.compute_pol_iwe(flow.detach(), w["t_ev"], v["res"], pos, neg, flow_scaling=max(H, W), round_idx=rnd)
        assert torch.equal(a, b)


def test_undefined_inputs_have_the_documented_results(golden, I):
    v = uploaded(golden, "bounds")
    H, W = v["res"]
    ev = np.array(v["events"])
    odd = np.array([[0.3, -1, 2, 1], [0.4, H, 2, 1], [0.5, 2, -1, -1], [0.6, 2, W, 1], [0.2, 2.5, 3, 1], [0.7, 1, 3.25, -1],
                    [0.8, np.nan, 1, 1], [0.1, 1, np.inf, 1]], F)
    where = [3, 40, 41, 100, 150, 200, 255, 256]
    masked_pm = np.array(v["pol_mask"])
    for b in range(ev.shape[0]):
        ev[b, where] = odd
        masked_pm[b, where] = 0
    clean = np.array(ev)
    clean[:, where] = 0
    flow = dev(v["flows"][0]).requires_grad_(True)
    bad = dict(v, t_ev=dev(ev))                                            # the odd events, unmasked ...
    good = dict(v, t_ev=dev(clean), t_pm=dev(masked_pm))                   # ... count as events that are not there
    loss_b, grads_b = warping(I, bad, [flow])
    loss_g, grads_g = warping(I, good, [flow])
    assert torch.isfinite(loss_b) and loss_b.cpu().numpy().tobytes() == loss_g.cpu().numpy().tobytes()
    assert grads_b[0].cpu().numpy().tobytes() == grads_g[0].cpu().numpy().tobytes()
    scaling = max(H, W)
    a = I.compute_pol_iwe(flow.detach(), bad["t_ev"], v["res"], bad["t_pm"][:, :, 0:1], bad["t_pm"][:, :, 1:2], flow_scaling=scaling)
    b = I.compute_pol_iwe(flow.detach(), good["t_ev"], v["res"], good["t_pm"][:, :, 0:1], good["t_pm"][:, :, 1:2], flow_scaling=scaling)
    assert torch.equal(a, b)
    avg = I.AveragedIWE(config(v), "cuda")(flow.detach(), bad["t_ev"], bad["t_pm"])
    assert torch.isfinite(avg).all()
    # a non-finite flow: weight 0 and index 0 for the event; the smoothness term still carries the NaN into the loss
    fe = np.array(v["flow_ev"])
    fe[0, 5], fe[1, 6], fe[2, 7] = (np.nan, 0.0), (0.0, np.inf), (-np.inf, np.nan)
    for rnd in (False, True):
        idx, wgt = I.get_interpolation(v["t_ev"], dev(fe), 1, v["res"], scaling, round_idx=rnd)
        n = ev.shape[1]
        for b, k in ((0, 5), (1, 6), (2, 7)):
            assert not idx[b, k::n].any() and not wgt[b, k::n].any()
        assert torch.isfinite(idx).all() and torch.isfinite(wgt).all()
    holed = np.array(v["flows"][0])
    holed[0, 1, 2, 3] = np.nan
    loss_n, grads_n = warping(I, v, [dev(holed).requires_grad_(True)])
    assert torch.isnan(loss_n)
    # interpolate: an index outside [0, H * W) is dropped
    idx = torch.tensor([[[0], [-1], [H * W], [5], [2 ** 40], [5], [-2 ** 40]]], device="cuda")
    wgt = torch.tensor([[[1.5], [7.0], [7.0], [0.25], [7.0], [0.125], [7.0]]], device="cuda")
    out = I.interpolate(idx, wgt, v["res"]).flatten()
    assert out[0] == 1.5 and out[5] == 0.375 and out.sum() == 1.875
    out = I.interpolate(idx.float(), wgt, v["res"]).flatten()
    assert out[0] == 1.5 and out[5] == 0.375 and out.sum() == 1.875


@pytest.mark.parametrize("n_hot", [63, 64, 65, 130])
def test_run_lengths_around_the_wave_walk(I, n_hot):
    """A run of 64 entries or more is walked by the whole wave, a shorter one by its own lane: one pixel that receives n_hot
    events, a second long run of 70 in the same wave and 40 scattered events, interleaved in the list, against the serial
    restatement -- for the plain scatter, the per-polarity images and AveragedIWE's count of distinct sources."""
    rng = np.random.default_rng(n_hot)
    B, H, W = 2, 8, 8
    n = n_hot + 70 + 40
    ev = np.zeros((B, n, 4), F)
    ev[:, :, 0] = rng.uniform(0.05, 0.95, (B, n))
    ev[:, :, 1], ev[:, :, 2] = rng.integers(0, H, (B, n)), rng.integers(0, W, (B, n))
    ev[:, :, 3] = rng.choice([-1.0, 1.0], (B, n))
    where = rng.permutation(n)
    ev[:, where[:n_hot], 1], ev[:, where[:n_hot], 2] = 3, 5
    ev[:, where[n_hot:n_hot + 70], 1], ev[:, where[n_hot:n_hot + 70], 2] = 6, 1
    flow = rng.uniform(-0.02, 0.02, (B, 2, H, W)).astype(F)                 # under a quarter pixel: runs stay together
    pm = np.stack([ev[:, :, 3] > 0, ev[:, :, 3] < 0], axis=2).astype(F) * rng.uniform(0.5, 1.5, (B, n, 1)).astype(F)
    res = (H, W)
    t_ev, t_flow, t_pm = dev(ev), dev(flow), dev(pm)
    fe = R.event_flow(flow, ev, res)
    idx, w = R.get_interpolation(ev, fe, 1, res, max(res))
    assert (R.interpolate(idx, w, res) != R.interpolate(idx, w, res, reverse=True)).any()      # the order matters here
    gi, gw = I.get_interpolation(t_ev, dev(fe), 1, res, max(res))
    assert torch.equal(gi, dev(idx)) and torch.equal(gw, dev(w))
    assert torch.equal(I.interpolate(gi.long(), gw, res), dev(R.interpolate(idx, w, res)))
    for rnd in (True, False):
        want = R.compute_pol_iwe(flow, ev, res, pm[:, :, 0:1], pm[:, :, 1:2], max(res), rnd)
        got = I.compute_pol_iwe(t_flow, t_ev, res, t_pm[:, :, 0:1], t_pm[:, :, 1:2], flow_scaling=max(res), round_idx=rnd)
        assert torch.equal(got, dev(want)), rnd
    # AveragedIWE: several sources into one destination, more than 64 events in the run
    ev2 = np.array(ev)
    ev2[:, where[:n_hot], 1] = rng.integers(2, 5, (B, n_hot))              # rows 2..4, all sent to row 3 by the flow below
    flow2 = np.zeros((B, 2, H, W), F)
    flow2[:, 1, 2, :], flow2[:, 1, 4, :] = F(0.125), F(-0.125)             # 8 * 0.125 * (1 - ts): up to one pixel
    ev2[:, :, 0] = rng.choice([0.0, 0.25], (B, n))
    want = R.averaged_iwe(flow2, ev2, pm, res)
    cfg = {"loader": {"resolution": [H, W], "batch_size": B}}
    got = I.AveragedIWE(cfg, "cuda")(dev(flow2), dev(ev2), t_pm)
    assert torch.equal(got, dev(want))
    unit = dev((pm != 0).astype(F))                     # whole counts: exact in any order, so eager torch must agree too
    assert torch.equal(I.AveragedIWE(cfg, "cuda")(dev(flow2), dev(ev2), unit), R.t_averaged_iwe(dev(flow2), dev(ev2), unit, res))


def test_averaged_iwe_refuses_a_batch_size_that_is_not_the_flows(golden, I):
    v = uploaded(golden, "average")
    with pytest.raises(ValueError):
        I.AveragedIWE(config(v, batch=2), "cuda")(dev(v["flows"][0]), v["t_ev"], v["t_pm"])
    empty = uploaded(golden, "empty")
    out = I.AveragedIWE(config(empty), "cuda")(dev(empty["flows"][0]), empty["t_ev"], empty["t_pm"])
    assert tuple(out.shape) == (2, 2) + empty["res"] and not out.any()


def test_the_reference_trainers_import_line_works():
    ns = {}
    exec("from loss import LaplacianLoss, Ternary, EventWarping, AveragedIWE", ns)
    exec("from myutils.iwe import deblur_events, compute_pol_iwe", ns)
    assert callable(ns["EventWarping"]) and callable(ns["compute_pol_iwe"])
