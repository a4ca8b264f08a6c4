"""GPU checks of the device reconstruction losses (ebfi_amd.bcloss, csrc/bcloss.hip): BrightnessConstancy's three terms and
Sobel against the reference's float64 run (tests/golden/bc_small.npz) or, where a fixture would be too large, against the
float64 restatement that tests/test_bc_host.py holds against that fixture (tests/bc_ref.py).  The bar per quantity is 8 times
the deviation of the reference's own float32 run from its float64 run (stored in the fixture), floor 4 float32 ulps: relative
for a loss, largest error over largest element for a gradient.  Every call is made twice and must give the same bytes."""
import os

import numpy as np
import pytest
import torch

from ebfi_amd import bcloss as _bcloss  # noqa: F401  (every test here is about this module: without it none may pass)

import bc_ref as R

pytestmark = pytest.mark.gpu
F = np.float32
CASES = ("general", "bounds", "pile", "nomask", "empty", "still")
TERMS = {"gen": ("flow", "img"), "tc": ("flow", "prev_img", "img"), "tv": ("img",)}
GRAD_KEY = {"flow": "gflow", "img": "gimg", "prev_img": "gprev"}


@pytest.fixture(scope="module")
def golden(golden_dir):
    return np.load(os.path.join(golden_dir, "bc_small.npz"))


@pytest.fixture(scope="module")
def BC():
    from ebfi_amd import bcloss
    return bcloss


def dev(a):
    return torch.from_numpy(np.ascontiguousarray(a)).cuda()


def raw(t):
    return t.detach().cpu().numpy().tobytes()


def case(golden, name):
    v = {k: golden["%s__%s" % (name, k)] for k in ("flow", "img", "prev_img", "cnt", "events", "pol_mask", "avg", "weights")}
    v["res"] = (int(golden[name + "__H"]), int(golden[name + "__W"]))
    return v


def module(BC, v):
    config = {"loss": {"reconstruction_regul_weight": [float(w) for w in v["weights"]]},
              "loader": {"resolution": list(v["res"]), "batch_size": v["flow"].shape[0]}}
    return BC.BrightnessConstancy(config, "cuda")


def upload(v):
    return {k: dev(v[k]) for k in ("flow", "img", "prev_img", "cnt", "events", "pol_mask")}


def term(bc, which, t, upstream=None):
    """(loss, {input name: gradient}) of one term; t[name] are used as given, gradients are taken at t[name + '_leaf'] if there."""
    inputs = {"inp_cnt": t["cnt"], "inp_list": t["events"], "inp_pol_mask": t["pol_mask"]}
    if which == "gen":
        loss = bc.generative_model(t["flow"], t["img"], inputs)
    elif which == "tc":
        loss = bc.temporal_consistency(t["flow"], t["prev_img"], t["img"])
    else:
        loss = bc.regularization(t["img"])
    leaves = [t.get(k + "_leaf", t[k]) for k in TERMS[which]]
    grads = torch.autograd.grad(loss if upstream is None else loss * upstream, leaves)
    return loss.detach(), {k: g.detach() for k, g in zip(TERMS[which], grads)}


def leaves(t):
    return dict(t, **{k: t[k].clone().requires_grad_(True) for k in ("flow", "img", "prev_img")})


def bars(golden):
    floor = 4 * 2.0 ** -23
    return max(8 * float(golden["dev_loss"]), floor), max(8 * float(golden["dev_grad"]), floor)


def check(golden, what, loss, grads, want_loss, want_grads, scale=1.0):
    bar_loss, bar_grad = bars(golden)
    err = abs(float(loss) - want_loss) / abs(want_loss)
    print("%s: loss %.9g, float64 %.17g, relative error %.3g (bar %.3g)" % (what, float(loss), want_loss, err, bar_loss))
    assert loss.dtype == torch.float32 and loss.dim() == 0 and loss.is_cuda and err <= bar_loss
    for k, g in grads.items():
        g64 = np.asarray(want_grads[k], np.float64) * scale
        assert g.dtype == torch.float32 and tuple(g.shape) == g64.shape
        err = np.abs(g.cpu().numpy().astype(np.float64) - g64).max() / max(np.abs(g64).max(), 1e-300)
        print("%s: gradient into %s: error %.3g of the largest element (bar %.3g)" % (what, k, err, bar_grad))
        assert err <= bar_grad, k


@pytest.mark.parametrize("which", sorted(TERMS))
@pytest.mark.parametrize("name", CASES)
def test_terms_against_the_float64_reference(golden, BC, name, which):
    v = case(golden, name)
    bc = module(BC, v)
    t = leaves(upload(v))
    keep = {k: a.detach().clone() for k, a in t.items()}
    loss, grads = term(bc, which, t)
    again, grads2 = term(bc, which, t)
    assert raw(loss) == raw(again)
    for k in grads:
        assert raw(grads[k]) == raw(grads2[k]), k
    for k, orig in keep.items():
        assert raw(t[k]) == raw(orig), k
    want = {k: golden["%s__%s_%s64" % (name, which, GRAD_KEY[k])] for k in TERMS[which]}
    check(golden, "%s %s" % (name, which), loss, grads, float(golden["%s__%s_loss64" % (name, which)]), want)
    if which == "gen":                                        # the averaged image the term stands on: the reference's bits
        masked = dev(R.masked_flow(v["flow"], v["cnt"]))
        assert torch.equal(bc.averaged_iwe(masked, t["events"], t["pol_mask"]), dev(v["avg"]))


def test_masked_pixels_draw_no_generative_flow_gradient(golden, BC):
    v = case(golden, "nomask")
    bc = module(BC, v)
    t = leaves(upload(v))
    _, grads = term(bc, "gen", t)
    masked = dev(v["cnt"].sum(axis=1) == 0)[:, None].expand(-1, 2, -1, -1)
    assert masked.float().mean() == 0.5
    at = grads["flow"][masked]
    assert (at == 0).all() and not at.view(torch.int32).any()             # +0.0, bit for bit
    assert (grads["flow"][~masked] != 0).any()
    _, grads = term(bc, "tc", t)
    assert (grads["flow"][masked] != 0).any()                             # temporal consistency takes the flow as given


def serial_scatter(v, reverse=False):
    """grad_prev_img of temporal consistency as the law states it, emulated on the host: the addend of (source pixel, corner)
    is float32(g * w), g and the bilinear weight w in float64; every destination adds its addends serially in float32, in
    ascending source-pixel index, then corner order top-left, top-right, bottom-left, bottom-right."""
    H, W = v["res"]
    ix, iy = R.coordinates(v["flow"], v["res"])
    resid = v["img"][:, 0].astype(np.float64) - R.sample(v["prev_img"][:, 0], ix, iy)[0]
    g = -(float(v["weights"][1]) * np.sign(resid))
    x0, y0 = np.floor(ix), np.floor(iy)
    tx, ty = ix - x0, iy - y0
    B = g.shape[0]
    entries = []
    for b in range(B):
        for h in range(H):
            for w in range(W):
                for c in range(4):
                    y, x = int(y0[b, h, w]) + (c >> 1), int(x0[b, h, w]) + (c & 1)
                    if 0 <= y < H and 0 <= x < W:
                        wt = (tx[b, h, w] if c & 1 else 1.0 - tx[b, h, w]) * (ty[b, h, w] if c >> 1 else 1.0 - ty[b, h, w])
                        entries.append((b, y, x, F(g[b, h, w] * wt)))
    out = np.zeros((B, 1, H, W), F)
    for b, y, x, a in (reversed(entries) if reverse else entries):
        out[b, 0, y, x] = out[b, 0, y, x] + a
    return out


@pytest.mark.parametrize("name", ["pile", "general", "bounds"])
def test_the_scatter_adds_in_the_promised_order(golden, BC, name):
    """Bit for bit: another fixed order of addition (the reversed one is tried here) gives other bits on these cases."""
    v = case(golden, name)
    bc = module(BC, v)
    _, grads = term(bc, "tc", leaves(upload(v)))
    want = serial_scatter(v)
    assert not np.array_equal(want, serial_scatter(v, reverse=True))
    assert grads["prev_img"].cpu().numpy().tobytes() == want.tobytes()


def sobel_images():
    rng = np.random.default_rng(11)
    ramp = (np.arange(6, dtype=F)[None, :] * F(0.5) + np.arange(5, dtype=F)[:, None] * F(0.25))[None, None]
    rand = rng.uniform(-1, 1, (3, 2, 9, 7)).astype(F)
    border = np.full((2, 1, 6, 8), F(0.3))
    border[:, :, 0, :], border[:, :, -1, :] = rng.uniform(0, 1, (2, 1, 8)), rng.uniform(0, 1, (2, 1, 8))
    border[:, :, :, 0], border[:, :, :, -1] = rng.uniform(0, 1, (2, 1, 6)), rng.uniform(0, 1, (2, 1, 6))
    wide = rng.uniform(-1, 1, (1, 1, 19, 300)).astype(F)                  # more than one block, no multiple of it
    return {"ramp": ramp, "random": rand, "border": border.astype(F), "wide": wide}


@pytest.mark.parametrize("name", ["ramp", "random", "border", "wide"])
def test_sobel_forward_and_backward(golden, BC, name):
    x = sobel_images()[name]
    B, C, H, W = x.shape
    rng = np.random.default_rng(5)
    ggx, ggy = rng.uniform(-1, 1, (B * C, 1, H, W)).astype(F), rng.uniform(-1, 1, (B * C, 1, H, W)).astype(F)
    sobel = BC.Sobel("cuda")
    t = dev(x).requires_grad_(True)
    keep = t.detach().clone()
    outs = []
    for _ in range(2):
        gx, gy = sobel(t)
        (g,) = torch.autograd.grad([gx, gy], [t], [dev(ggx), dev(ggy)])
        outs.append((gx.detach(), gy.detach(), g))
    for a, b in zip(*outs):
        assert raw(a) == raw(b)
    assert raw(t) == raw(keep)
    gx, gy, g = outs[0]
    assert tuple(gx.shape) == tuple(gy.shape) == (B * C, 1, H, W) and tuple(g.shape) == x.shape
    want_x, want_y = R.sobel(x.reshape(B * C, H, W))
    want_g = R.sobel_adjoint(ggx[:, 0], ggy[:, 0]).reshape(x.shape)
    _, bar = bars(golden)
    for what, got, want in (("gradx", gx[:, 0], want_x), ("grady", gy[:, 0], want_y), ("adjoint", g, want_g)):
        err = np.abs(got.cpu().numpy().astype(np.float64) - want).max() / np.abs(want).max()
        print("sobel %s %s: error %.3g of the largest element (bar %.3g)" % (name, what, err, bar))
        assert err <= bar, what
    if name == "ramp":                                        # exact: 4 * 0.5 * 2 / 8 inside, half of it at the replicated border
        assert torch.equal(gx[0, 0, :, 1:-1], torch.full((5, 4), 0.5, device="cuda")) and torch.equal(gx[0, 0, :, 0], torch.full((5,), 0.25, device="cuda"))
        assert torch.equal(gy[0, 0, 1:-1, :], torch.full((3, 6), 0.25, device="cuda"))
    # one output alone: the other draws no gradient
    gx, gy = sobel(t)
    (g1,) = torch.autograd.grad(gx, t, dev(ggx))
    want = R.sobel_adjoint(ggx[:, 0], np.zeros_like(ggx[:, 0])).reshape(x.shape)
    assert np.abs(g1.cpu().numpy() - want).max() <= bar * np.abs(want).max()


def odd_case(B, H, W, n, seed):
    """Inputs under the fixture's kink conditions at a size that is no multiple of any tile.  With an odd H or W the zero-flow
    coordinate p * n / (n - 1) - 0.5 is integral in the middle, so a masked pixel that offends is unmasked."""
    rng = np.random.default_rng(seed)
    draw = lambda: rng.uniform(-0.03, 0.03, (B, 2, H, W)).astype(F)
    ev = np.zeros((B, n, 4), F)
    ev[:, :, 0] = rng.uniform(0.02, 0.98, (B, n))
    ev[:, :, 1], ev[:, :, 2] = rng.integers(0, H, (B, n)), rng.integers(0, W, (B, n))
    ev[:, :, 3] = rng.choice([-1.0, 1.0], (B, n))
    cnt = rng.integers(0, 3, (B, 2, H, W)).astype(F)
    cnt[:, :, :, : W // 3] = 0
    v = dict(flow=draw(), img=rng.uniform(0, 1, (B, 1, H, W)).astype(F), prev_img=rng.uniform(0, 1, (B, 1, H, W)).astype(F), cnt=cnt,
             events=ev, pol_mask=np.stack([ev[:, :, 3] > 0, ev[:, :, 3] < 0], axis=2).astype(F), res=(H, W),
             weights=np.array([0.1, 0.5]))
    for _ in range(200):
        bad = R.kinks(v["flow"], v["cnt"], v["prev_img"], v["img"], v["res"])
        if not bad.any():
            break
        fresh = draw()
        for ch in range(2):
            v["flow"][:, ch][bad] = fresh[:, ch][bad]
            v["cnt"][:, ch][bad] = 1
        v["img"][:, 0][bad] = rng.uniform(0, 1, int(bad.sum()))
        v["prev_img"][:, 0][bad] = rng.uniform(0, 1, int(bad.sum()))
    return v


@pytest.mark.parametrize("shape", [(1, 70, 130), (2, 33, 66)])
def test_odd_sizes_against_the_float64_restatement(golden, BC, shape):
    B, H, W = shape
    v = odd_case(B, H, W, 3000, seed=H)
    assert not R.kinks(v["flow"], v["cnt"], v["prev_img"], v["img"], v["res"]).any()
    masked = v["cnt"].sum(axis=1) == 0
    assert 0.1 < masked.mean() < 0.5 and (B * H * W) % 256 != 0 and (4 * B * H * W) % 1024 != 0
    bc = module(BC, v)
    t = leaves(upload(v))
    avg = bc.averaged_iwe(dev(R.masked_flow(v["flow"], v["cnt"])), t["events"], t["pol_mask"])
    assert avg.any()
    want = {}
    want["gen"] = R.generative(v["flow"], v["img"], v["cnt"], avg.cpu().numpy(), v["res"])
    want["tc"] = R.temporal(v["flow"], v["prev_img"], v["img"], v["res"], v["weights"][1])
    want["tv"] = R.total_variation(v["img"], v["weights"][0])
    for which in sorted(TERMS):
        loss, grads = term(bc, which, t)
        again, grads2 = term(bc, which, t)
        assert raw(loss) == raw(again) and all(raw(grads[k]) == raw(grads2[k]) for k in grads)
        check(golden, "%dx%dx%d %s" % (B, H, W, which), loss, grads, float(want[which][0]), dict(zip(TERMS[which], want[which][1:])))
    _, grads = term(bc, "gen", t)
    at = grads["flow"][dev(masked)[:, None].expand(-1, 2, -1, -1)]
    assert not at.view(torch.int32).any()


def test_flow_variants_and_upstream_factor(golden, BC):
    """A strided flow (a channel-sliced view) and a non-leaf flow (2 * leaf) give the gradients of the contiguous leaf, times
    2 for the latter; an upstream factor of 0.37 scales every gradient."""
    v = case(golden, "general")
    bc = module(BC, v)
    base = upload(v)
    B, _, H, W = v["flow"].shape
    for which in ("gen", "tc"):
        plain = leaves(base)
        loss, grads = term(bc, which, plain)
        wide = torch.zeros((B, 5, H, W), device="cuda")
        wide[:, 1:5:2] = base["flow"]
        wide.requires_grad_(True)
        view = wide[:, 1:5:2]                                            # channels 1 and 3 of five
        assert not view.is_contiguous() and not view.is_leaf
        loss_s, grads_s = term(bc, which, dict(plain, flow=view, flow_leaf=wide))
        assert raw(loss_s) == raw(loss)
        assert raw(grads_s["flow"][:, 1:5:2].contiguous()) == raw(grads["flow"]) and not grads_s["flow"][:, 0:5:2].any()
        for k in TERMS[which][1:]:
            assert raw(grads_s[k]) == raw(grads[k]), k
        half = (base["flow"] * 0.5).requires_grad_(True)
        loss_n, grads_n = term(bc, which, dict(plain, flow=2 * half, flow_leaf=half))
        assert raw(loss_n) == raw(loss) and raw(grads_n["flow"]) == raw(2 * grads["flow"])
    for which in sorted(TERMS):
        t = leaves(base)
        loss, grads = term(bc, which, t, upstream=0.37)
        want = {k: golden["general__%s_%s64" % (which, GRAD_KEY[k])] for k in TERMS[which]}
        check(golden, "general %s x 0.37" % which, loss, grads, float(golden["general__%s_loss64" % which]), want, scale=0.37)
    # a term whose image needs no gradient sorts nothing and gives the same flow gradient
    plain = leaves(base)
    for which, frozen in (("gen", ("img",)), ("tc", ("prev_img",)), ("tc", ("prev_img", "img"))):
        _, grads = term(bc, which, plain)
        some = dict(plain, **{k: base[k] for k in frozen})
        inputs = {"inp_cnt": some["cnt"], "inp_list": some["events"], "inp_pol_mask": some["pol_mask"]}
        loss = bc.generative_model(some["flow"], some["img"], inputs) if which == "gen" else bc.temporal_consistency(some["flow"], some["prev_img"], some["img"])
        (g,) = torch.autograd.grad(loss, some["flow"])
        assert raw(g) == raw(grads["flow"])


@pytest.mark.parametrize("name", ["general", "pile"])
def test_all_terms_replay_from_one_graph(golden, BC, name):
    v = case(golden, name)
    bc = module(BC, v)
    t = leaves(upload(v))

    def everything():
        out = []
        for which in ("gen", "tc", "tv"):
            loss, grads = term(bc, which, t)
            out += [loss] + [grads[k] for k in TERMS[which]]
        return out
    eager = [a.clone() for a in everything()]
    torch.cuda.synchronize()
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        main = torch.cuda.current_stream()
        captured = everything()
        assert torch.cuda.current_stream() == main and torch.cuda.is_current_stream_capturing()
    for _ in range(3):
        for a in captured:
            a.zero_()
        graph.replay()
        torch.cuda.synchronize()
        for a, b in zip(captured, eager):
            assert raw(a) == raw(b)


def test_a_non_finite_coordinate_samples_zero_and_passes_no_gradient(golden, BC):
    v = case(golden, "nomask")
    v["cnt"] = np.ones_like(v["cnt"])
    flow = np.array(v["flow"])
    spots = [(0, 1, 2), (1, 3, 4), (1, 5, 7)]
    for (b, h, w), (fx, fy) in zip(spots, ((np.nan, 0.01), (0.02, np.inf), (-np.inf, np.nan))):
        flow[b, 0, h, w], flow[b, 1, h, w] = fx, fy
    far = np.array(v["flow"])
    for b, h, w in spots:
        far[b, :, h, w] = 50.0                                             # finite, every corner far outside: samples 0 too
    bc = module(BC, v)
    t_bad, t_far = leaves(upload(dict(v, flow=flow))), leaves(upload(dict(v, flow=far)))
    loss_b, grads_b = term(bc, "tc", t_bad)
    loss_f, grads_f = term(bc, "tc", t_far)
    assert torch.isfinite(loss_b) and raw(loss_b) == raw(loss_f)
    for k in ("prev_img", "img"):
        assert raw(grads_b[k]) == raw(grads_f[k]) and torch.isfinite(grads_b[k]).all()
    assert torch.isfinite(grads_b["flow"]).all()
    for b, h, w in spots:
        assert not grads_b["flow"][b, :, h, w].any()
    loss_b, grads_b = term(bc, "gen", t_bad)                               # the averaged image drops those events either way
    loss_f, grads_f = term(bc, "gen", t_far)
    assert torch.isfinite(loss_b) and raw(loss_b) == raw(loss_f) and raw(grads_b["img"]) == raw(grads_f["img"])
    assert torch.isfinite(grads_b["flow"]).all() and torch.isfinite(grads_b["img"]).all()
    for b, h, w in spots:
        assert not grads_b["flow"][b, :, h, w].any()


def test_the_reference_trainers_import_lines_work():
    ns = {}
    exec("from loss import *\nfrom myutils.gradients import Sobel", ns)
    assert callable(ns["BrightnessConstancy"]) and callable(ns["Sobel"]) and callable(ns["AveragedIWE"])
