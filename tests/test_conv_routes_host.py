"""Host-side checks of tests/conv_routes_ref.py: the mode statements and their gradients, that the bound of the GPU tests rejects
planted kernel defects at the shapes of the case table, and that the table reaches every route it is there for.  Nothing here
computes on a GPU: the fp32 CPU statement stands in for the device."""
import functools
import os
import sys

import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import conv_routes_ref as R  # noqa: E402

IDS = [c.id for c in R.CASES]
X3_IDS = [c.id for c in R.CASES if any(R.route(c)[1].get(n) == "bf16x3" for n in R.wanted(c))]
LEAKY_IDS = [c.id for c in R.CASES if c.act == R.LEAKY and not c.gpre and R.wanted(c) != ["y"]]
GB_IDS = [c.id for c in R.CASES if "gb" in R.wanted(c)]


# ------------------------------------------------------------------------------------------------ statements and gradients
@pytest.mark.parametrize("arith", ["fp32", "bf16", "bf16x3", "f16"])
@pytest.mark.parametrize("k,s,p", [(3, 1, 1), (3, 2, 0), (3, 1, 3), (1, 1, 1), (7, 2, 2)])
def test_gradient_statements_are_the_adjoints_of_the_forward_statement(arith, k, s, p):
    """Sum over the operand images of conv2d_input / conv2d_weight == float64 autograd of the forward statement on the same images."""
    c = R.C("t", "t", "t", "fp32", (2, 5, 9, 10, 4, k, s, p))
    gen = torch.Generator().manual_seed(k * 100 + s * 10 + p)
    x, w = torch.randn(2, 5, 9, 10, generator=gen), torch.randn(4, 5, k, k, generator=gen)
    g = torch.randn(2, 4, *R.out_hw(c.shape), generator=gen)
    fwd, dgrad, wgrad = R.ops(c)
    sc = {n: R.scale_law(t.abs().max()) for n, t in (("x", x), ("w", w), ("g", g))}
    dt = torch.float64
    # data gradient: images of (g, w); d/dX of sum_i <conv64(X, w_i), g_i>
    pairs = R.images(g, w, arith, sc["g"], sc["w"])
    X = torch.zeros(2, 5, 9, 10, dtype=dt, requires_grad=True)
    sum((fwd(X, b.to(dt)) * a.to(dt)).sum() for a, b in pairs).backward()
    got = R.evaluate(dgrad, pairs, dt)
    assert (got - X.grad).abs().max() <= 1e-12 * X.grad.abs().max()
    # weight gradient: images of (x, g); d/dW of sum_i <conv64(x_i, W), g_i>
    pairs = R.images(x, g, arith, sc["x"], sc["g"])
    Wt = torch.zeros(4, 5, k, k, dtype=dt, requires_grad=True)
    sum((fwd(a.to(dt), Wt) * b.to(dt)).sum() for a, b in pairs).backward()
    got = R.evaluate(wgrad, pairs, dt)
    assert (got - Wt.grad).abs().max() <= 1e-12 * Wt.grad.abs().max()


def test_images_are_what_the_modes_say():
    gen = torch.Generator().manual_seed(5)
    v = torch.randn(1000, generator=gen) * torch.logspace(-6, 6, 1000)
    h, l = R.split(v)
    assert torch.equal(h, v.bfloat16().float()) and torch.equal(l, (v - h).bfloat16().float())
    assert ((v - h).abs() <= 2.0 ** -8 * v.abs()).all() and ((v.double() - h.double() - l.double()).abs() <= 2.0 ** -16 * v.abs().double()).all()
    s = R.scale_law(v.abs().max())
    assert 2 <= v.abs().max().item() * s < 4 and s == 2.0 ** round(torch.log2(torch.tensor(s)).item())
    assert torch.equal(R.q16(v, s), (v * s).half().double() / s)
    assert R.scale_law(0.0) == 1.0 and R.scale_law(float("inf")) == 1.0 and R.scale_law(1e-45) == 2.0 ** 120
    from ebfi_amd import f16scale
    for a in (1e-30, 0.3, 0.5, 1.0, 3.999, 4.0, 7e4):
        assert f16scale.next_scale(torch.tensor(a)).item() == R.scale_law(torch.tensor(a).float())


@pytest.mark.parametrize("k,s,p", [(3, 1, 1), (1, 1, 0), (7, 1, 3), (3, 1, 3)])
def test_split_precision_statement_is_within_2e15_of_the_plain_conv(k, s, p):
    """|S64_bf16x3 - conv64(x, w)| <= 2^-15 * conv64(|x|, |w|) componentwise: the dropped lo*lo product and the rounding of the lo
    images are each <= 2^-18 relative per term."""
    c = R.C("t", "t", "t", "fp32", (2, 20, 9, 37, 12, k, s, p))
    gen = torch.Generator().manual_seed(k + p)
    x, w = torch.randn(2, 20, 9, 37, generator=gen), torch.randn(12, 20, k, k, generator=gen)
    fwd = R.ops(c)[0]
    dt = torch.float64
    plain, mag = fwd(x.to(dt), w.to(dt)), fwd(x.abs().to(dt), w.abs().to(dt))
    x3 = R.evaluate(fwd, R.images(x, w, "bf16x3"), dt)
    assert ((x3 - plain).abs() <= 2.0 ** -15 * mag).all()
    assert (x3 - plain).abs().max() > 0                     # (an emulation that does nothing would pass the line above)
    one = R.evaluate(fwd, R.images(x, w, "bf16"), dt)
    assert not ((one - plain).abs() <= 2.0 ** -15 * mag).all()


# ------------------------------------------------------------------------------------------------ the bound has teeth
@functools.lru_cache(maxsize=None)
def _stand_in(cid):
    """(S32, S64, scales, labels) of the case with the fp32 CPU statement as the device (its own y gives act')"""
    c = R.BY_ID[cid]
    x, w, b, g = R.inputs(cid)
    sc = R.first_use_scales(c, x, w, g) if c.bank else None
    s32 = R.statement(c, None, torch.float32, sc)
    s64 = R.statement(c, s32["y"], torch.float64, sc)
    return s32, s64, sc, R.route(c)[0]


def _rejected(c, names, planted):
    s32, s64, sc, labels = _stand_in(c.id)
    return R.check_bound(c.id, planted, s64, s32, names, labels, out=lambda s: None)


@pytest.mark.parametrize("cid", IDS)
def test_unplanted_stand_in_passes(cid):
    c = R.BY_ID[cid]
    s32, s64, sc, labels = _stand_in(cid)
    assert not R.check_bound(cid, s32, s64, s32, R.wanted(c), labels)
    # ... and so does another fp32 evaluation order of the same statement (the images accumulated in reverse)
    rev = R.statement(c, s32["y"], torch.float32, sc, tweak=lambda name, op, pairs, dt: R.evaluate(op, pairs[::-1], dt))
    assert not R.check_bound(cid + " (reversed)", rev, s64, s32, R.wanted(c), labels)


def _block(n):
    return slice(0, min(16, n))


@pytest.mark.parametrize("cid", X3_IDS)
def test_bound_rejects_a_dropped_hi_lo_product(cid):
    """one hi*lo product dropped at one tap of one 16-channel block, in every result the case computes in split precision"""
    c = R.BY_ID[cid]
    ar = R.route(c)[1]
    names = [n for n in R.wanted(c) if ar.get(n) == "bf16x3"]
    k = c.shape[5]
    ky, kx = k // 2, k - 1
    s32, _, sc, _ = _stand_in(cid)

    def tweak(name, op, pairs, dt):
        if ar.get(name) != "bf16x3":
            return R.evaluate(op, pairs, dt)
        (al, bh), (ah, bl), (ah2, bh2) = pairs
        if name in ("y", "gx"):                       # b = the weight: the tap of one input-channel block
            cut = bl.clone()
            cut[:, _block(bl.shape[1]), ky, kx] = 0
            return R.evaluate(op, [(al, bh), (ah, cut), (ah2, bh2)], dt)
        full = R.evaluate(op, pairs, dt)              # gw: the tap IS the result's index
        full[:, _block(full.shape[1]), ky, kx] -= op(ah.to(dt), bl.to(dt))[:, _block(full.shape[1]), ky, kx]
        return full
    planted = R.statement(c, s32["y"], torch.float32, sc, tweak=tweak)
    bad = {n for n, *_ in _rejected(c, names, planted)}
    assert bad == set(names), (cid, names, bad)


@pytest.mark.parametrize("cid", IDS)
def test_bound_rejects_a_halo_one_pixel_off_on_the_last_row(cid):
    c = R.BY_ID[cid]
    s32, _, sc, _ = _stand_in(cid)
    B, Cin, H, W, Cout, k, s, p = c.shape
    last = min(R.out_hw(c.shape)[0] - 1, (H - 1 + p) // s)       # the last output row whose window meets the input (pad == k: not Ho-1)

    def tweak(name, op, pairs, dt):
        out = R.evaluate(op, pairs, dt)
        if name == "y":
            out[:, :, last, :] = R.evaluate(op, [(torch.roll(a, 1, dims=3), b) for a, b in pairs], dt)[:, :, last, :]
        return out
    planted = R.statement(c, s32["y"], torch.float32, sc, tweak=tweak)
    assert [n for n, *_ in _rejected(c, ["y"], planted)] == ["y"]


@pytest.mark.parametrize("cid", LEAKY_IDS)
def test_bound_rejects_a_leaky_derivative_of_one_at_a_negative_output(cid):
    c = R.BY_ID[cid]
    names = [n for n in R.wanted(c) if n != "y"]
    s32, _, sc, _ = _stand_in(cid)

    def gp_tweak(gp, g, y):
        neg = y <= 0                                   # (slope 0: a negative pre-activation leaves as 0)
        ring = max(c.shape[7] - (c.shape[5] - 1), 0)   # (pad == k: the outer ring reaches no input pixel and no weight gradient)
        if ring:
            neg[:, :, :ring], neg[:, :, -ring:], neg[:, :, :, :ring], neg[:, :, :, -ring:] = False, False, False, False
        gp = gp.clone().reshape(-1)
        i = int(neg.reshape(-1).nonzero()[0])
        gp[i] = g.reshape(-1)[i]
        return gp.view_as(g)
    planted = R.statement(c, s32["y"], torch.float32, sc, gp_tweak=gp_tweak)
    bad = {n for n, *_ in _rejected(c, names, planted)}
    assert bad == set(names), (cid, names, bad)


@pytest.mark.parametrize("cid", IDS)
def test_bound_rejects_a_tile_written_twice(cid):
    c = R.BY_ID[cid]
    s32, _, _, _ = _stand_in(cid)
    planted = dict(s32, y=s32["y"].clone())
    planted["y"][-1, :32, :8, :64] *= 2
    assert [n for n, *_ in _rejected(c, ["y"], planted)] == ["y"]


@pytest.mark.parametrize("cid", GB_IDS)
def test_bound_rejects_a_bias_gradient_missing_a_row_band(cid):
    c = R.BY_ID[cid]
    s32, _, sc, _ = _stand_in(cid)
    x, w, b, g = R.inputs(cid)
    gp = g if c.gpre else R.grad_preact(g, s32["y"], c.act, c.slope)
    band = min(8, gp.shape[2] - 1)
    planted = dict(s32, gb=gp[:, :, band:, :].sum(dim=(0, 2, 3)))
    assert [n for n, *_ in _rejected(c, ["gb"], planted)] == ["gb"]


# ------------------------------------------------------------------------------------------------ the case table is closed
def test_every_required_route_is_claimed_by_a_case():
    routes = [(c,) + R.route(c) for c in R.CASES]
    missing = [name for name, pred in R.REQUIRED if not any(pred(c, labels, inst) for c, labels, ar, inst in routes)]
    assert not missing, missing
    for name, pred in R.REQUIRED:
        print("%-80s %s" % (name, ", ".join(c.id for c, labels, ar, inst in routes if pred(c, labels, inst))))


def test_every_case_states_its_instance_and_predicts_its_results():
    for c in R.CASES:
        labels, ar, inst = R.route(c)
        assert c.why and len(c.why) > 10, c.id
        assert labels and all(l.startswith("conv") and l not in R.HELPERS for l in labels), (c.id, labels)
        assert set(R.wanted(c)) - {"gb"} <= set(ar), (c.id, ar)
        assert set(c.subset) <= set("xwb") and set(c.mis) <= set("xg") and c.layout in ("", "slice", "sum")


def test_no_fp16_case_stages_a_subnormal():
    n = 0
    for c in R.CASES:
        if not c.bank:
            continue
        labels, ar, inst = R.route(c)
        x, w, b, g = R.inputs(c.id)
        sc = R.first_use_scales(c, x, w, g)
        s32, _, _, _ = _stand_in(c.id)
        gp = R.grad_preact(g, s32["y"], c.act, c.slope)
        staged = []
        if ar.get("gw") == "f16":
            staged += [x * sc["x"], gp * sc["g"]]
        if ar.get("gx") == "f16":
            staged += [gp * sc["g"], w * sc["w"]]
        for t in staged:
            n += 1
            assert R.F16_MIN_NORMAL <= t.abs().min().item() and t.abs().max().item() < 4, c.id
    assert n >= 8
