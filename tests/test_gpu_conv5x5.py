"""The 5x5 convolution kernels through the C ABI (ebfi_conv5x5_* of include/ebfi_hip.h, csrc/conv2d.hip): forward at stride 1
and 2, the stride-1 data gradient (the forward kernel on the transposed filter), the stride-2 data gradient by output parity
(conv5s2_dgrad_f32) and the slab weight / bias gradient, against torch's CPU convolution and torch.nn.grad.conv2d_input /
conv2d_weight in float64.

Bound (tests/conv_routes_ref.py): per result eK <= 8 * e32 + 4 * 2^-24 * max|S64|, e32 the error of the same statement in CPU
float32.  Every figure is printed.  The test supplies saved_output itself, bounded away from zero (|y| in [0.1, 1] for the
LeakyReLU kinds, y in [0.05, 0.95] for the sigmoid): no mask is ambiguous, and g * act'(y) in CPU float32 is the very value the
kernels multiply, so the side output grad_preact_out is compared bit for bit.  Outputs and the workspace are pre-filled with NaN
and every result must come back finite everywhere; every gradient runs twice and must give the same bytes.

The table covers, at stride 2, H + 2 pad - 5 even and odd in each axis for every pad 0..4, maps down to 1 x 1 and 2 x 3, more
than one row / column tile of the parity kernel; output widths 64 / 65 and heights 4 / 5 (the forward tile), 28 / 29 at stride 1
and 30 / 31 at stride 2 (the weight gradient's width tile WTX and WTX + 1); Cin in {1, 5, 7, 17, 33, 40} (17: one past the
weight gradient's 16-channel block; > 32: the second row block of the data gradients), Cout in {1, 3, 32, 33, 65}; B = 2.
"""
import functools
import os
import sys

import pytest
import torch
import torch.nn.functional as F

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import conv_routes_ref as R  # noqa: E402

from ebfi_amd import _native as N  # noqa: E402

pytestmark = pytest.mark.gpu

NONE, LEAKY, SIGMOID = R.NONE, R.LEAKY, R.SIGMOID
RELU = (LEAKY, 0.0)
LK = (LEAKY, 0.1)
SG = (SIGMOID, 0.0)
NO = (NONE, 0.0)


def _table():
    t = []

    def add(tag, B, Cin, H, W, Cout, s, p, act, bias, gpre):
        t.append((tag, (B, Cin, H, W, Cout, s, p), act, bias, gpre))
    # ---- stride 1
    add("s1_ragged", 2, 5, 9, 37, 3, 1, 2, LK, True, True)
    add("s1_Ho4_Wo64", 2, 7, 4, 64, 32, 1, 2, NO, False, False)
    add("s1_Ho5_Wo65", 2, 1, 5, 65, 33, 1, 2, RELU, True, True)
    add("s1_Wo28_wtx", 2, 17, 6, 28, 65, 1, 2, SG, True, True)
    add("s1_Wo29_wtx1", 2, 17, 6, 29, 1, 1, 2, LK, False, False)
    add("s1_pad0", 2, 5, 9, 37, 3, 1, 0, RELU, True, False)
    add("s1_pad1", 2, 7, 9, 37, 3, 1, 1, SG, False, True)
    add("s1_pad3", 2, 5, 9, 37, 3, 1, 3, NO, True, False)
    add("s1_pad4", 2, 7, 9, 37, 3, 1, 4, LK, True, True)
    add("s1_Cin33", 2, 33, 5, 7, 5, 1, 2, RELU, True, True)
    add("s1_1x1", 2, 3, 1, 1, 3, 1, 2, LK, True, True)
    add("s1_2x3", 2, 3, 2, 3, 4, 1, 2, SG, False, False)
    # ---- stride 2: every pad, H + 2 pad - 5 even / odd in each axis
    kinds = [LK, NO, RELU, SG, LK]
    for p in range(5):
        add("s2_pad%d_even_odd" % p, 2, 5, 9, 12, 3, 2, p, kinds[p], p % 2 == 0, p % 2 == 1)
        add("s2_pad%d_odd_even" % p, 2, 7, 10, 11, 3, 2, p, kinds[(p + 2) % 5], p % 2 == 1, p % 2 == 0)
    add("s2_pad2_even_even", 2, 5, 9, 11, 3, 2, 2, SG, True, True)
    add("s2_pad2_odd_odd", 2, 5, 10, 12, 3, 2, 2, RELU, False, False)
    add("s2_1x1", 2, 3, 1, 1, 4, 2, 2, LK, True, True)
    add("s2_2x3", 2, 3, 2, 3, 4, 2, 2, RELU, True, True)
    add("s2_Ho4_Wo64", 2, 7, 7, 127, 32, 2, 2, NO, True, False)
    add("s2_Ho5_Wo65", 2, 1, 9, 129, 33, 2, 2, LK, False, True)
    add("s2_Wo30_wtx", 2, 17, 6, 59, 65, 2, 2, SG, True, True)
    add("s2_Wo31_wtx1", 2, 17, 5, 61, 1, 2, 2, RELU, True, True)
    add("s2_Cin40", 2, 40, 9, 12, 5, 2, 2, LK, True, True)
    add("s2_rows3tiles", 2, 5, 19, 12, 3, 2, 1, SG, False, True)
    add("s2_cols2tiles_pad0", 2, 3, 6, 133, 3, 2, 0, RELU, True, False)
    add("s2_cols2tiles_pad3", 2, 3, 5, 130, 33, 2, 3, LK, True, True)
    add("s2_pad4_tiny", 2, 1, 1, 2, 3, 2, 4, NO, True, False)
    assert len({c[0] for c in t}) == len(t)
    return t


TABLE = _table()
BY_TAG = {c[0]: c for c in TABLE}


def _out_hw(geo):
    B, Cin, H, W, Cout, s, p = geo
    return (H + 2 * p - 5) // s + 1, (W + 2 * p - 5) // s + 1


@functools.lru_cache(maxsize=None)
def _reference(tag):
    """inputs (CPU fp32) and the float64 / float32 statements of the case: computed once, shared, never modified."""
    _, geo, (act, slope), bias, _ = BY_TAG[tag]
    B, Cin, H, W, Cout, s, p = geo
    Ho, Wo = _out_hw(geo)
    gen = torch.Generator().manual_seed(9000 + [c[0] for c in TABLE].index(tag))
    x = torch.randn(B, Cin, H, W, generator=gen)
    w = torch.randn(Cout, Cin, 5, 5, generator=gen) / (Cin * 25) ** 0.5
    b = torch.randn(Cout, generator=gen) * 0.1 if bias else None
    g = torch.randn(B, Cout, Ho, Wo, generator=gen)
    u = torch.rand(B, Cout, Ho, Wo, generator=gen)
    if act == SIGMOID:
        ysaved = 0.05 + 0.9 * u
    else:                                       # bounded away from zero, both signs
        ysaved = (0.1 + 0.9 * u) * (torch.randint(0, 2, u.shape, generator=gen) * 2 - 1).float()
    gp = R.grad_preact(g, ysaved, act, slope) if act != NONE else g
    st = {}
    for dt in (torch.float64, torch.float32):
        pre = F.conv2d(x.to(dt), w.to(dt), None if b is None else b.to(dt), s, p)
        st[dt] = {"y": R.act_fwd(pre, act, slope),
                  "gx": torch.nn.grad.conv2d_input((B, Cin, H, W), w.to(dt), gp.to(dt), stride=s, padding=p),
                  "gw": torch.nn.grad.conv2d_weight(x.to(dt), (Cout, Cin, 5, 5), gp.to(dt), stride=s, padding=p),
                  "gb": gp.to(dt).sum(dim=(0, 2, 3))}
    return dict(x=x, w=w, b=b, g=g, ysaved=ysaved if act != NONE else None, gp=gp, s64=st[torch.float64], s32=st[torch.float32])


def _nan(*shape):
    return torch.full(shape, float("nan"), device="cuda")


def _dev(t):
    return None if t is None else t.cuda().contiguous()


def _bytes(t):
    return t.cpu().numpy().tobytes()


@pytest.mark.parametrize("tag", [c[0] for c in TABLE])
def test_conv5x5_kernels_against_float64(tag):
    _, geo, (act, slope), bias, want_gpre = BY_TAG[tag]
    B, Cin, H, W, Cout, s, p = geo
    Ho, Wo = _out_hw(geo)
    ref = _reference(tag)
    lib, st = N.lib(), N.stream_ptr()
    x, w, b, g, ys = (_dev(ref[k]) for k in ("x", "w", "b", "g", "ysaved"))
    got = {}
    # ---- forward
    y = _nan(B, Cout, Ho, Wo)
    N.check(lib.ebfi_conv5x5_forward(N.ptr(x), N.ptr(w), N.ptr(b), N.ptr(y), *geo, act, slope, st), tag)
    got["y"] = y.cpu()
    # ---- weight / bias gradient, twice
    need = int(lib.ebfi_conv5x5_backward_weight_workspace(*geo))
    assert need > 0
    runs = []
    for _ in range(2):
        ws = torch.full((need // 4,), float("nan"), device="cuda")
        gw, gb = _nan(Cout, Cin, 5, 5), (_nan(Cout) if bias else None)
        gpre = _nan(B, Cout, Ho, Wo) if want_gpre else None
        N.check(lib.ebfi_conv5x5_backward_weight(N.ptr(x), N.ptr(g), N.ptr(ys), N.ptr(gw), N.ptr(gb), N.ptr(gpre), *geo, act, slope,
                                                 N.ptr(ws), need, st), tag)
        runs.append((gw, gb, gpre))
    assert _bytes(runs[0][0]) == _bytes(runs[1][0])
    if bias:
        assert _bytes(runs[0][1]) == _bytes(runs[1][1])
    got["gw"] = runs[0][0].cpu()
    names = ["y", "gw"]
    if bias:
        got["gb"] = runs[0][1].cpu()
        names.append("gb")
    if want_gpre:                                # the values the kernel multiplied: grad_output * act', bit for bit
        assert torch.equal(runs[0][2].cpu(), ref["gp"]) and torch.equal(runs[1][2].cpu(), ref["gp"])
    # ---- data gradient with the derivative folded into the staging, twice; then on the side output
    dx = []
    for _ in range(2):
        gx = _nan(B, Cin, H, W)
        N.check(lib.ebfi_conv5x5_backward_data(N.ptr(g), N.ptr(ys), N.ptr(w), N.ptr(gx), *geo, act, slope, st), tag)
        dx.append(gx)
    assert _bytes(dx[0]) == _bytes(dx[1])
    got["gx"] = dx[0].cpu()
    names.append("gx")
    bad = R.check_bound(tag, got, ref["s64"], ref["s32"], names)
    if want_gpre:
        gx = _nan(B, Cin, H, W)
        N.check(lib.ebfi_conv5x5_backward_data(N.ptr(runs[0][2]), N.ptr(None), N.ptr(w), N.ptr(gx), *geo, NONE, 0.0, st), tag)
        bad += R.check_bound(tag + " (gx from grad_preact_out)", {"gx": gx.cpu()}, ref["s64"], ref["s32"], ["gx"])
    assert all(torch.isfinite(v).all() for v in got.values())
    assert not bad, bad
    # the inputs are untouched
    assert torch.equal(x.cpu(), ref["x"]) and torch.equal(g.cpu(), ref["g"]) and torch.equal(w.cpu(), ref["w"])


def test_rows_and_columns_no_window_reaches_are_zero():
    """H + 2 pad - 5 odd at stride 2 and no padding to absorb the spare line: the last input row / column lies in no window;
    grad_input there is written, as zero."""
    lib, st = N.lib(), N.stream_ptr()
    geo = (2, 3, 10, 12, 4, 2, 0)                # H - 5 = 5, W - 5 = 7: both odd
    Ho, Wo = _out_hw(geo)
    gen = torch.Generator().manual_seed(5)
    g, w = torch.randn(2, 4, Ho, Wo, generator=gen).cuda(), torch.randn(4, 3, 5, 5, generator=gen).cuda()
    gx = _nan(2, 3, 10, 12)
    N.check(lib.ebfi_conv5x5_backward_data(N.ptr(g), N.ptr(None), N.ptr(w), N.ptr(gx), *geo, NONE, 0.0, st), "zeros")
    assert torch.isfinite(gx).all()
    last_row, last_col = 2 * (Ho - 1) + 4, 2 * (Wo - 1) + 4      # where the window of the last output row / column ends
    assert last_row == 10 - 2 and last_col == 12 - 2
    assert not gx[:, :, last_row + 1:].any() and not gx[:, :, :, last_col + 1:].any()
    assert gx[:, :, :last_row + 1, :last_col + 1].abs().min() > 0


def test_empty_batch_is_a_no_op_and_the_weight_gradient_zero_fills():
    lib, st = N.lib(), N.stream_ptr()
    geo = (0, 3, 8, 8, 4, 2, 2)
    t = _nan(16)
    gw, gb = _nan(4, 3, 5, 5), _nan(4)
    assert lib.ebfi_conv5x5_forward(N.ptr(t), N.ptr(t), N.ptr(None), N.ptr(t), *geo, 0, 0.0, st) == 0
    assert lib.ebfi_conv5x5_backward_data(N.ptr(t), N.ptr(None), N.ptr(t), N.ptr(t), *geo, 0, 0.0, st) == 0
    need = int(lib.ebfi_conv5x5_backward_weight_workspace(*geo))
    ws = torch.empty(max(need, 4), dtype=torch.uint8, device="cuda")
    assert lib.ebfi_conv5x5_backward_weight(N.ptr(t), N.ptr(t), N.ptr(None), N.ptr(gw), N.ptr(gb), N.ptr(None), *geo, 0, 0.0,
                                            N.ptr(ws), need, st) == 0
    assert torch.isnan(t).all() and not gw.any() and not gb.any()
