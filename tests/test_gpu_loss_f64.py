"""csrc/laploss.hip against float64 (tests/loss_ref64.py, itself held by test_loss_f64_host.py), through the C ABI.

The L1 gradient is a sign, so the kernels are checked in the two halves the workspace separates:
  (A) the sign field ebfi_laploss_forward leaves in the workspace, element by element: bit-equal to coef * 2^l * sign(lap64) where
      |lap64| > tau_l, exactly 0 where the whole footprint is zero, one of -v, 0, +v elsewhere; bit-identical when repeated;
  (B) ebfi_laploss_backward, a linear map of the workspace, on the field the device itself produced and (B') on arbitrary fields
      (randn, and magnitudes spread over 2^-20 .. 2^20): every gradient element within the bound of the float64 adjoint;
  (C) the value within the summed margins plus the project's 2e-5 for the order of the partial sums;
  (D) TrainLoss end to end (what _LapLoss adds: the split of the output, the incoming gradient, the coefficient order at the
      10 000-iteration switch, a None second prediction), on rand and on near-target inputs;
  (E) the same device results must MISS deliberately wrong references (replicate padding, top-left subsampling, exchanged
      coefficients, a wrong level weight) by at least 10 margins: the margins are tight enough to see such faults.
Margins and their derivation: tests/loss_ref64.py.  Measured figures: profiles/loss_f64.md (printed here with -s)."""
import os
import sys

import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import loss_ref64 as R  # noqa: E402
from oracle import loss_ref  # noqa: E402

pytestmark = pytest.mark.gpu

ALL = list(R.CASES)
G32 = float(torch.tensor(R.G_IN, dtype=torch.float32))
_runs, _rows, _rows_d = {}, {}, []


def _bits(t):
    return t.contiguous().view(torch.int32)


def _forward(a, b, t, ca, cb, levels):
    """(workspace, partial sums) of ebfi_laploss_forward on device images (b may be None)."""
    from ebfi_amd import _native as N
    lib = N.lib()
    B, C, H, W = a.shape
    planes = B * C * (2 if b is not None else 1)
    n_ws = int(lib.ebfi_laploss_workspace_floats(planes, H, W, levels))
    assert n_ws == R.workspace_floats(planes, H, W, levels)
    ws = torch.empty(n_ws, dtype=torch.float32, device=a.device)
    partial = torch.empty(int(lib.ebfi_laploss_partials(planes, H, W, levels)), dtype=torch.float32, device=a.device)
    N.check(lib.ebfi_laploss_forward(N.ptr(a), N.ptr(b) if b is not None else None, N.ptr(t), ca, cb, N.ptr(ws), N.ptr(partial),
                                     B * C, H, W, levels, N.stream_ptr(a.device)), "ebfi_laploss_forward")
    return ws, partial


def _backward(ws, n_images, C, H, W, levels, g=G32):
    """Gradient [n_images, C, H, W] (CPU) of ebfi_laploss_backward on a device workspace, which it consumes."""
    from ebfi_amd import _native as N
    gl = torch.tensor([g], dtype=torch.float32, device=ws.device)
    out = torch.empty((n_images, C, H, W), dtype=torch.float32, device=ws.device)
    N.check(N.lib().ebfi_laploss_backward(N.ptr(gl), N.ptr(ws), N.ptr(out), n_images * C, H, W, levels, N.stream_ptr(ws.device)),
            "ebfi_laploss_backward")
    return out.cpu()


def _run(name):
    """One forward (and a second, for repeatability), the cloned sign field, and the backward on the device's own workspace."""
    if name not in _runs:
        a, b, t, y = R.yardstick(name)
        ca, cb = R.CASES[name]["coefs"]
        ad, bd, td = a.cuda(), (b.cuda() if b is not None else None), t.cuda()
        ws, partial = _forward(ad, bd, td, ca, cb, y.levels)
        field = ws.clone().cpu()
        ws2, partial2 = _forward(ad, bd, td, ca, cb, y.levels)
        again = torch.equal(_bits(ws), _bits(ws2)) and torch.equal(_bits(partial), _bits(partial2))
        grad = _backward(ws, y.n_images, y.C, y.H, y.W, y.levels)
        _runs[name] = dict(field=R.split_levels(field, y.n_images, y.C, y.H, y.W, y.levels), again=again,
                           value=partial.sum().item(), grad=grad)
    return _runs[name]


@pytest.fixture(scope="module", autouse=True)
def table():
    yield
    if _rows:
        print("\n| case | sign mismatches (all ambiguous), worst |lap64| / tau there | ambiguous | (B) err / bound | (B') randn, spread "
              "| value err / allowed |")
        print("|---|---|---|---|---|---|")
        for name, r in _rows.items():
            print("| %s | %s | %s | %s | %s | %s |" % (name, r.get("A", "-"), r.get("amb", "-"), r.get("B", "-"),
                                                      ", ".join(r[k] for k in ("Bp0", "Bp1") if k in r) or "-", r.get("C", "-")))
    if _rows_d:
        print("\n| TrainLoss | inputs | gradient err / allowed | value rel err |\n|---|---|---|---|")
        for row in _rows_d:
            print("| %s | %s | %.3f | %.2e |" % row)


# ------------------------------------------------------------------------------------------------ (A) the sign field
@pytest.mark.parametrize("name", ALL)
def test_sign_field_against_float64(name):
    _, _, _, y = R.yardstick(name)
    run = _run(name)
    want = y.sign_field()
    mism, worst, amb = 0, 0.0, 0
    for l, e in enumerate(run["field"]):
        v = y.v(l).float().expand_as(e)
        assert torch.equal(_bits(e)[y.clear[l]], _bits(want[l])[y.clear[l]]), (name, l)
        assert (e[y.zero[l]] == 0).all(), (name, l)
        assert ((e == v) | (e == -v) | (e == 0)).all(), (name, l)
        # what (A) can infer of the device's error: where its sign is not float64's, it erred by at least |lap64|
        off = (torch.sign(e.double()) != torch.sign(y.lap[l])) & ~y.zero[l]
        assert not (off & ~y.ambiguous[l]).any()
        mism += int(off.sum())
        amb += int(y.ambiguous[l].sum())
        if off.any():
            worst = max(worst, (y.lap[l].abs() / y.tau[l])[off].max().item())
    assert run["again"], "a second forward on the same inputs left other bits"
    _rows.setdefault(name, {}).update(A="%d, %.3f" % (mism, worst), amb="%d" % amb)
    print("%-6s sign field: %d ambiguous elements, %d of them with float64's sign not taken (worst |lap64| / tau %.3f)"
          % (name, amb, mism, worst))


# ------------------------------------------------------------------------------------------------ (B) the adjoint
def _adjoint_check(s_levels, grad, g=G32):
    bound = R.grad_bound(s_levels, g)
    err = (grad.double() - g * R.adjoint64(s_levels)).abs()
    ratio = (err / bound.clamp_min(1e-300))[bound > 0]
    return err, bound, (ratio.max().item() if ratio.numel() else 0.0)


@pytest.mark.parametrize("name", ALL)
def test_adjoint_of_the_devices_own_field(name):
    _, _, _, y = R.yardstick(name)
    run = _run(name)
    err, bound, worst = _adjoint_check(run["field"], run["grad"])
    _rows.setdefault(name, {}).update(B="%.3f" % worst)
    print("%-6s adjoint of the device's field: worst err / bound %.3f (max |grad| %.3g)" % (name, worst, run["grad"].abs().max()))
    assert torch.isfinite(run["grad"]).all()
    assert (err <= bound + 1e-30).all(), (name, worst)
    if name == "patch":
        assert (run["grad"][y.B + 1, 2] == 0).all()


@pytest.mark.parametrize("spread", [False, True], ids=["randn", "spread"])
@pytest.mark.parametrize("name", ["min5", "ragged", "min2", "min3"])
def test_adjoint_of_arbitrary_fields(name, spread):
    _, _, _, y = R.yardstick(name)
    s = R.spread_field([lp.shape for lp in y.lap], 17 + spread, spread)
    grad = _backward(R.join_levels(s).cuda(), y.n_images, y.C, y.H, y.W, y.levels)
    err, bound, worst = _adjoint_check(s, grad)
    _rows.setdefault(name, {}).update({"Bp%d" % spread: "%.3f" % worst})
    print("%-6s adjoint of a %s field: worst err / bound %.3f" % (name, "spread" if spread else "randn", worst))
    assert torch.isfinite(grad).all()
    assert (err <= bound + 1e-30).all(), (name, worst)


# ------------------------------------------------------------------------------------------------ (C) the value
@pytest.mark.parametrize("name", ALL)
def test_value_against_float64(name):
    _, _, _, y = R.yardstick(name)
    got, ref = _run(name)["value"], y.value()
    allowed = y.value_margin() + 2e-5 * ref
    _rows.setdefault(name, {}).update(C="%.2e / %.2e" % (abs(got - ref), allowed))
    print("%-6s value %.9g float64 %.9g: err %.3g, allowed %.3g (margins %.3g)" % (name, got, ref, abs(got - ref), allowed,
                                                                                y.value_margin()))
    assert abs(got - ref) <= allowed


# ------------------------------------------------------------------------------------------------ (D) TrainLoss end to end
CONFIGS = [(2, 64, 64, 0, True, 1), (1, 32, 48, 20000, True, 2), (2, 48, 32, 0, False, 1)]


@pytest.mark.parametrize("kind", ["rand", "near3"])
@pytest.mark.parametrize("B,H,W,it,detail,accu", CONFIGS, ids=["it0", "it20000_accu2", "detail_off"])
def test_train_loss_end_to_end(B, H, W, it, detail, accu, kind):
    from ebfi_amd.loss import TrainLoss
    a, b, t = R.make_inputs(kind, (B, 3, H, W), 100 + H + it % 7)            # a: sharp, b: sharp_pre
    c_sharp, c_pre = (0.1, 1.0) if it < 10e3 else (1.0, 0.1)
    if not detail:
        c_sharp, c_pre = 1.0, 0.0
    preds = [(a, c_sharp), (b, c_pre)] if detail else [(a, c_sharp)]
    ws, _ = _forward(a.cuda(), b.cuda() if detail else None, t.cuda(), c_sharp, c_pre, 5)
    s = R.split_levels(ws.cpu(), B * len(preds), 3, H, W, 5)
    lap = R.adjoint64(s) / accu
    bound = R.grad_bound(s) / accu
    ad, bd = a.cuda().requires_grad_(), b.cuda().requires_grad_()
    out = TrainLoss(detail).cuda()(bd, ad, t.cuda(), iteration=it, accu_step=accu)
    out.backward()
    ref = loss_ref.train_loss(b.double(), a.double(), t.double(), iteration=it, accu_step=accu, detail_enabled=detail).item()
    worst = 0.0
    for i, ((p, coef), dev) in enumerate(zip(preds, (ad, bd))):
        x = p.detach().double().requires_grad_()
        loss_ref.census_loss(x, t.double()).backward()
        census = float(torch.tensor(coef, dtype=torch.float32)) * x.grad / accu
        allowed = bound[i * B:(i + 1) * B] + 5e-5 * census.abs().max()
        err = (dev.grad.cpu().double() - (lap[i * B:(i + 1) * B] + census)).abs()
        worst = max(worst, (err / allowed).max().item())
        assert (err <= allowed).all(), (i, worst)
    if not detail:
        assert bd.grad is None
    print("TrainLoss %s %dx%dx%d it=%d detail=%d accu=%d: worst gradient err / allowed %.3f, value %.9g float64 %.9g (rel %.2e)"
          % (kind, B, H, W, it, detail, accu, worst, out.item(), ref, abs(out.item() - ref) / abs(ref)))
    _rows_d.append(("%dx3x%dx%d it=%d detail=%d accu=%d" % (B, H, W, it, detail, accu), kind, worst, abs(out.item() - ref) / abs(ref)))
    assert abs(out.item() - ref) <= 2e-5 * abs(ref)


# ------------------------------------------------------------------------------------------------ (E) sensitivity
PYRAMIDS = {
    "replicate padding": lambda d, L: R.general_pyramid(d, L, pad="replicate"),
    "top-left subsampling": lambda d, L: R.general_pyramid(d, L, pool="topleft"),
}


@pytest.mark.parametrize("name", ["ragged", "min5"])
def test_wrong_references_are_missed_by_ten_margins(name):
    _, _, _, y = R.yardstick(name)
    run = _run(name)
    swapped = R.plane_coefs(y.coefs[::-1], y.n_images, y.B)
    weights = [2 ** l for l in range(y.levels)]
    weights[2] = 2 ** 3
    fields = {"coef_a and coef_b exchanged": (y.lap, y.sign_field(coef=swapped)),
              "level weight 2^(l+1) at level 2": (y.lap, y.sign_field(weights=weights))}
    for label, pyr in PYRAMIDS.items():
        lap = pyr(y.d, y.levels)
        fields[label + " in the pyramid"] = (lap, y.sign_field(lap))
    for label, (lap, want) in fields.items():
        # (A) with ten times the margin: elements whose wrong reference is that far from zero and whose bits the device misses
        missed, far = 0, 0.0
        for l, e in enumerate(run["field"]):
            sure = lap[l].abs() > 10 * y.tau[l]
            miss = sure & (_bits(e) != _bits(want[l]))
            missed += int(miss.sum())
            if miss.any():
                far = max(far, (lap[l].abs() / y.tau[l])[miss].max().item())
        print("%-6s sign field against %s: %d elements missed beyond 10 tau, the farthest at %.3g tau" % (name, label, missed, far))
        assert missed >= 1 and far >= 10, label
    for label, pyr in PYRAMIDS.items():
        bound = R.grad_bound(run["field"], G32)
        err = (run["grad"].double() - G32 * R.adjoint64(run["field"], pyr)).abs()
        worst = (err / bound).max().item()
        print("%-6s adjoint against %s in the adjoint: missed by %.3g bounds" % (name, label, worst))
        assert worst >= 10, label
