"""Host-side checks of the device reconstruction losses (ebfi_amd.bcloss, csrc/bcloss.hip, loss/reconstruction.py,
myutils/gradients.py): the float64 numpy restatement the GPU tests lean on (tests/bc_ref.py) reproduces the REFERENCE'S OWN
float64 losses and gradients (tests/golden/bc_small.npz, written by tests/golden/make_golden_bc.py with one torch thread); the
fixture's cases exercise what they are for; the header, the binding and the library agree; the shims export the reference's
names; the wrappers refuse what they must.  No compute calls: there is no GPU here."""
import ctypes
import inspect
import os
import re

import numpy as np
import pytest
import torch

from ebfi_amd import _native as N
from ebfi_amd import bcloss as BC  # noqa: F401  (every test here is about this module: without it none may pass)

import bc_ref as R
import iwe_ref as I

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CASES = ("general", "bounds", "pile", "nomask", "empty", "still")
LOSSES = ("gen_loss", "tc_loss", "tv_loss")
GRADS = ("gen_gflow", "gen_gimg", "tc_gflow", "tc_gprev", "tc_gimg", "tv_gimg")


@pytest.fixture(scope="module")
def golden(golden_dir):
    return np.load(os.path.join(golden_dir, "bc_small.npz"))


def case(golden, name):
    v = {k: golden["%s__%s" % (name, k)] for k in ("flow", "img", "prev_img", "cnt", "events", "pol_mask", "avg", "weights")}
    v["res"] = (int(golden[name + "__H"]), int(golden[name + "__W"]))
    return v


def restated(v):
    out = {}
    out["gen_loss"], out["gen_gflow"], out["gen_gimg"] = R.generative(v["flow"], v["img"], v["cnt"], v["avg"], v["res"])
    out["tc_loss"], out["tc_gflow"], out["tc_gprev"], out["tc_gimg"] = R.temporal(v["flow"], v["prev_img"], v["img"], v["res"],
                                                                                  v["weights"][1])
    out["tv_loss"], out["tv_gimg"] = R.total_variation(v["img"], v["weights"][0])
    return out


@pytest.mark.parametrize("name", CASES)
def test_restatement_reproduces_the_float64_reference(golden, name):
    v = case(golden, name)
    keep = {k: np.array(a) for k, a in v.items() if isinstance(a, np.ndarray)}
    out = restated(v)
    for k in LOSSES:
        want = float(golden["%s__%s64" % (name, k)])
        assert abs(float(out[k]) - want) <= 1e-12 * abs(want), k
    for k in GRADS:
        want = golden["%s__%s64" % (name, k)]
        assert out[k].shape == want.shape and want.dtype == np.float64, k
        assert np.abs(out[k] - want).max() <= 1e-12 * max(np.abs(want).max(), 1.0), k
    # the stand-in of the float64 run is the serial float32 AveragedIWE of the masked flow
    assert np.array_equal(v["avg"], I.averaged_iwe(R.masked_flow(v["flow"], v["cnt"]), v["events"], v["pol_mask"], v["res"]))
    for k, a in keep.items():
        assert np.array_equal(v[k], a)


def test_sobel_restatement_against_torch_in_float64():
    rng = np.random.default_rng(3)
    x = rng.uniform(-1, 1, (2, 3, 5, 6))
    t = torch.from_numpy(x).requires_grad_(True)
    gx, gy = R.t_sobel(t)
    ggx, ggy = rng.uniform(-1, 1, gx.shape), rng.uniform(-1, 1, gy.shape)
    ((gx * torch.from_numpy(ggx)).sum() + (gy * torch.from_numpy(ggy)).sum()).backward()
    mine = R.sobel(x.reshape(6, 5, 6))
    assert np.abs(mine[0] - gx.detach().numpy()[:, 0]).max() <= 1e-14 and np.abs(mine[1] - gy.detach().numpy()[:, 0]).max() <= 1e-14
    adj = R.sobel_adjoint(ggx[:, 0], ggy[:, 0])
    assert np.abs(adj - t.grad.numpy().reshape(6, 5, 6)).max() <= 1e-14
    ramp = np.arange(6.0)[None, None, :] * np.ones((1, 5, 1))
    gx, gy = R.sobel(ramp)
    assert np.array_equal(gx[0, :, 1:-1], np.ones((5, 4))) and np.array_equal(gx[0, :, 0], np.full(5, 0.5)) and not gy.any()


def test_torch_restatement_agrees_with_the_closed_form(golden):
    v = case(golden, "general")
    t = lambda a: torch.from_numpy(np.array(a)).double()
    flow, img, prev = (t(v[k]).requires_grad_(True) for k in ("flow", "img", "prev_img"))
    loss = R.t_generative(flow, img, t(v["cnt"]), t(v["avg"]), v["res"]) + R.t_temporal(flow, prev, img, v["res"], v["weights"][1]) \
        + R.t_total_variation(img, v["weights"][0])
    loss.backward()
    out = restated(v)
    assert abs(float(loss.detach()) - (out["gen_loss"] + out["tc_loss"] + out["tv_loss"])) <= 1e-12 * float(loss.detach())
    for got, want in ((flow.grad, out["gen_gflow"] + out["tc_gflow"]), (prev.grad, out["tc_gprev"]),
                      (img.grad, out["gen_gimg"] + out["tc_gimg"] + out["tv_gimg"])):
        assert np.abs(got.numpy() - want).max() <= 1e-12 * np.abs(want).max()


def test_fixture_cases_exercise_what_they_are_for(golden):
    assert 0 < float(golden["dev_loss"]) < 1e-6 and 0 < float(golden["dev_grad"]) < 1e-4
    assert os.path.getsize(os.path.join(ROOT, "tests", "golden", "bc_small.npz")) < 300 * 1024
    for name in CASES:
        v = case(golden, name)
        H, W = v["res"]
        assert H % 2 == 0 and W % 2 == 0
        assert not R.kinks(v["flow"], v["cnt"], v["prev_img"], v["img"], v["res"]).any(), name
        for k in ("flow", "img", "prev_img", "cnt", "events", "pol_mask", "avg"):
            assert v[k].dtype == np.float32, (name, k)
    v = case(golden, "general")
    assert v["flow"].shape == (2, 2, 12, 20) and v["events"].shape == (2, 600, 4) and np.abs(v["flow"]).max() <= 0.15
    assert np.abs(v["flow"]).max() * 20 > 2.5                              # three-pixel shifts
    ev = v["events"]
    cnt = np.zeros_like(v["cnt"])
    for b in range(2):
        for _, y, x, p in ev[b]:
            cnt[b, 0 if p > 0 else 1, int(y), int(x)] += 1
    assert np.array_equal(cnt, v["cnt"])                                   # inp_cnt consistent with the list
    # bounds: samples outside by less and by more than a pixel; partially and fully padded corners
    v = case(golden, "bounds")
    H, W = v["res"]
    ix, iy = R.coordinates(R.masked_flow(v["flow"], v["cnt"]), v["res"])
    out = np.maximum(np.maximum(-ix, ix - (W - 1)), np.maximum(-iy, iy - (H - 1)))
    assert ((out > 0) & (out < 1)).any() and (out > 1).any() and (out > 2).any()
    inside = [((np.floor(iy) + (c >> 1) >= 0) & (np.floor(iy) + (c >> 1) < H) & (np.floor(ix) + (c & 1) >= 0) & (np.floor(ix) + (c & 1) < W))
              for c in range(4)]
    n_in = sum(a.astype(int) for a in inside)
    assert set(np.unique(n_in)) >= {0, 1, 2, 4}
    # pile: every sample of both terms in one 2 x 2 footprint
    v = case(golden, "pile")
    for f in (v["flow"], R.masked_flow(v["flow"], v["cnt"])):
        ix, iy = R.coordinates(f, v["res"])
        assert (np.floor(ix) == 4).all() and (np.floor(iy) == 3).all()
    # nomask: half the pixels masked, events on some of them anyway; they take part in the temporal term
    v = case(golden, "nomask")
    masked = v["cnt"].sum(axis=1) == 0
    assert masked.mean() == 0.5
    ev = v["events"]
    assert any(masked[b, int(y), int(x)] for b in range(ev.shape[0]) for _, y, x, _ in ev[b])
    assert not golden["nomask__gen_gflow64"].transpose(1, 0, 2, 3)[:, masked].any()
    assert not golden["nomask__gen_gflow32"].transpose(1, 0, 2, 3)[:, masked].any()
    assert (golden["nomask__tc_gflow64"].transpose(1, 0, 2, 3)[:, masked] != 0).any()
    assert (golden["nomask__gen_gflow64"].transpose(1, 0, 2, 3)[:, ~masked] != 0).any()
    v = case(golden, "empty")
    assert v["events"].shape[1] == 0 and not v["avg"].any() and float(golden["empty__gen_loss64"]) > 0
    v = case(golden, "still")
    assert not v["flow"].any() and v["avg"].any()


def test_the_order_of_addition_is_exercised(golden):
    """Adding a destination's float32 addends in the reversed order must change bits, or the cases say nothing about order."""
    for name in ("pile", "general"):
        v = case(golden, name)
        ix, iy = R.coordinates(v["flow"], v["res"])
        g = -(v["weights"][1] * np.sign(v["img"][:, 0].astype(np.float64) - R.sample(v["prev_img"][:, 0], ix, iy)[0]))
        B, H, W = g.shape
        x0, y0 = np.floor(ix).astype(int), np.floor(iy).astype(int)
        tx, ty = ix - x0, iy - y0
        fwd, rev = np.zeros((B, H, W), np.float32), np.zeros((B, H, W), np.float32)
        entries = []
        for b in range(B):
            for h in range(H):
                for w in range(W):
                    for c in range(4):
                        y, x = y0[b, h, w] + (c >> 1), x0[b, h, w] + (c & 1)
                        if 0 <= y < H and 0 <= x < W:
                            wt = (tx[b, h, w] if c & 1 else 1 - tx[b, h, w]) * (ty[b, h, w] if c >> 1 else 1 - ty[b, h, w])
                            entries.append((b, y, x, np.float32(g[b, h, w] * wt)))
        for b, y, x, a in entries:
            fwd[b, y, x] = fwd[b, y, x] + a
        for b, y, x, a in reversed(entries):
            rev[b, y, x] = rev[b, y, x] + a
        assert not np.array_equal(fwd, rev), name
        want = golden[name + "__tc_gprev64"][:, 0]
        assert np.abs(fwd - want).max() <= 8 * float(golden["dev_grad"]) * np.abs(want).max()


# ------------------------------------------------------------------ the ABI
NEW = {"ebfi_bc_workspace", "ebfi_bc_forward_workspace", "ebfi_sobel_forward", "ebfi_sobel_backward", "ebfi_bc_mask_flow",
       "ebfi_bc_generative_forward", "ebfi_bc_generative_backward", "ebfi_bc_temporal_forward", "ebfi_bc_temporal_backward",
       "ebfi_bc_tv_forward", "ebfi_bc_tv_backward"}


@pytest.fixture(scope="module")
def lib():
    if not os.path.exists(N.LIB_PATH):
        N.build()
    return N.lib()


def test_new_symbols_are_declared_bound_and_exported(lib):
    assert NEW <= set(N.declared_symbols()) and NEW <= set(N.SIGNATURES)
    h = ctypes.CDLL(N.LIB_PATH)
    for name in NEW:
        assert hasattr(h, name), name
    header = open(os.path.join(ROOT, "include", "ebfi_hip.h")).read()
    assert "#define EBFI_ABI_VERSION 14" in header and lib.ebfi_abi_version() == 14 == N.ABI_VERSION      # a pure addition
    assert "ebfi_bc_* / ebfi_sobel_*" in header                                                          # the index comment
    _i, _i64, _vp, _f, _d = ctypes.c_int, ctypes.c_int64, ctypes.c_void_p, ctypes.c_float, ctypes.c_double
    flow = [_vp] + [_i64] * 4
    assert N.SIGNATURES["ebfi_bc_workspace"] == (_i64, [_i64, _i, _i]) == N.SIGNATURES["ebfi_bc_forward_workspace"]
    assert N.SIGNATURES["ebfi_sobel_forward"] == (_i, [_vp, _i64, _i, _i, _vp, _vp, _vp])
    assert N.SIGNATURES["ebfi_sobel_backward"] == (_i, [_vp, _vp, _i64, _i, _i, _vp, _vp])
    assert N.SIGNATURES["ebfi_bc_generative_forward"] == (_i, flow + [_vp, _vp, _i, _vp, _i64, _i, _i, _f, _vp, _vp, _vp, _i64, _vp])
    assert N.SIGNATURES["ebfi_bc_temporal_backward"] == (_i, flow + [_vp, _vp, _i64, _i, _i, _f, _d, _vp, _vp, _vp, _vp, _vp, _i64, _vp])
    assert N.SIGNATURES["ebfi_bc_tv_forward"] == (_i, [_vp, _i64, _i, _i, _d, _vp, _vp, _i64, _vp])


def test_workspace_arithmetic(lib):
    ws, fw = lib.ebfi_bc_workspace, lib.ebfi_bc_forward_workspace
    a = ws(2, 12, 20)
    assert a > 0 and a % 256 == 0 and 0 < fw(2, 12, 20) < a and fw(2, 12, 20) % 256 == 0
    assert a >= 2 * 12 * 20 * (4 * 4 * 4 + 4 * 8 + 8)                      # keys and positions twice, two planes of addends, two images
    assert ws(3, 12, 20) > a and ws(2, 13, 20) > a and ws(2, 12, 21) > a   # monotone in B, H and W
    last = 0
    for B, H, W in ((1, 2, 2), (1, 2, 3), (1, 3, 3), (2, 3, 3), (2, 64, 64), (2, 64, 65), (3, 64, 65), (8, 256, 256), (8, 256, 257)):
        now = ws(B, H, W)
        assert now >= last and fw(B, H, W) <= now, (B, H, W)               # (tiny sizes share their 256-byte blocks)
        assert now > last or B * H * W < 64, (B, H, W)
        last = now
    assert fw(1, 1024, 1024) > fw(1, 16, 16)
    for bad in ((0, 4, 4), (-1, 4, 4), (1, 1, 4), (1, 4, 1), (1, 0, 4), (1, 4, -3), (1, 1 << 16, 1 << 16), (2, 1 << 16, 1 << 15),
                (1, (1 << 16) + 1, (1 << 16) - 1)):
        assert ws(*bad) == 0 and fw(*bad) == 0, bad
    # the sort's entry positions are 32-bit: 4 * B * H * W < 2**32; the partial sums alone (Sobel and the total variation sort
    # nothing) go up to B * H * W < 2**32 - 1
    for big in ((1, 1 << 15, 1 << 15), (4, 1 << 14, 1 << 14), (1, (1 << 16) - 1, 1 << 16)):
        assert ws(*big) == 0 and fw(*big) > 0, big
    assert ws(1, 1 << 15, (1 << 15) - 1) > 0                               # 4 * B * H * W just under 2**32


def test_argument_errors_do_not_touch_the_gpu(lib):
    p = ctypes.c_void_p(256)               # never dereferenced: every call below is refused before a launch
    odd = ctypes.c_void_p(264)
    big = 1 << 40
    flow = (p, 32, 16, 4, 1)
    sf, sb = lib.ebfi_sobel_forward, lib.ebfi_sobel_backward
    assert sf(None, 1, 4, 4, p, p, None) == -1 and b"null" in lib.ebfi_last_error()
    assert sf(p, 1, 4, 4, p, None, None) == -1
    assert sf(p, 0, 4, 4, p, p, None) == -1 and sf(p, 1, 1, 4, p, p, None) == -1 and sf(p, 1, 4, 1, p, p, None) == -1
    assert sf(p, 1, 1 << 16, 1 << 16, p, p, None) == N.EBFI_ERR_UNSUPPORTED and b"2^32 - 1" in lib.ebfi_last_error()
    assert sb(p, p, 2, 1 << 16, 1 << 15, p, None) == N.EBFI_ERR_UNSUPPORTED
    assert sb(None, None, 1, 4, 4, p, None) == -1 and sb(p, p, 1, 4, 4, None, None) == -1 and sb(p, p, 1, 4, 1, p, None) == -1
    mf = lib.ebfi_bc_mask_flow
    assert mf(*flow, None, 2, 1, 4, 4, p, None) == -1 and mf(*flow, p, 0, 1, 4, 4, p, None) == -1 and mf(*flow, p, 2, 1, 4, 4, None, None) == -1
    assert mf(None, 32, 16, 4, 1, p, 2, 1, 4, 4, p, None) == -1 and mf(*flow, p, 2, 1, 1, 4, p, None) == -1
    gf = lib.ebfi_bc_generative_forward
    assert gf(*flow, None, p, 2, p, 1, 4, 4, 4.0, p, p, p, big, None) == -1
    assert gf(*flow, p, p, 2, None, 1, 4, 4, 4.0, p, p, p, big, None) == -1
    assert gf(*flow, p, p, 0, p, 1, 4, 4, 4.0, p, p, p, big, None) == -1 and b"channel" in lib.ebfi_last_error()
    assert gf(*flow, p, p, 2, p, 1, 4, 1, 4.0, p, p, p, big, None) == -1
    assert gf(*flow, p, p, 2, p, 1, 4, 4, 4.0, p, p, None, 0, None) == -4
    assert gf(*flow, p, p, 2, p, 1, 4, 4, 4.0, p, p, p, 8, None) == -4
    assert gf(*flow, p, p, 2, p, 1, 4, 4, 4.0, p, p, odd, big, None) == -1 and b"aligned" in lib.ebfi_last_error()
    assert gf(*flow, p, p, 2, p, 1, 1 << 15, 1 << 15, 4.0, p, p, p, big, None) == N.EBFI_ERR_UNSUPPORTED
    gb = lib.ebfi_bc_generative_backward
    assert gb(*flow, p, p, 2, None, 1, 4, 4, 4.0, p, p, p, p, big, None) == -1
    assert gb(*flow, p, p, 2, p, 1, 4, 4, 4.0, None, p, p, p, big, None) == -1
    assert gb(*flow, p, p, 2, p, 1, 4, 4, 4.0, p, None, None, p, big, None) == -1
    assert gb(*flow, p, p, 2, p, 1, 4, 4, 4.0, p, p, p, p, lib.ebfi_bc_workspace(1, 4, 4) - 1, None) == -4
    assert gb(*flow, p, p, 2, p, 1, 4, 4, 4.0, p, p, p, odd, big, None) == -1
    tf = lib.ebfi_bc_temporal_forward
    assert tf(*flow, None, p, 1, 4, 4, 4.0, 0.5, p, p, p, big, None) == -1
    assert tf(*flow, p, p, 1, 4, 4, 4.0, 0.5, p, None, p, big, None) == -1
    assert tf(*flow, p, p, 0, 4, 4, 4.0, 0.5, p, p, p, big, None) == -1
    assert tf(*flow, p, p, 1, 4, 4, 4.0, 0.5, p, p, p, 0, None) == -4
    tb = lib.ebfi_bc_temporal_backward
    assert tb(*flow, p, None, 1, 4, 4, 4.0, 0.5, p, p, p, p, p, big, None) == -1
    assert tb(*flow, p, p, 1, 4, 4, 4.0, 0.5, p, None, None, None, p, big, None) == -1
    assert tb(*flow, p, p, 1, 4, 4, 4.0, 0.5, p, p, p, p, p, lib.ebfi_bc_forward_workspace(1, 4, 4), None) == -4      # grad_prev sorts
    assert tb(*flow, p, p, 1, 4, 4, 4.0, 0.5, p, p, p, p, None, 0, None) == -4
    tvf, tvb = lib.ebfi_bc_tv_forward, lib.ebfi_bc_tv_backward
    assert tvf(None, 1, 4, 4, 0.1, p, p, big, None) == -1 and tvf(p, 1, 4, 4, 0.1, None, p, big, None) == -1
    assert tvf(p, 1, 4, 4, 0.1, p, p, 0, None) == -4 and tvf(p, 1, 4, 4, 0.1, p, odd, big, None) == -1
    assert tvf(p, 1, 1 << 16, 1 << 16, 0.1, p, p, big, None) == N.EBFI_ERR_UNSUPPORTED
    assert tvb(p, 1, 1 << 16, 1 << 16, 0.1, p, p, None) == N.EBFI_ERR_UNSUPPORTED
    assert lib.ebfi_bc_temporal_forward(*flow, p, p, 1, 1 << 15, 1 << 15, 4.0, 0.5, p, p, p, big, None) == N.EBFI_ERR_UNSUPPORTED
    assert mf(*flow, p, 2, 1, 1 << 15, 1 << 15, p, None) == N.EBFI_ERR_UNSUPPORTED and b"4 * B * H * W" in lib.ebfi_last_error()
    assert tvb(p, 1, 4, 4, 0.1, None, p, None) == -1 and tvb(p, 1, 4, 4, 0.1, p, None, None) == -1 and tvb(p, 1, 1, 4, 0.1, p, p, None) == -1


def test_the_library_puts_a_single_chain_on_the_callers_stream():
    """One chain of launches on the stream it is handed, nothing else: no stream or event of its own, no synchronisation, no
    copy, no allocation, and no float atomic (the only atomic is the integer histogram of the sort); every entry point
    validates before its first launch; a forward is the pixel kernel and the final reduction."""
    src = open(os.path.join(ROOT, "ebfi-be_amd", "csrc", "bcloss.hip")).read()
    for word in ("hipStreamCreate", "hipEventRecord", "hipStreamWaitEvent", "hipDeviceSynchronize", "hipStreamSynchronize",
                 "hipMemcpy", "hipMemset", "hipMalloc", "hipLaunchCooperativeKernel", "unsafeAtomicAdd", "atomicAdd_system"):
        assert word not in src, word
    atomics = re.findall(r"atomic\w*\(([^;]*);", src)
    assert len(atomics) == 1 and atomics[0].startswith("&h[")             # uint32 LDS bins
    assert "#pragma clang fp contract(off)" in src
    assert src.count("hipLaunchKernelGGL(") == 1 and "hipLaunchKernelGGL(kern, grid, dim3(kBlock), 0, st, __VA_ARGS__)" in src
    bodies = re.findall(r'extern "C" int (ebfi_\w+)\((?:[^{]*)\{(.*?)\n\}', src, flags=re.S)
    assert {name for name, _ in bodies} == NEW - {"ebfi_bc_workspace", "ebfi_bc_forward_workspace"}
    for name, body in bodies:
        first = min(body.index("BC_LAUNCH("), body.index("ordered_scatter(") if "ordered_scatter(" in body else len(body))
        for word in ("fail(EBFI_ERR_ARG", "sizes_ok("):
            assert word in body[:first], (name, word)
        assert "fail(" not in body[first:] and "workspace_ok(" not in body[first:], name
        if name.endswith("_forward") and name != "ebfi_sobel_forward":
            assert body.count("BC_LAUNCH(") == 2 and "bc_loss_final" in body, name      # the pixel kernel and the final reduction


# ------------------------------------------------------------------ the Python surface
def test_shims_export_the_reference_names(golden_dir):
    rows = [line.split() for line in open(os.path.join(golden_dir, "reconstruction_names.txt")).read().splitlines() if line.strip()]
    assert rows == [["loss", "BrightnessConstancy"], ["myutils.gradients", "Sobel"]]
    for module, star in (("loss", "from loss import *"), ("myutils.gradients", "from myutils.gradients import *")):
        ns = {}
        exec(star, ns)
        for mod, name in rows:
            if mod == module:
                assert name in ns, (module, name)
    ns = {}
    exec("from loss import BrightnessConstancy, EventWarping, AveragedIWE\nfrom myutils.gradients import Sobel", ns)
    import loss.reconstruction
    import myutils.gradients
    from ebfi_amd import iwe
    assert ns["BrightnessConstancy"] is BC.BrightnessConstancy is loss.reconstruction.BrightnessConstancy
    assert ns["Sobel"] is BC.Sobel is myutils.gradients.Sobel and ns["AveragedIWE"] is iwe.AveragedIWE
    assert loss.reconstruction.__all__ == ["BrightnessConstancy"] and myutils.gradients.__all__ == ["Sobel"]
    params = lambda f: list(inspect.signature(f).parameters)
    assert params(BC.Sobel.__init__) == ["self", "device"] and params(BC.Sobel.forward) == ["self", "x"]
    assert params(BC.BrightnessConstancy.__init__) == ["self", "config", "device"]
    assert params(BC.BrightnessConstancy.generative_model) == ["self", "flow", "img", "inputs"]
    assert params(BC.BrightnessConstancy.temporal_consistency) == ["self", "flow", "prev_img", "img"]
    assert params(BC.BrightnessConstancy.regularization) == ["self", "img"]
    config = {"loss": {"reconstruction_regul_weight": [0.1, 0.5]}, "loader": {"resolution": [4, 6], "batch_size": 2}}
    bc = BC.BrightnessConstancy(config, "cpu")
    assert (bc.res, bc.flow_scaling, bc.weights) == ([4, 6], 6, [0.1, 0.5])
    assert isinstance(bc.sobel, BC.Sobel) and isinstance(bc.averaged_iwe, iwe.AveragedIWE) and bc.averaged_iwe.batch_size == 2
    assert bc.indices.dtype == torch.float32 and tuple(bc.indices.shape) == (1, 2, 4, 6)
    assert torch.equal(bc.indices[0, 0], torch.arange(4.0)[:, None].expand(4, 6))      # rows, then columns
    assert torch.equal(bc.indices[0, 1], torch.arange(6.0)[None, :].expand(4, 6))
    assert bc.sobel.a.flatten().tolist() == [-1, 0, 1, -2, 0, 2, -1, 0, 1] and tuple(bc.sobel.a.shape) == (1, 1, 3, 3)
    assert bc.sobel.b.flatten().tolist() == [-1, -2, -1, 0, 0, 0, 1, 2, 1] and bc.sobel.b.dtype == torch.float32
    assert isinstance(bc.sobel.pad, torch.nn.ReplicationPad2d)
    for doc in (open(os.path.join(ROOT, "README.md")).read(), open(os.path.join(ROOT, "ebfi-be_amd", "ebfi_amd", "iwe.py")).read()):
        assert "ot provided" not in doc.replace("\n", " ")


def test_the_wrappers_refuse_what_they_cannot_run():
    from unittest import mock
    config = {"loss": {"reconstruction_regul_weight": [0.1, 0.5]}, "loader": {"resolution": [4, 4], "batch_size": 1}}
    bc = BC.BrightnessConstancy(config, "cpu")
    z = lambda *s, **k: torch.zeros(*s, **k)
    t = dict(flow=z(1, 2, 4, 4), img=z(1, 1, 4, 4), prev=z(1, 1, 4, 4), cnt=z(1, 2, 4, 4), ev=z(1, 5, 4), pm=z(1, 5, 2))
    inputs = lambda a: {"inp_cnt": a["cnt"], "inp_list": a["ev"], "inp_pol_mask": a["pm"]}
    calls = {
        "generative_model": (lambda a: bc.generative_model(a["flow"], a["img"], inputs(a)), ("flow", "img", "cnt", "ev", "pm")),
        "temporal_consistency": (lambda a: bc.temporal_consistency(a["flow"], a["prev"], a["img"]), ("flow", "prev", "img")),
        "regularization": (lambda a: bc.regularization(a["img"]), ("img",)),
        "Sobel": (lambda a: BC.Sobel("cpu")(a["img"]), ("img",)),
    }
    for name, (call, used) in calls.items():
        with pytest.raises(NotImplementedError):                          # CPU tensors
            call(t)
        for which in used:
            with pytest.raises(TypeError) as e:                           # float64
                call(dict(t, **{which: t[which].double()}))
            assert "float32" in str(e.value), (name, which)
    with pytest.raises(TypeError):
        bc.regularization([[0.0]])
    with pytest.raises(TypeError):
        bc.generative_model(t["flow"], t["img"], {"inp_cnt": None, "inp_list": t["ev"], "inp_pol_mask": t["pm"]})
    # the rest is decided after the device check: meta tensors stand in for GPU tensors, nothing is dereferenced
    m = lambda *s: torch.zeros(*s, device="meta")
    g = dict(flow=m(1, 2, 4, 4), img=m(1, 1, 4, 4), prev=m(1, 1, 4, 4), cnt=m(1, 2, 4, 4), ev=m(1, 5, 4), pm=m(1, 5, 2))
    with mock.patch.object(N, "require_gpu", lambda *a: None):
        with pytest.raises(ValueError) as e:
            bc.temporal_consistency(g["flow"], t["prev"], g["img"])
        assert "different devices" in str(e.value) and "temporal_consistency" in str(e.value)
        for name, (call, used) in calls.items():
            if name in ("regularization", "Sobel"):
                continue
            for shape in ((1, 2, 4, 5), (1, 3, 4, 4), (2, 4, 4)):         # a flow of another size
                with pytest.raises(ValueError) as e:
                    call(dict(g, flow=m(*shape)))
                assert "flow" in str(e.value) and name in str(e.value)
            with pytest.raises(ValueError) as e:                          # C != 1
                call(dict(g, img=m(1, 2, 4, 4)))
            assert "img" in str(e.value) and "one channel" in str(e.value)
        with pytest.raises(ValueError) as e:
            bc.temporal_consistency(g["flow"], m(1, 3, 4, 4), g["img"])
        assert "prev_img" in str(e.value)
        with pytest.raises(ValueError) as e:
            bc.generative_model(g["flow"], g["img"], inputs(dict(g, cnt=m(1, 2, 4, 5))))
        assert "inp_cnt" in str(e.value)
        with pytest.raises(ValueError) as e:
            bc.regularization(m(4, 4))
        assert "img" in str(e.value)
        for H, W in ((1, 4), (4, 1)):                                     # the law divides by n - 1
            small = BC.BrightnessConstancy(dict(config, loader={"resolution": [H, W], "batch_size": 1}), "cpu")
            for call in (lambda: small.temporal_consistency(m(1, 2, H, W), m(1, 1, H, W), m(1, 1, H, W)),
                         lambda: small.generative_model(m(1, 2, H, W), m(1, 1, H, W), inputs(dict(g, cnt=m(1, 2, H, W)))),
                         lambda: small.regularization(m(1, 1, H, W)), lambda: BC.Sobel("cpu")(m(1, 1, H, W))):
                with pytest.raises(ValueError) as e:
                    call()
                assert "at least 2" in str(e.value)
        with mock.patch.object(N, "lib", side_effect=AssertionError("device work before a refusal")):
            # what AveragedIWE refuses is refused before the masked flow is launched
            for bad, word in ((dict(g, ev=m(1, 5, 3)), "event_list"), (dict(g, ev=m(2, 5, 4)), "inp_list"), (dict(g, pm=m(1, 5, 1)), "inp_pol_mask"),
                              (dict(g, pm=m(1, 4, 2)), "inp_pol_mask"), (dict(g, ev=m(1, 1 << 30, 4), pm=m(1, 1 << 30, 2)), "2**32")):
                with pytest.raises(ValueError) as e:
                    bc.generative_model(bad["flow"], bad["img"], inputs(bad))
                assert word in str(e.value) and "generative_model" in str(e.value), word
            two = BC.BrightnessConstancy(dict(config, loader={"resolution": [4, 4], "batch_size": 2}), "cpu")
            with pytest.raises(ValueError) as e:
                two.generative_model(g["flow"], g["img"], inputs(g))
            assert "batch_size" in str(e.value)
            mid = BC.BrightnessConstancy(config, "cpu")
            mid.res = [1 << 15, 1 << 15]                                  # sorted entries would not fit, the pixels do
            with pytest.raises(ValueError) as e:
                mid.temporal_consistency(m(1, 2, 1 << 15, 1 << 15), m(1, 1, 1 << 15, 1 << 15), m(1, 1, 1 << 15, 1 << 15))
            assert "4 * B * H * W" in str(e.value)
        huge = BC.BrightnessConstancy(config, "cpu")
        huge.res = [1 << 16, 1 << 16]                                     # (set afterwards: the constructor builds an index image)
        for call in (lambda: huge.temporal_consistency(m(1, 2, 1 << 16, 1 << 16), m(1, 1, 1 << 16, 1 << 16), m(1, 1, 1 << 16, 1 << 16)),
                     lambda: huge.regularization(m(1, 1, 1 << 16, 1 << 16)), lambda: BC.Sobel("cpu")(m(1, 1, 1 << 16, 1 << 16))):
            with pytest.raises(ValueError) as e:
                call()
            assert "2**32 - 1" in str(e.value)
