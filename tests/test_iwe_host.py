"""Host-side checks of the device warping losses (ebfi_amd.iwe, csrc/iwe.hip, loss/flow.py, myutils/iwe.py): the numpy
restatement the GPU tests lean on (tests/iwe_ref.py) reproduces the REFERENCE'S OWN outputs (tests/golden/iwe_small.npz,
written by tests/golden/make_golden_iwe.py with one torch thread) bit for bit; its torch form reproduces the stored float64
loss and gradient; the fixture's cases exercise what they are for; the header, the binding and the library agree; the shims
export the reference's names; the wrappers refuse what they must.  No compute calls: there is no GPU here."""
import ctypes
import os
import re

import numpy as np
import pytest
import torch

from ebfi_amd import _native as N
from ebfi_amd import iwe as I  # noqa: F401  (every test here is about this module: without it none may pass)

import iwe_ref as R

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CASES = ("general", "pile", "bounds", "ties", "empty", "padding", "average")
TOLERANCE_CASES = ("general", "pile", "bounds", "padding")
F = np.float32


@pytest.fixture(scope="module")
def golden(golden_dir):
    return np.load(os.path.join(golden_dir, "iwe_small.npz"))


def case(golden, name):
    v = {k: golden["%s__%s" % (name, k)] for k in ("events", "pol_mask", "flows")}
    v.update(res=(int(golden[name + "__H"]), int(golden[name + "__W"])), weight=float(golden[name + "__weight"]))
    v["flow_ev"] = R.event_flow(v["flows"][0], v["events"], v["res"])      # the first flow at every event's source pixel
    return v


def same_bits(a, b):
    """Equal values with equal signs of zero apart: the reference stores -0.0 for a purged negative index, which is index 0."""
    return a.dtype == b.dtype and a.shape == b.shape and np.array_equal(a, b)


@pytest.mark.parametrize("name", CASES)
def test_restatement_reproduces_the_reference(golden, name):
    v = case(golden, name)
    ev, pm, flow, fe, res = v["events"], v["pol_mask"], v["flows"][0], v["flow_ev"], v["res"]
    keep = {k: np.array(a) for k, a in v.items() if isinstance(a, np.ndarray)}
    g = lambda k: golden["%s__%s" % (name, k)]
    at = (ev[:, :, 1] * res[1] + ev[:, :, 2]).astype(np.int64)             # the gather, by hand
    for b in range(ev.shape[0]):
        assert np.array_equal(fe[b, :, 0], flow[b, 1].reshape(-1)[at[b]]) and np.array_equal(fe[b, :, 1], flow[b, 0].reshape(-1)[at[b]])
    for branch, rnd in (("bil", False), ("rnd", True)):
        for tref in (1, 0):
            idx, w = R.get_interpolation(ev, fe, tref, res, max(res), rnd)
            assert same_bits(idx, g("gi_%s_t%d_idx" % (branch, tref))), (branch, tref)
            assert same_bits(w, g("gi_%s_t%d_w" % (branch, tref))), (branch, tref)
    idx, w = R.get_interpolation(ev, fe, 1, res, max(res))
    pm4 = np.concatenate([pm] * 4, axis=1)
    assert same_bits(R.interpolate(idx, w, res, pm4[:, :, 0:1]), g("interp"))
    assert same_bits(R.interpolate(idx, w, res), g("interp_plain"))
    assert same_bits(R.deblur_events(flow, ev, res, max(res)), g("deblur"))
    for key, rnd in (("pol_rnd", True), ("pol_bil", False)):
        assert same_bits(R.compute_pol_iwe(flow, ev, res, pm[:, :, 0:1], pm[:, :, 1:2], max(res), rnd), g(key)), key
    assert same_bits(R.averaged_iwe(flow, ev, pm, res), g("avg"))
    for k, a in keep.items():
        assert np.array_equal(v[k], a)


def bars(golden):
    """8 times the float32 reference's own deviation from the float64 reference, floor 4 float32 ulps (relative)."""
    floor = 4 * 2.0 ** -23
    return max(8 * float(golden["dev_loss"]), floor), max(8 * float(golden["dev_grad"]), floor)


@pytest.mark.parametrize("name", CASES)
def test_torch_restatement_reproduces_the_float64_reference(golden, name):
    v = case(golden, name)
    t = lambda a: torch.from_numpy(np.array(a)).double()
    leaves = [t(f).requires_grad_(True) for f in v["flows"]]
    loss = R.t_event_warping(leaves, t(v["events"]), t(v["pol_mask"]), v["res"], v["weight"])
    loss.backward()
    want = float(golden[name + "__loss64"])
    assert abs(float(loss.detach()) - want) <= 1e-12 * abs(want)
    for leaf, g64 in zip(leaves, golden[name + "__grad64"]):
        assert np.abs(leaf.grad.numpy() - g64).max() <= 1e-12 * max(np.abs(g64).max(), 1.0)
    avg = R.t_averaged_iwe(t(v["flows"][0]).float(), t(v["events"]).float(), t(v["pol_mask"]).float(), v["res"])
    assert np.array_equal(avg.numpy(), golden[name + "__avg"])
    # the serial float32 images with float64 squares and sums (the kernels' recipe) meet the bar the GPU test applies
    mine = sum(R.warping_loss(f, v["events"], v["pol_mask"], v["res"], v["weight"]) for f in v["flows"])
    assert abs(mine - want) <= bars(golden)[0] * abs(want)


def test_fixture_cases_exercise_what_they_are_for(golden):
    assert 0 < float(golden["dev_loss"]) < 1e-6 and 0 < float(golden["dev_grad"]) < 1e-3
    for name in TOLERANCE_CASES:
        v = case(golden, name)
        assert not R.near_integer(v["flows"], v["events"], v["pol_mask"], v["res"]).any(), name
    v = case(golden, "general")
    assert v["events"].shape == (2, 600, 4) and v["res"] == (12, 20) and len(v["flows"]) == 2
    assert np.abs(v["flows"]).max() <= 0.15
    w = golden["general__gi_bil_t1_w"]
    assert 0.03 < (w == 0).mean() < 0.3                                   # some warps leave the image
    # pile: 300 events of one source pixel, every one of them into one 2 x 2 footprint per direction
    v = case(golden, "pile")
    ev = v["events"][0]
    pile = (ev[:, 1] == 3) & (ev[:, 2] == 4)
    assert pile.sum() >= 300
    for tref in (1, 0):
        idx = golden["pile__gi_bil_t%d_idx" % tref][0, :, 0].reshape(4, -1)[:, pile]
        assert all(len(set(row.tolist())) == 1 for row in idx) and len(set(idx[:, 0].tolist())) == 4
    # bounds: 4 N straddles the sort workgroups; pixel 0 and the last pixel of every item, first and last in the list
    v = case(golden, "bounds")
    ev, (H, W) = v["events"], v["res"]
    assert ev.shape[:2] == (3, 257) and (4 * 257) % 256 != 0
    assert (ev[:, 0, 1:3] == 0).all() and (ev[:, -1, 1] == H - 1).all() and (ev[:, -1, 2] == W - 1).all()
    assert (golden["bounds__gi_bil_t1_w"][1, :, 0].reshape(4, -1)[:, [0, -1]] == 0).any()      # item 1 loses corners outwards
    v = case(golden, "ties")
    assert not v["flows"].any() and (v["events"][0, :, 0] == 0).any() and (v["events"][0, :, 0] == 1).any()
    assert np.abs(golden["ties__grad32"]).max() > 0                       # half the gradient through the tied max
    v = case(golden, "empty")
    assert v["events"].shape == (2, 0, 4) and not golden["empty__avg"].any() and float(golden["empty__loss32"]) > 0
    v = case(golden, "padding")
    dead = v["pol_mask"].sum(axis=2) == 0
    assert dead.sum() == 75 and not v["events"][dead].any()
    avg, pol = golden["average__avg"][0], golden["average__pol_rnd"][0]
    assert pol[0, 2, 1] == 3 and avg[0, 2, 1] == 1.5                      # three events from two sources
    assert pol[1, 2, 1] == 1 and avg[1, 2, 1] == 1
    assert pol[0, 4, 2] == 3 and avg[0, 4, 2] == 1.5 and pol[0, 3, 2] == 0      # 3.5 rounds to 4, 2.5 to 2
    assert pol[0].sum() == 7 and pol[1].sum() == 1                        # the two events that leave the image are gone


@pytest.mark.parametrize("name", ["pile", "general"])
def test_the_order_of_addition_is_exercised(golden, name):
    """Feeding every pixel its addends in the reversed order must change output bits, or the fixture says nothing about order."""
    v = case(golden, name)
    idx, w = R.get_interpolation(v["events"], v["flow_ev"], 1, v["res"], max(v["res"]))
    fwd = R.interpolate(idx, w, v["res"])
    assert np.array_equal(fwd, golden[name + "__interp_plain"])
    assert not np.array_equal(R.interpolate(idx, w, v["res"], reverse=True), fwd)
    img = R.warping_images(v["flows"][0], v["events"], v["pol_mask"], v["res"])
    rev = R.warping_images(v["flows"][0], v["events"], v["pol_mask"], v["res"], reverse=True)
    assert not np.array_equal(img[:, :, 2:], rev[:, :, 2:])               # the stamp-weighted sums of both directions


# ------------------------------------------------------------------ the ABI
NEW = {"ebfi_iwe_workspace", "ebfi_iwe_index_bytes", "ebfi_iwe_get_interpolation", "ebfi_iwe_interpolate", "ebfi_iwe_deblur", "ebfi_iwe_source_index",
       "ebfi_iwe_warping_forward", "ebfi_iwe_warping_backward", "ebfi_iwe_averaged"}


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
    _i, _i64, _vp, _f, _d = ctypes.c_int, ctypes.c_int64, ctypes.c_void_p, ctypes.c_float, ctypes.c_double
    assert N.SIGNATURES["ebfi_iwe_workspace"] == (_i64, [_i64, _i64, _i, _i])
    assert N.SIGNATURES["ebfi_iwe_get_interpolation"] == (_i, [_vp, _vp, _i64, _i64, _f, _i, _i, _f, _i, _vp, _vp, _vp])
    assert N.SIGNATURES["ebfi_iwe_warping_forward"] == (_i, [_vp] + [_i64] * 4 + [_vp, _vp, _i64, _i64, _i, _i, _f, _d, _vp, _vp,
                                                             _vp, _i64, _vp])
    a = lib.ebfi_iwe_workspace(2, 1000, 12, 20)
    assert a > 0 and a % 256 == 0
    assert lib.ebfi_iwe_workspace(2, 2000, 12, 20) > a and lib.ebfi_iwe_workspace(2, 1000, 24, 20) > a
    assert lib.ebfi_iwe_workspace(1, 0, 1, 1) > 0
    for bad in ((0, 4, 4, 4), (1, -1, 4, 4), (1, 4, 0, 4), (1, 4, 4, 0), (1, 1 << 30, 4, 4), (4, 1 << 28, 4, 4),
                (1, 4, 1 << 16, 1 << 16), (2, 4, 1 << 16, 1 << 15)):
        assert lib.ebfi_iwe_workspace(*bad) == 0, bad
    assert lib.ebfi_iwe_workspace(1, (1 << 30) - 1, 4, 4) > 0
    b = lib.ebfi_iwe_index_bytes(2, 1000, 12, 20)
    assert 0 < b < a // 4 and b % 256 == 0 and lib.ebfi_iwe_index_bytes(2, 2000, 12, 20) > b      # B N entries, not 4 B N
    assert lib.ebfi_iwe_index_bytes(0, 4, 4, 4) == 0 and lib.ebfi_iwe_index_bytes(1, 1 << 30, 4, 4) == 0


def test_argument_errors_do_not_touch_the_gpu(lib):
    p = ctypes.c_void_p(256)               # never dereferenced: every call below is refused before a launch
    big = 1 << 40
    flow = (p, 80, 40, 10, 1)
    gi = lib.ebfi_iwe_get_interpolation
    assert gi(None, p, 1, 8, 1.0, 4, 4, 4.0, 0, p, p, None) == -1 and b"null" in lib.ebfi_last_error()
    assert gi(p, p, 0, 8, 1.0, 4, 4, 4.0, 0, p, p, None) == -1
    assert gi(p, p, 1, 1 << 30, 1.0, 4, 4, 4.0, 0, p, p, None) == N.EBFI_ERR_UNSUPPORTED
    assert gi(None, None, 1, 0, 1.0, 4, 4, 4.0, 0, None, None, None) == 0       # nothing to do
    it = lib.ebfi_iwe_interpolate
    assert it(p, 1, p, None, 1, 8, 4, 4, None, p, big, None) == -1
    assert it(None, 1, p, None, 1, 8, 4, 4, p, p, big, None) == -1
    assert it(p, 1, p, None, 1, -1, 4, 4, p, p, big, None) == -1
    assert it(p, 1, p, None, 1, 8, 4, 4, p, p, 16, None) == -4
    assert it(p, 1, p, None, 1, 8, 4, 4, p, ctypes.c_void_p(264), big, None) == -1 and b"aligned" in lib.ebfi_last_error()
    assert it(p, 1, p, None, 1, 8, 1 << 16, 1 << 16, p, p, big, None) == N.EBFI_ERR_UNSUPPORTED
    db = lib.ebfi_iwe_deblur
    assert db(*flow, p, 1, 8, 4, 4, 4.0, 1, 1, None, None, 1, None, p, big, None) == -1
    assert db(*flow, p, 1, 8, 4, 4, 4.0, 1, 2, p, None, 1, p, p, big, None) == -1       # two planes need two masks
    assert db(*flow, p, 1, 8, 4, 4, 4.0, 1, 3, p, p, 1, p, p, big, None) == -1 and b"planes" in lib.ebfi_last_error()
    assert db(*flow, None, 1, 8, 4, 4, 4.0, 1, 1, None, None, 1, p, p, big, None) == -1
    assert db(*flow, p, 1, 8, 4, 4, 4.0, 1, 1, None, None, 1, p, None, 0, None) == -4
    assert lib.ebfi_iwe_source_index(p, 1, 8, 4, 4, None, 0, None) == -4
    assert lib.ebfi_iwe_source_index(None, 1, 8, 4, 4, p, big, None) == -1
    fw = lib.ebfi_iwe_warping_forward
    assert fw(*flow, p, p, 1, 8, 4, 4, 4.0, 0.1, None, p, p, big, None) == -1
    assert fw(*flow, None, p, 1, 8, 4, 4, 4.0, 0.1, p, p, p, big, None) == -1
    assert fw(*flow, p, p, 1, 8, 4, 4, 4.0, 0.1, p, p, p, 64, None) == -4
    bw = lib.ebfi_iwe_warping_backward
    assert bw(*flow, p, p, 1, 8, 4, 4, 4.0, 0.1, p, p, big, None, p, None) == -1
    assert bw(*flow, p, p, 1, 8, 4, 4, 4.0, 0.1, p, None, 0, p, p, None) == -4
    av = lib.ebfi_iwe_averaged
    assert av(*flow, p, p, 1, 8, 4, 4, 4.0, None, p, big, None) == -1
    assert av(*flow, p, None, 1, 8, 4, 4, 4.0, p, p, big, None) == -1
    assert av(*flow, p, p, 1, 8, 4, 4, 4.0, p, p, 64, None) == -4


def test_the_library_puts_a_single_chain_on_the_callers_stream():
    """One chain of launches on the stream it is handed, nothing else: no stream or event of its own, no synchronisation, no
    copy, no allocation, and no float atomic (the only atomic is the integer histogram of the sort)."""
    src = open(os.path.join(ROOT, "ebfi-be_amd", "csrc", "iwe.hip")).read()
    for word in ("hipStreamCreate", "hipEventRecord", "hipStreamWaitEvent", "hipDeviceSynchronize", "hipStreamSynchronize",
                 "hipMemcpy", "hipMalloc", "hipLaunchCooperativeKernel", "unsafeAtomicAdd", "atomicAdd_system"):
        assert word not in src, word
    atomics = re.findall(r"atomic\w*\(([^;]*);", src)
    assert len(atomics) == 1 and atomics[0].startswith("&h[")             # uint32 LDS bins
    assert "#pragma clang fp contract(off)" in src
    assert src.count("hipLaunchKernelGGL(") == 1 and "hipLaunchKernelGGL(kern, grid, dim3(kBlock), 0, st, __VA_ARGS__)" in src
    assert src.count("IWE_LAUNCH(") >= 20
    assert len(re.findall(r"hipMemsetAsync\(p, 0, bytes, st\)", src)) == src.count("hipMemsetAsync(")


# ------------------------------------------------------------------ the Python surface
def test_shims_export_the_reference_names(golden_dir):
    import inspect
    rows = [line.split() for line in open(os.path.join(golden_dir, "loss_names.txt")).read().splitlines() if line.strip()]
    assert len(rows) == 16 and ["loss", "BrightnessConstancy"] not in rows
    for module, star in (("loss", "from loss import *"), ("myutils.iwe", "from myutils.iwe import *")):
        ns = {}
        exec(star, ns)
        for mod, name in rows:
            if mod == module:
                assert name in ns, (module, name)
    ns = {}
    exec("from loss import LaplacianLoss, Ternary, EventWarping, AveragedIWE", ns)      # the reference trainer's own uses
    import loss.flow
    import myutils.iwe as shim
    from ebfi_amd import iwe as I
    from ebfi_amd import loss as L
    assert ns["EventWarping"] is I.EventWarping is loss.flow.EventWarping and ns["AveragedIWE"] is I.AveragedIWE
    assert ns["LaplacianLoss"] is L.LaplacianLoss and ns["Ternary"] is L.Ternary
    want = {
        "purge_unfeasible": ["x", "res"],
        "get_interpolation": ["events", "flow", "tref", "res", "flow_scaling", "round_idx"],
        "interpolate": ["idx", "weights", "res", "polarity_mask"],
        "deblur_events": ["flow", "event_list", "res", "flow_scaling", "round_idx", "polarity_mask"],
        "compute_pol_iwe": ["flow", "event_list", "res", "pos_mask", "neg_mask", "flow_scaling", "round_idx"],
    }
    assert sorted(want) == sorted(shim.__all__) == sorted(name for mod, name in rows if mod == "myutils.iwe")
    for name, params in want.items():
        assert getattr(shim, name) is getattr(I, name)
        assert list(inspect.signature(getattr(I, name)).parameters) == params, name
    d = lambda f: {k: p.default for k, p in inspect.signature(f).parameters.items() if p.default is not inspect.Parameter.empty}
    assert d(I.get_interpolation) == {"round_idx": False} and d(I.interpolate) == {"polarity_mask": None}
    assert d(I.deblur_events) == {"flow_scaling": 128, "round_idx": True, "polarity_mask": None}
    assert d(I.compute_pol_iwe) == {"flow_scaling": 128, "round_idx": True}
    assert list(inspect.signature(I.EventWarping.forward).parameters) == ["self", "flow_list", "event_list", "pol_mask", "resolution"]
    assert list(inspect.signature(I.AveragedIWE.forward).parameters) == ["self", "flow", "event_list", "pol_mask"]
    config = {"loss": {"flow_regul_weight": 0.25}, "loader": {"resolution": [4, 6], "batch_size": 2}}
    assert I.EventWarping(config, "cpu").weight == 0.25
    a = I.AveragedIWE(config, "cpu")
    assert (a.res, a.flow_scaling, a.batch_size) == ([4, 6], 6, 2)


def test_purge_unfeasible_is_the_reference_rule():
    from ebfi_amd.iwe import purge_unfeasible
    x = torch.tensor([[[0.0, 0.0], [-1.0, 2.0], [3.0, 5.0], [4.0, 1.0], [2.0, 6.0], [2.0, -0.5]]])
    y, mask = purge_unfeasible(x, (4, 6))
    assert mask[0, :, 0].tolist() == [1, 0, 1, 0, 0, 0] and torch.equal(y, x * mask) and x[0, 1, 0] == -1
    y, mask = purge_unfeasible(torch.tensor([[[float("nan"), 1.0], [1.0, float("nan")], [-1.0, float("nan")]]]), (4, 6))
    assert mask[0, :, 0].tolist() == [1, 1, 0] and mask.dtype == torch.float32      # a NaN compares false: it is not purged


def test_the_wrappers_refuse_what_they_cannot_run():
    from unittest import mock
    from ebfi_amd import iwe as I
    config = {"loss": {"flow_regul_weight": 0.1}, "loader": {"resolution": [4, 4], "batch_size": 1}}
    z = lambda *s, **k: torch.zeros(*s, **k)
    ev, fl, pm, fe = z(1, 5, 4), z(1, 2, 4, 4), z(1, 5, 2), z(1, 5, 2)
    calls = {
        "get_interpolation": lambda ev=ev, fl=fl, pm=pm, fe=fe: I.get_interpolation(ev, fe, 1, (4, 4), 4),
        "interpolate": lambda ev=ev, fl=fl, pm=pm, fe=fe: I.interpolate(z(1, 5, 1, dtype=torch.long, device=ev.device), ev[:, :, 0:1],
                                                                       (4, 4), polarity_mask=pm[:, :, 0:1]),
        "deblur_events": lambda ev=ev, fl=fl, pm=pm, fe=fe: I.deblur_events(fl, ev, (4, 4)),
        "compute_pol_iwe": lambda ev=ev, fl=fl, pm=pm, fe=fe: I.compute_pol_iwe(fl, ev, (4, 4), pm[:, :, 0:1], pm[:, :, 1:2]),
        "EventWarping": lambda ev=ev, fl=fl, pm=pm, fe=fe: I.EventWarping(config, "cpu")([fl], ev, pm, (4, 4)),
        "AveragedIWE": lambda ev=ev, fl=fl, pm=pm, fe=fe: I.AveragedIWE(config, "cpu")(fl, ev, pm),
    }
    for name, call in calls.items():
        with pytest.raises(NotImplementedError):                          # CPU tensors
            call()
        for which in ("ev", "fl", "pm", "fe"):
            used = {"get_interpolation": ("ev", "fe"), "interpolate": ("ev", "pm")}.get(name, ("ev", "fl", "pm"))
            if which not in used or (name == "deblur_events" and which == "pm"):
                continue
            with pytest.raises(TypeError) as e:                           # float64
                call(**{which: dict(ev=ev, fl=fl, pm=pm, fe=fe)[which].double()})
            assert "float32" in str(e.value), (name, which)
    with pytest.raises(TypeError):
        I.interpolate(z(1, 5, 1, dtype=torch.int32), z(1, 5, 1), (4, 4))
    with pytest.raises(TypeError):
        I.deblur_events(fl, ev, (4, 4), round_idx=False)                  # the bilinear form needs its mask
    # the rest is decided after the device check: meta tensors stand in for GPU tensors, nothing is dereferenced
    m = lambda *s: torch.zeros(*s, device="meta")
    with mock.patch.object(N, "require_gpu", lambda *a: None):
        with pytest.raises(ValueError) as e:
            I.get_interpolation(ev, m(1, 5, 2), 1, (4, 4), 4)
        assert "different devices" in str(e.value)
        with pytest.raises(ValueError) as e:
            I.EventWarping(config, "cpu")([m(1, 2, 4, 4)], ev, pm, (4, 4))
        assert "different devices" in str(e.value)
        with pytest.raises(ValueError) as e:
            I.AveragedIWE(config, "cpu")(m(1, 2, 4, 4), m(1, 5, 4), pm)
        assert "different devices" in str(e.value)
        with pytest.raises(ValueError) as e:
            I.get_interpolation(m(1, 1 << 30, 4), m(1, 1 << 30, 2), 1, (4, 4), 4)
        assert "2**32" in str(e.value)
        with pytest.raises(ValueError) as e:
            I.EventWarping(config, "cpu")([m(2, 2, 4, 4)], m(2, 1 << 29, 4), m(2, 1 << 29, 2), (4, 4))
        assert "2**32" in str(e.value)
        with pytest.raises(ValueError) as e:
            I.deblur_events(m(1, 2, 1 << 16, 1 << 16), m(1, 5, 4), (1 << 16, 1 << 16))
        assert "2**32 - 1" in str(e.value)
        with pytest.raises(ValueError) as e:
            I.AveragedIWE(dict(config, loader={"resolution": [4, 4], "batch_size": 3}), "cpu")(m(1, 2, 4, 4), m(1, 5, 4), m(1, 5, 2))
        assert "batch_size" in str(e.value)
        with pytest.raises(ValueError):
            I.EventWarping(config, "cpu")([m(1, 2, 4, 5)], m(1, 5, 4), m(1, 5, 2), (4, 4))      # a flow of another size
        with pytest.raises(ValueError):
            I.compute_pol_iwe(m(1, 2, 4, 4), m(1, 5, 4), (4, 4), m(1, 5, 2), m(1, 5, 1))        # a mask of two columns
