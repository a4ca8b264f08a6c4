"""Host-side checks of the device encodings (ebfi_amd.encodings, csrc/encodings.hip, dataloader/encodings.py): the numpy
restatement the GPU tests use as their oracle (tests/encodings_ref.py) reproduces the REFERENCE'S OWN outputs
(tests/golden/encodings_small.npz, written by tests/golden/make_golden_encodings.py with one torch thread) bit for bit; the
fixture's fractional-weight cases really depend on the order of addition; the C ABI, the binding and the header agree; the shim
exports exactly the reference's names; CPU tensors, float64 lists and the undefined bilinear combination are refused.
No compute calls: there is no GPU here."""
import ctypes
import os

import numpy as np
import pytest
import torch

from ebfi_amd import _native as N

import encodings_ref as R

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
EVENT_CASES = ("c1", "b1", "n0", "n3", "n4", "tzero", "hot4096")
F = np.float32


@pytest.fixture(scope="module")
def golden(golden_dir):
    return np.load(os.path.join(golden_dir, "encodings_small.npz"))


def case(golden, name):
    v = {k: golden["%s__%s" % (name, k)] for k in ("xs", "ys", "ts", "tsn", "ps")}
    v.update(B=int(golden[name + "__B"]), ss=(int(golden[name + "__H"]), int(golden[name + "__W"])))
    return v


def restate(v):
    """Every event-list function of the restatement on one case, under the fixture's output names."""
    xs, ys, ts, tsn, ps, B, ss = (v[k] for k in ("xs", "ys", "ts", "tsn", "ps", "B", "ss"))
    xl, yl = np.trunc(xs).astype(np.int64), np.trunc(ys).astype(np.int64)
    return {
        "image": R.events_to_image(xs, ys, ps, ss),
        "image_torch": R.events_to_image_torch(xs, ys, ps, ss),
        "image_long": R.events_to_image_torch(xl, yl, ps, ss),
        "image_long_bilinear": R.events_to_image_torch(xl, yl, ps, ss, interpolation="bilinear"),
        "voxel_bilinear": R.events_to_voxel_torch(xs, ys, ts, ps, B, ss),
        "voxel_naive": R.events_to_voxel_torch(xs, ys, ts, ps, B, ss, temporal_bilinear=False),
        "voxel_norm": R.events_to_voxel(xs, ys, tsn, ps, B, ss),
        "stack_no_polarity": R.events_to_stack_no_polarity(xs, ys, ts, ps, B, ss),
        "channels": R.events_to_channels(xs, ys, ps, ss),
        "mask": R.events_to_mask(xs, ys, ps, ss),
        "bilinear_pad_clip": R.events_to_image_torch(xs, ys, ps, ss, interpolation="bilinear"),
        "bilinear_pad_noclip": R.events_to_image_torch(xs, ys, ps, ss, interpolation="bilinear", clip_out_of_range=False),
        "bilinear_nopad_clip": R.events_to_image_torch(xs, ys, ps, ss, interpolation="bilinear", padding=False),
        "polarity_mask": R.events_polarity_mask(ps),
    }


@pytest.mark.parametrize("name", EVENT_CASES)
def test_restatement_reproduces_the_reference(golden, name):
    v = case(golden, name)
    keep = {k: np.array(a) for k, a in v.items() if isinstance(a, np.ndarray)}
    for key, got in restate(v).items():
        want = golden["%s__%s" % (name, key)]
        assert got.dtype == np.float32 and got.shape == want.shape, (name, key, got.shape, want.shape)
        assert np.array_equal(got, want), (name, key, int((got != want).sum()))
    for k, a in keep.items():
        assert np.array_equal(v[k], a)                       # (the reference edits its inputs; the restatement must not)


def test_restatement_reproduces_the_reference_bilinear(golden):
    g = lambda k: golden["bil__" + k]
    ss = (int(g("H")), int(g("W")))
    for name, kw in (("pad_clip", {}), ("pad_noclip", dict(clip_out_of_range=False)), ("nopad_clip", dict(padding=False))):
        got = R.events_to_image_torch(g("xs"), g("ys"), g("ps"), ss, interpolation="bilinear", **kw)
        assert np.array_equal(got, g("out_" + name)), name
    assert g("out_pad_clip").shape == (ss[0] + 1, ss[1] + 1) and g("out_nopad_clip").shape == ss
    got = R.interpolate_to_image(g("px"), g("py"), g("dx"), g("dy"), g("w"), g("img"))
    assert np.array_equal(got, g("out_interpolate")) and not np.array_equal(got, g("img"))
    with pytest.raises(ValueError):
        R.events_to_image_torch(g("xs"), g("ys"), g("ps"), ss, clip_out_of_range=False, interpolation="bilinear", padding=False)


def test_restatement_reproduces_the_reference_masks_and_counts(golden):
    for c in "ab":
        got = R.events_to_mask(golden["mask__%s_xs" % c], golden["mask__%s_ys" % c], golden["mask__%s_ps" % c], (1, 4))
        assert np.array_equal(got, golden["mask__%s_out" % c]), c
    assert golden["mask__a_out"].tolist() == [[0, 0, 1, 0]]          # last writer wins
    assert golden["mask__b_out"].tolist() == [[0, 0, 0, 1]]          # an out-of-range last writer clears (0,0)
    for name, idx, max_px in (("all", 10, 100), ("two", 10, 2), ("young", 5, 100)):
        mask, rate = R.get_hot_event_mask(golden["hot__rate"], idx, max_px=max_px)
        assert np.array_equal(mask, golden["hot__%s_mask" % name]) and np.array_equal(rate, golden["hot__%s_rate" % name]), name
    mask, rate = R.get_hot_event_mask(golden["hot__nan_in"], 10)
    assert np.array_equal(mask, golden["hot__nan_mask"]) and np.array_equal(rate, golden["hot__nan_rate"], equal_nan=True)
    assert np.array_equal(R.stack2cnt(golden["cnt__stack"]), golden["cnt__out"])


def test_fixture_cases_exercise_what_they_are_for(golden):
    v = case(golden, "c1")
    xs, ys, ts, ps, B, (H, W) = v["xs"], v["ys"], v["ts"], v["ps"], v["B"], v["ss"]
    assert (H, W, B, len(ts)) == (5, 7, 5, 64)
    ok, iy, ix = R.pixel(xs, ys, H, W)
    frac = ok & (iy == 2) & (ix == 3) & (ps != np.rint(ps))
    assert frac.sum() >= 3                                               # several fractional weights on one pixel
    assert (xs == -1).any() and (xs == W).any() and (ys == H).any()     # the three borders
    assert (np.diff(ts) == 0).sum() >= 2 and (np.diff(ts) >= 0).all()   # duplicate stamps, sorted
    bounds = R.naive_bounds(ts, B)
    shared = [k for k in np.flatnonzero(~ok) if sum(b <= k < e for b, e in bounds) >= 2]
    assert shared                                                        # an out-of-range event in two naive bins
    delta_t = F(R.time_span(ts) / F(B))
    edges = [F(ts[0] + F(delta_t * F(b))) for b in range(1, B)]
    assert all((ts == e).any() for e in edges)                           # stamps exactly on the bin edges
    tn = (ts - ts[0]) / R.time_span(ts) * F(B - 1)
    assert tn[0] == 0                                                    # ... and on a bin centre
    assert (~ok & (ps < 0)).any() and (~ok & (ps > 0)).any()
    # rule 1 is live: a later bin of the voxel grid has weight at (0,0) that bin 0's in-range events alone do not explain
    vox = golden["c1__voxel_bilinear"]
    ay, ax, ws = R.voxel_addends(xs, ys, ts, ps, B, (H, W))
    dropped = np.stack([R.scatter((H, W), ay, ax, np.where(ok, wb, F(0))) for wb in ws])
    assert np.array_equal(vox[0], dropped[0]) and not np.array_equal(vox[1:, 0, 0], dropped[1:, 0, 0])
    # rule 3 is live: the negative channel counts an out-of-range event at (0,0), the positive one does not
    ch = golden["c1__channels"]
    inside = R.events_to_channels(xs[ok], ys[ok], ps[ok], (H, W))
    assert np.array_equal(ch[0], inside[0]) and ch[1, 0, 0] != inside[1, 0, 0]
    hot = case(golden, "hot4096")
    assert len(hot["ts"]) == 4096 and len(set(zip(hot["xs"].tolist(), hot["ys"].tolist()))) == 1
    assert not golden["tzero__ts"].any() and not golden["tzero__voxel_bilinear"].any() and golden["tzero__voxel_norm"].any()
    assert not golden["n3__voxel_bilinear"].any() and golden["n4__voxel_bilinear"].any() and golden["n3__voxel_norm"].any()
    st = golden["cnt__stack"]
    assert (np.abs(st - np.trunc(st)) == 0.5).any() and ((st < 0) & (np.abs(st - np.trunc(st)) == 0.5)).any()
    assert golden["cnt__out"][0, 0, 0, 0] == 4 and golden["cnt__out"][0, 1, 0, 0] == 4      # 0 + 2 + 2 and 0 + 2 + 2


@pytest.mark.parametrize("name", ["c1", "hot4096"])
def test_the_order_of_addition_is_exercised(golden, name):
    """A fixture on which every order gives the same bits proves nothing about ordering: feeding each pixel its addends in the
    REVERSED order must change at least one output bit of every fractional-weight function."""
    v = case(golden, name)
    xs, ys, ts, ps, B, (H, W) = v["xs"], v["ys"], v["ts"], v["ps"], v["B"], v["ss"]
    ok, iy, ix = R.pixel(xs, ys, H, W)
    w = np.where(ok, ps, F(0))
    fwd = R.serial_sum((H, W), iy, ix, w)
    assert np.array_equal(fwd, golden[name + "__image"])                 # the plain loop is the law np.add.at follows
    assert not np.array_equal(R.serial_sum((H, W), iy, ix, w, reverse=True), fwd)
    iy, ix, ws = R.voxel_addends(xs, ys, ts, ps, B, (H, W))
    fwd = np.stack([R.serial_sum((H, W), iy, ix, wb) for wb in ws])
    rev = np.stack([R.serial_sum((H, W), iy, ix, wb, reverse=True) for wb in ws])
    assert np.array_equal(fwd, golden[name + "__voxel_bilinear"]) and not np.array_equal(rev, fwd)
    ch = (ps * np.where(ps > 0, F(0), ps)).astype(F)
    assert not np.array_equal(R.serial_sum((H, W), iy, ix, ch, reverse=True), golden[name + "__channels"][1])


def test_the_pass_order_of_the_bilinear_image_is_exercised(golden):
    g = lambda k: golden["bil__" + k]
    px, py, dx, dy, w = (g(k) for k in ("px", "py", "dx", "dy", "w"))
    rev = slice(None, None, -1)
    swapped = R.interpolate_to_image(px[rev], py[rev], dx[rev], dy[rev], w[rev], g("img"))
    assert not np.array_equal(swapped, g("out_interpolate"))
    # one index_put_ per corner in turn is not the same sum as event by event with its four corners
    img = np.array(g("img"))
    one = F(1)
    for k in range(len(w)):
        for oy, ox, a in ((0, 0, w[k] * (one - dx[k]) * (one - dy[k])), (0, 1, w[k] * dx[k] * (one - dy[k])),
                          (1, 0, w[k] * (one - dx[k]) * dy[k]), (1, 1, w[k] * dx[k] * dy[k])):
            img[py[k] + oy, px[k] + ox] = F(img[py[k] + oy, px[k] + ox] + F(a))
    assert not np.array_equal(img, g("out_interpolate"))


# ------------------------------------------------------------------ the ABI
NEW = {"ebfi_events_grid_workspace", "ebfi_events_to_grid", "ebfi_interpolate_to_image", "ebfi_hot_event_mask",
       "ebfi_stack_to_cnt", "ebfi_polarity_mask"}


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
    assert "#define EBFI_ABI_VERSION 14" in header                      # a pure addition: the generation stays
    assert lib.ebfi_abi_version() == 14 == N.ABI_VERSION
    modes = ["IMAGE", "VOXEL_BILINEAR", "VOXEL_NORMALISED", "VOXEL_NAIVE", "STACK_NO_POLARITY", "CHANNELS", "MASK",
             "BILINEAR_PADDED", "BILINEAR_CLIPPED"]
    assert [N.CONSTANTS["EBFI_GRID_" + m] for m in modes] == list(range(9))
    _i, _i64, _vp = ctypes.c_int, ctypes.c_int64, ctypes.c_void_p
    assert N.SIGNATURES["ebfi_events_to_grid"] == (_i, [_vp] * 4 + [_i64] + [_i] * 4 + [_vp, _vp, _i64, _vp])
    assert N.SIGNATURES["ebfi_events_grid_workspace"] == (_i64, [_i64, _i, _i, _i])
    assert N.SIGNATURES["ebfi_events_to_stack"][1][:4] == [_vp] * 4 and lib.ebfi_events_workspace(16) == 33 * 8      # untouched
    # the workspace query is host arithmetic and grows with the events, the pixels and the bins
    a = lib.ebfi_events_grid_workspace(1000, 5, 180, 240)
    assert a > 0 and a % 256 == 0
    assert lib.ebfi_events_grid_workspace(2000, 5, 180, 240) > a and lib.ebfi_events_grid_workspace(1000, 5, 360, 240) > a
    assert lib.ebfi_events_grid_workspace(1000, 500, 180, 240) > a
    assert lib.ebfi_events_grid_workspace(0, 1, 1, 1) > 0
    for bad in ((-1, 1, 4, 4), (4, 0, 4, 4), (4, 1, 0, 4), (4, 1, 4, 0), (1 << 31, 1, 4, 4), (4, 1, 1 << 16, 1 << 16)):
        assert lib.ebfi_events_grid_workspace(*bad) == 0, bad


def test_argument_errors_do_not_touch_the_gpu(lib):
    p = ctypes.c_void_p(256)               # never dereferenced: every call below is refused before a launch
    big = 1 << 30
    grid = lambda *a: lib.ebfi_events_to_grid(*a)
    assert grid(p, p, p, p, 8, 1, 5, 4, 4, None, p, big, None) == -1 and b"null" in lib.ebfi_last_error()
    assert grid(None, p, p, p, 8, 1, 5, 4, 4, p, p, big, None) == -1
    assert grid(p, p, None, p, 8, 1, 5, 4, 4, p, p, big, None) == -1           # a timed mode needs the stamps
    assert grid(p, p, p, p, -1, 1, 5, 4, 4, p, p, big, None) == -1
    assert grid(p, p, p, p, 8, 1, 0, 4, 4, p, p, big, None) == -1
    assert grid(p, p, p, p, 8, 1, 5, 0, 4, p, p, big, None) == -1
    assert grid(p, p, p, p, 8, 9, 1, 4, 4, p, p, big, None) == -1 and b"mode" in lib.ebfi_last_error()
    assert grid(p, p, p, p, 8, -1, 1, 4, 4, p, p, big, None) == -1
    assert grid(p, p, None, p, 8, 0, 2, 4, 4, p, p, big, None) == -1          # an image is one plane
    assert grid(p, p, None, p, 8, 5, 1, 4, 4, p, p, big, None) == -1          # channels are two
    need = lib.ebfi_events_grid_workspace(8, 5, 4, 4)
    assert grid(p, p, p, p, 8, 1, 5, 4, 4, p, p, need - 1, None) == -4
    assert grid(p, p, p, p, 8, 1, 5, 4, 4, p, None, 0, None) == -4
    assert grid(p, p, p, p, 8, 1, 5, 4, 4, p, ctypes.c_void_p(264), big, None) == -1 and b"aligned" in lib.ebfi_last_error()
    assert grid(p, p, p, p, 1 << 31, 1, 5, 4, 4, p, p, big, None) == N.EBFI_ERR_UNSUPPORTED
    interp = lambda *a: lib.ebfi_interpolate_to_image(*a)
    assert interp(p, p, p, p, p, 8, 4, 4, None, p, big, None) == -1
    assert interp(p, None, p, p, p, 8, 4, 4, p, p, big, None) == -1
    assert interp(p, p, p, p, p, 8, 0, 4, p, p, big, None) == -1
    assert interp(p, p, p, p, p, 8, 4, 4, p, p, 16, None) == -4
    assert interp(p, p, p, p, p, 0, 4, 4, p, None, 0, None) == 0              # nothing to add: a no-op
    assert lib.ebfi_hot_event_mask(None, 4, 4, 1, 0.8, p, None) == -1
    assert lib.ebfi_hot_event_mask(p, 0, 4, 1, 0.8, p, None) == -1
    assert lib.ebfi_hot_event_mask(p, 4, 4, -1, 0.8, p, None) == -1
    assert lib.ebfi_stack_to_cnt(None, 1, 2, 16, p, None) == -1 and lib.ebfi_stack_to_cnt(p, -1, 2, 16, p, None) == -1
    assert lib.ebfi_stack_to_cnt(p, 0, 2, 16, p, None) == 0
    assert lib.ebfi_polarity_mask(None, 4, p, None) == -1 and lib.ebfi_polarity_mask(p, -1, p, None) == -1
    assert lib.ebfi_polarity_mask(p, 0, p, None) == 0


def test_the_library_puts_a_single_chain_on_the_callers_stream():
    """A captured call must be one chain of launches with no parallel branch: the translation unit launches on the stream it is
    handed only -- it creates no stream, records and waits for no event, synchronises nothing and copies nothing to the host."""
    src = open(os.path.join(ROOT, "ebfi-be_amd", "csrc", "encodings.hip")).read()
    for word in ("hipStreamCreate", "hipEventRecord", "hipStreamWaitEvent", "hipDeviceSynchronize", "hipStreamSynchronize",
                 "hipMemcpy", "hipMalloc", "hipLaunchCooperativeKernel"):
        assert word not in src, word
    launches = src.count("hipLaunchKernelGGL(")
    assert launches >= 12
    import re
    for m in re.finditer(r"hipLaunchKernelGGL\(([^;]*);", src):
        if "EBFI_GRID_LAUNCH(M)" in src[max(0, m.start() - 40):m.start()] or "grid_accumulate<M>" in m.group(1):
            assert ", st, " in m.group(1)
            continue
        assert ", 0, st, " in m.group(1), m.group(1)[:80]                      # every launch names the caller's stream


# ------------------------------------------------------------------ the Python surface
def test_shim_exports_exactly_the_reference_names(golden_dir):
    import inspect
    names = open(os.path.join(golden_dir, "encodings_names.txt")).read().split()
    assert len(names) == 14
    ns = {}
    exec("from dataloader.encodings import *", ns)
    assert sorted(k for k in ns if k != "__builtins__") == sorted(names)
    import dataloader.encodings as shim
    from ebfi_amd import encodings as E
    want = {
        "interpolate_to_image": ["pxs", "pys", "dxs", "dys", "weights", "img"],
        "events_to_image_torch": ["xs", "ys", "ps", "device", "sensor_size", "clip_out_of_range", "interpolation", "padding"],
        "binary_search_torch_tensor": ["t", "l", "r", "x", "side"],
        "events_to_voxel_torch": ["xs", "ys", "ts", "ps", "B", "device", "sensor_size", "temporal_bilinear"],
        "events_to_stack_polarity": ["xs", "ys", "ts", "ps", "B", "device", "sensor_size"],
        "events_to_stack_no_polarity": ["xs", "ys", "ts", "ps", "B", "device", "sensor_size"],
        "events_to_image": ["xs", "ys", "ps", "sensor_size"],
        "events_to_voxel": ["xs", "ys", "ts", "ps", "num_bins", "sensor_size"],
        "events_to_channels": ["xs", "ys", "ps", "sensor_size"],
        "events_to_stack": ["xs", "ys", "ts", "ps", "B", "sensor_size"],
        "events_to_mask": ["xs", "ys", "ps", "sensor_size"],
        "events_polarity_mask": ["ps"],
        "get_hot_event_mask": ["event_rate", "idx", "max_px", "min_obvs", "max_rate"],
        "stack2cnt": ["stack"],
    }
    assert sorted(want) == sorted(names)
    for name, params in want.items():
        f = getattr(shim, name)
        assert f is getattr(E, name)
        sig = inspect.signature(f)
        assert list(sig.parameters) == params, name
        if "sensor_size" in params:
            assert sig.parameters["sensor_size"].default == (180, 240)
    d = {k: p.default for k, p in inspect.signature(E.events_to_image_torch).parameters.items()}
    assert (d["device"], d["clip_out_of_range"], d["interpolation"], d["padding"]) == (None, True, None, True)
    d = {k: p.default for k, p in inspect.signature(E.get_hot_event_mask).parameters.items()}
    assert (d["max_px"], d["min_obvs"], d["max_rate"]) == (100, 5, 0.8)
    assert inspect.signature(E.events_to_voxel_torch).parameters["temporal_bilinear"].default is True


def test_binary_search_is_the_reference_search():
    from ebfi_amd.encodings import binary_search_torch_tensor as bs
    t = torch.tensor([0.0, 0.5, 0.5, 0.5, 1.0, 2.0])
    a = t.numpy()
    for x in (-1.0, 0.0, 0.25, 0.5, 0.75, 1.0, 2.0, 3.0):
        for side in ("left", "right"):
            assert bs(t, 0, len(t) - 1, x, side=side) == R.bsearch(a, 0, len(a) - 1, x, side)
    assert bs(t, 0, None, 1.0) == 4


def test_cpu_tensors_float64_and_the_undefined_bilinear_form_are_refused():
    from ebfi_amd import encodings as E
    z = lambda n=5: torch.zeros(n)
    zl = lambda n=5: torch.zeros(n, dtype=torch.long)
    calls = [
        lambda: E.events_to_image(z(), z(), z(), (4, 4)),
        lambda: E.events_to_image(zl(), zl(), z(), (4, 4)),
        lambda: E.events_to_image_torch(z(), z(), z(), sensor_size=(4, 4)),
        lambda: E.events_to_image_torch(z(), z(), z(), sensor_size=(4, 4), interpolation="bilinear"),
        lambda: E.interpolate_to_image(zl(), zl(), z(), z(), z(), torch.zeros(4, 4)),
        lambda: E.events_to_voxel_torch(z(), z(), z(), z(), 4, sensor_size=(4, 4)),
        lambda: E.events_to_voxel_torch(z(), z(), z(), z(), 4, sensor_size=(4, 4), temporal_bilinear=False),
        lambda: E.events_to_voxel(z(), z(), z(), z(), 4, (4, 4)),
        lambda: E.events_to_stack_polarity(z(), z(), z(), z(), 4, sensor_size=(4, 4)),
        lambda: E.events_to_stack_no_polarity(z(), z(), z(), z(), 4, sensor_size=(4, 4)),
        lambda: E.events_to_channels(z(), z(), z(), (4, 4)),
        lambda: E.events_to_mask(z(), z(), z(), (4, 4)),
        lambda: E.events_polarity_mask(z()),
        lambda: E.get_hot_event_mask(torch.zeros(4, 4), 10),
        lambda: E.stack2cnt(torch.zeros(1, 2, 4, 4)),
    ]
    for k, call in enumerate(calls):
        with pytest.raises(NotImplementedError):
            call()
    d = lambda n=5: torch.zeros(n, dtype=torch.float64)
    for k, call in enumerate([
        lambda: E.events_to_voxel_torch(z(), z(), d(), z(), 4, sensor_size=(4, 4)),
        lambda: E.events_to_voxel_torch(d(), d(), d(), z(), 4, sensor_size=(4, 4)),
        lambda: E.events_to_voxel(z(), z(), d(), z(), 4, (4, 4)),
        lambda: E.events_to_stack_no_polarity(z(), z(), d(), z(), 4, sensor_size=(4, 4)),
        lambda: E.events_to_image(d(), z(), z(), (4, 4)),
        lambda: E.events_to_image(z(), z(), d(), (4, 4)),
        lambda: E.events_to_channels(z(), z(), d(), (4, 4)),
        lambda: E.events_to_mask(z(), d(), z(), (4, 4)),
        lambda: E.events_polarity_mask(d()),
        lambda: E.interpolate_to_image(zl(), zl(), d(), z(), z(), torch.zeros(4, 4)),
        lambda: E.get_hot_event_mask(torch.zeros(4, 4, dtype=torch.float64), 10),
        lambda: E.stack2cnt(torch.zeros(1, 2, 4, 4, dtype=torch.float64)),
    ]):
        with pytest.raises(TypeError) as e:
            call()
        assert "float32" in str(e.value), k
    with pytest.raises(ValueError) as e:
        E.events_to_image_torch(z(), z(), z(), sensor_size=(4, 4), clip_out_of_range=False, interpolation="bilinear", padding=False)
    assert "IndexError" in str(e.value)
    with pytest.raises(ValueError):
        E.events_to_image_torch(z(), z(), z(), sensor_size=(4, 4), interpolation="cubic")
    with pytest.raises(ValueError):
        E.events_to_voxel_torch(z(), z(), z(), z(), 4, device="cuda:0", sensor_size=(4, 4))
    # tensors of one call on two devices are refused before anything is dereferenced (meta tensors stand in for a second GPU)
    from unittest import mock
    m = lambda: torch.zeros(5, device="meta")
    with mock.patch.object(N, "require_gpu", lambda *a: None):
        with pytest.raises(ValueError) as e:
            E.events_to_image(z(), m(), z(), (4, 4))
        assert "different devices" in str(e.value)
        with pytest.raises(ValueError):
            E.interpolate_to_image(zl(), zl(), z(), z(), m(), torch.zeros(4, 4))
