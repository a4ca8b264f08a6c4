"""GPU checks of the device encodings (ebfi_amd.encodings, csrc/encodings.hip).  Every comparison is torch.equal: the law is a
serial fp32 sum per pixel in event-list order with single-rounded, unfused arithmetic, so there is no tolerance to choose.  The
expected values are what the reference itself returned (tests/golden/encodings_small.npz) or, where a fixture would be too
large, the numpy restatement that tests/test_encodings_host.py holds against that fixture (tests/encodings_ref.py)."""
import os

import numpy as np
import pytest
import torch

import encodings_ref as R

pytestmark = pytest.mark.gpu
F = np.float32


@pytest.fixture(scope="module")
def golden(golden_dir):
    return np.load(os.path.join(golden_dir, "encodings_small.npz"))


@pytest.fixture(scope="module")
def E():
    from ebfi_amd import encodings
    return encodings


def dev(a):
    return torch.from_numpy(np.ascontiguousarray(a)).cuda()


def case(golden, name):
    v = {k: golden["%s__%s" % (name, k)] for k in ("xs", "ys", "ts", "tsn", "ps")}
    v.update(B=int(golden[name + "__B"]), ss=(int(golden[name + "__H"]), int(golden[name + "__W"])))
    return v


def run_all(E, v):
    """Every event-list function on one case, under the fixture's output names.  The inputs are uploaded once and checked
    bit-unchanged after every call (the reference edits them; ours must not)."""
    B, ss = v["B"], v["ss"]
    t = {k: dev(v[k]) for k in ("xs", "ys", "ts", "tsn", "ps")}
    t["xl"], t["yl"] = dev(np.trunc(v["xs"]).astype(np.int64)), dev(np.trunc(v["ys"]).astype(np.int64))
    keep = {k: a.clone() for k, a in t.items()}
    xs, ys, ts, tsn, ps, xl, yl = (t[k] for k in ("xs", "ys", "ts", "tsn", "ps", "xl", "yl"))
    calls = {
        "image": lambda: E.events_to_image(xs, ys, ps, ss),
        "image_torch": lambda: E.events_to_image_torch(xs, ys, ps, sensor_size=ss),
        "image_long": lambda: E.events_to_image_torch(xl, yl, ps, sensor_size=ss),
        "image_long_bilinear": lambda: E.events_to_image_torch(xl, yl, ps, sensor_size=ss, interpolation="bilinear"),
        "voxel_bilinear": lambda: E.events_to_voxel_torch(xs, ys, ts, ps, B, sensor_size=ss),
        "voxel_naive": lambda: E.events_to_voxel_torch(xs, ys, ts, ps, B, sensor_size=ss, temporal_bilinear=False),
        "voxel_norm": lambda: E.events_to_voxel(xs, ys, tsn, ps, B, ss),
        "stack_no_polarity": lambda: E.events_to_stack_no_polarity(xs, ys, ts, ps, B, device=xs.device, sensor_size=ss),
        "channels": lambda: E.events_to_channels(xs, ys, ps, ss),
        "mask": lambda: E.events_to_mask(xs, ys, ps, ss),
        "bilinear_pad_clip": lambda: E.events_to_image_torch(xs, ys, ps, sensor_size=ss, interpolation="bilinear"),
        "bilinear_pad_noclip": lambda: E.events_to_image_torch(xs, ys, ps, sensor_size=ss, interpolation="bilinear",
                                                               clip_out_of_range=False),
        "bilinear_nopad_clip": lambda: E.events_to_image_torch(xs, ys, ps, sensor_size=ss, interpolation="bilinear", padding=False),
        "polarity_mask": lambda: E.events_polarity_mask(ps),
    }
    out = {}
    for name, call in calls.items():
        a = call()
        b = call()                                           # reproducibility: the same bits twice in one process
        assert a.is_cuda and a.dtype == torch.float32 and torch.equal(a, b), name
        assert a.cpu().numpy().tobytes() == b.cpu().numpy().tobytes(), name
        for k, orig in keep.items():
            assert torch.equal(t[k], orig), (name, k)         # immutability
        out[name] = a
    return out


def expect(want):
    return torch.from_numpy(np.ascontiguousarray(want)).cuda()


@pytest.mark.parametrize("name", ["c1", "b1", "n0", "n3", "n4", "tzero", "hot4096"])
def test_fixture_cases(golden, E, name):
    """Cases 1 to 3: the 5 x 7 grid with everything at once; B = 1, N in {0, 3, 4}, all stamps zero; 4096 events on one pixel
    (the sort has one path for every run length; the walk switches at 64: test_run_lengths_around_the_wave_walk)."""
    got = run_all(E, case(golden, name))
    for key, a in got.items():
        want = golden["%s__%s" % (name, key)]
        assert tuple(a.shape) == want.shape, (name, key)
        assert torch.equal(a, expect(want)), (name, key, int((a != expect(want)).sum()))


@pytest.mark.parametrize("n_hot", [63, 64, 65, 130])
def test_run_lengths_around_the_wave_walk(E, n_hot):
    """Case 3, second part: a run of 64 events or more is walked by the whole wave, a shorter one by its own lane.  One pixel
    with n_hot events (one below the switch, at it, one above, two full rounds and a partial one), a second long run of 70 in
    the same wave, and 40 scattered events, interleaved in the list: the bits of the serial restatement on either path."""
    rng = np.random.default_rng(n_hot)
    H, W, B = 8, 8, 5
    n = n_hot + 70 + 40
    xs = rng.uniform(-0.5, W + 0.25, n).astype(F)
    ys = rng.uniform(-0.5, H + 0.25, n).astype(F)
    where = rng.permutation(n)
    xs[where[:n_hot]], ys[where[:n_hot]] = F(3.25), F(5.75)
    xs[where[n_hot:n_hot + 70]], ys[where[n_hot:n_hot + 70]] = F(6.5), F(1.5)
    ps = rng.uniform(-1.5, 1.5, n).astype(F)
    ts = np.sort(rng.uniform(0.125, 0.875, n)).astype(F)
    tsn = ((ts - ts[0]) / (ts[-1] - ts[0])).astype(F)
    ss = (H, W)
    want = {
        "image": R.events_to_image(xs, ys, ps, ss),
        "voxel_bilinear": R.events_to_voxel_torch(xs, ys, ts, ps, B, ss),
        "voxel_naive": R.events_to_voxel_torch(xs, ys, ts, ps, B, ss, temporal_bilinear=False),
        "voxel_norm": R.events_to_voxel(xs, ys, tsn, ps, B, ss),
        "stack_no_polarity": R.events_to_stack_no_polarity(xs, ys, ts, ps, B, ss),
        "channels": R.events_to_channels(xs, ys, ps, ss),
        "mask": R.events_to_mask(xs, ys, ps, ss),
    }
    assert (want["image"] != R.serial_sum(ss, *R.pixel(xs, ys, H, W)[1:], np.where(R.in_range(xs, ys, H, W), ps, F(0)),
                                          reverse=True)).any()                      # the order matters on this list
    got = run_all(E, dict(xs=xs, ys=ys, ts=ts, tsn=tsn, ps=ps, B=B, ss=ss))
    for key, w in want.items():
        assert torch.equal(got[key], expect(w)), (key, int((got[key] != expect(w)).sum()))


@pytest.fixture(scope="module")
def uniform():
    """Case 4: 33 x 65, N = 20000 uniform -- 79 workgroups in the sort, 20 tiles in the scan, 9 in the accumulation."""
    rng = np.random.default_rng(4)
    H, W, B, n = 33, 65, 5, 20000
    xs = rng.uniform(-0.5, W + 0.25, n).astype(F)
    ys = rng.uniform(-0.5, H + 0.25, n).astype(F)
    ps = rng.uniform(-1.5, 1.5, n).astype(F)
    ts = np.sort(rng.uniform(0.125, 0.875, n)).astype(F)
    tsn = ((ts - ts[0]) / (ts[-1] - ts[0])).astype(F)
    return dict(xs=xs, ys=ys, ts=ts, tsn=tsn, ps=ps, B=B, ss=(H, W))


def test_uniform_list_over_several_workgroups(E, uniform):
    v = uniform
    xs, ys, ts, tsn, ps, B, ss = (v[k] for k in ("xs", "ys", "ts", "tsn", "ps", "B", "ss"))
    xl, yl = np.trunc(xs).astype(np.int64), np.trunc(ys).astype(np.int64)
    want = {
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
    got = run_all(E, v)
    assert sorted(got) == sorted(want)
    for key, a in got.items():
        assert torch.equal(a, expect(want[key])), (key, int((a != expect(want[key])).sum()))


def test_uniform_voxel_replays_from_a_graph(E, uniform):
    """The case-4 voxel grid captured into a graph and replayed twice: the same bits as the eager call.  The call puts a single
    chain of launches on the capturing stream: no side stream, no host read."""
    v = uniform
    xs, ys, ts, ps = (dev(v[k]) for k in ("xs", "ys", "ts", "ps"))
    eager = E.events_to_voxel_torch(xs, ys, ts, ps, v["B"], sensor_size=v["ss"])
    torch.cuda.synchronize()
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        out = E.events_to_voxel_torch(xs, ys, ts, ps, v["B"], sensor_size=v["ss"])
    for _ in range(2):
        out.zero_()
        graph.replay()
        torch.cuda.synchronize()
        assert torch.equal(out, eager)
    assert torch.equal(eager, expect(R.events_to_voxel_torch(v["xs"], v["ys"], v["ts"], v["ps"], v["B"], v["ss"])))


def test_default_sensor_voxel(E):
    """Case 5: 180 x 240 (the module's default sensor_size), N = 100000, B = 5, voxel only: 391 sort workgroups, so the
    [digit][workgroup] table has 100096 entries and its scan crosses 97 tile boundaries."""
    rng = np.random.default_rng(5)
    H, W, B, n = 180, 240, 5, 100000
    xs = rng.uniform(-1.0, W + 1.0, n).astype(F)
    ys = rng.uniform(-1.0, H + 1.0, n).astype(F)
    ps = rng.choice(np.array([-1.0, 1.0, 0.3, -0.7], F), n)
    ts = np.sort(rng.uniform(10.0, 10.5, n)).astype(F)
    txs, tys, tts, tps = dev(xs), dev(ys), dev(ts), dev(ps)
    got = E.events_to_voxel_torch(txs, tys, tts, tps, B)
    assert torch.equal(got, expect(R.events_to_voxel_torch(xs, ys, ts, ps, B, (H, W))))
    for a, b in ((txs, xs), (tys, ys), (tts, ts), (tps, ps)):
        assert torch.equal(a, dev(b))


def test_bilinear_images(golden, E):
    """Case 6: fractional coordinates that reach the last column and row, both paddings, both clip settings where defined,
    interpolate_to_image on a pre-filled image (contiguous and as a strided view)."""
    g = lambda k: golden["bil__" + k]
    ss = (int(g("H")), int(g("W")))
    xs, ys, ps = dev(g("xs")), dev(g("ys")), dev(g("ps"))
    keep = [a.clone() for a in (xs, ys, ps)]
    assert ((g("xs") >= ss[1] - 1) & (g("xs") < ss[1])).any() and ((g("ys") >= ss[0] - 1) & (g("ys") < ss[0])).any()
    for name, kw in (("pad_clip", {}), ("pad_noclip", dict(clip_out_of_range=False)), ("nopad_clip", dict(padding=False))):
        a = E.events_to_image_torch(xs, ys, ps, sensor_size=ss, interpolation="bilinear", **kw)
        b = E.events_to_image_torch(xs, ys, ps, sensor_size=ss, interpolation="bilinear", **kw)
        assert torch.equal(a, expect(g("out_" + name))) and torch.equal(a, b), name
    with pytest.raises(ValueError):
        E.events_to_image_torch(xs, ys, ps, sensor_size=ss, clip_out_of_range=False, interpolation="bilinear", padding=False)
    px, py, dx, dy, w = (dev(g(k)) for k in ("px", "py", "dx", "dy", "w"))
    keep += [a.clone() for a in (px, py, dx, dy, w)]
    img = dev(g("img"))
    assert E.interpolate_to_image(px, py, dx, dy, w, img) is None
    assert torch.equal(img, expect(g("out_interpolate")))
    again = dev(g("img"))
    E.interpolate_to_image(px, py, dx, dy, w, again)
    assert again.cpu().numpy().tobytes() == img.cpu().numpy().tobytes()          # the same bits twice
    wide = torch.zeros(ss[0] + 1, 2 * (ss[1] + 1), device="cuda")
    view = wide[:, ::2]
    view.copy_(dev(g("img")))
    E.interpolate_to_image(px, py, dx, dy, w, view)
    assert torch.equal(view, expect(g("out_interpolate"))) and not wide[:, 1::2].any()
    for a, b in zip((xs, ys, ps, px, py, dx, dy, w), keep):
        assert torch.equal(a, b)


def test_mask_last_writer_wins(golden, E):
    """Case 7: 1 x 4, duplicates, and an out-of-range last writer at (0,0)."""
    for c in "ab":
        xs, ys, ps = (dev(golden["mask__%s_%s" % (c, k)]) for k in ("xs", "ys", "ps"))
        keep = [a.clone() for a in (xs, ys, ps)]
        a = E.events_to_mask(xs, ys, ps, (1, 4))
        assert torch.equal(a, expect(golden["mask__%s_out" % c])) and torch.equal(a, E.events_to_mask(xs, ys, ps, (1, 4))), c
        assert all(torch.equal(x, k) for x, k in zip((xs, ys, ps), keep))
    assert golden["mask__a_out"].tolist() == [[0, 0, 1, 0]] and golden["mask__b_out"].tolist() == [[0, 0, 0, 1]]


def test_hot_event_mask(golden, E):
    """Case 8: two equal maxima, max_px below the number of hot pixels, idx <= min_obvs, a NaN; event_rate is edited in place
    exactly as the reference edits it."""
    for name, idx, max_px in (("all", 10, 100), ("two", 10, 2), ("young", 5, 100)):
        rate = dev(golden["hot__rate"])
        mask = E.get_hot_event_mask(rate, idx, max_px=max_px)
        assert torch.equal(mask, expect(golden["hot__%s_mask" % name])), name
        assert torch.equal(rate, expect(golden["hot__%s_rate" % name])), name
        rate2 = dev(golden["hot__rate"])
        mask2 = E.get_hot_event_mask(rate2, idx, max_px=max_px)
        assert torch.equal(mask2, mask) and torch.equal(rate2, rate), name        # the same bits twice
    # four hot pixels: float32(0.8) at [0, 8] is not above max_rate = 0.8 (the comparison is made in float32)
    assert (golden["hot__all_mask"] == 0).sum() == 4 and golden["hot__all_mask"][0, 8] == 1
    assert (golden["hot__two_mask"] == 0).sum() == 2
    assert golden["hot__two_mask"][1, 2] == 0 and golden["hot__two_mask"][4, 7] == 0          # the tie, in flat-index order
    assert golden["hot__young_mask"].all() and np.array_equal(golden["hot__young_rate"], golden["hot__rate"])
    rate = dev(golden["hot__nan_in"])
    mask = E.get_hot_event_mask(rate, 10)
    assert torch.equal(mask, expect(golden["hot__nan_mask"]))
    assert np.array_equal(rate.cpu().numpy(), golden["hot__nan_rate"], equal_nan=True)
    strided = torch.zeros(6, 18, device="cuda")[:, ::2]
    strided.copy_(dev(golden["hot__rate"]))
    mask = E.get_hot_event_mask(strided, 10)
    assert torch.equal(mask, expect(golden["hot__all_mask"])) and torch.equal(strided, expect(golden["hot__all_rate"]))


def test_stack2cnt(golden, E):
    """Case 9: halves go to the even neighbour, negative halves too; the result stays on the device."""
    stack = dev(golden["cnt__stack"])
    keep = stack.clone()
    cnt = E.stack2cnt(stack)
    assert cnt.is_cuda and torch.equal(cnt, expect(golden["cnt__out"])) and torch.equal(stack, keep)
    assert torch.equal(cnt, E.stack2cnt(stack))
    assert cnt[0, :, 0, 0].tolist() == [4.0, 4.0]


def test_stack_polarity_is_events_to_stack(golden_dir, E):
    """Case 10: on the inputs of the existing events_to_stack fixture."""
    z = np.load(os.path.join(golden_dir, "events_to_stack.npz"))
    names = sorted({k.split(".")[0] for k in z.files})
    assert names
    for name in names:
        xs, ys, ts, ps = (dev(z["%s.%s" % (name, k)]) for k in ("xs", "ys", "ts", "ps"))
        B, ss = int(z[name + ".B"]), tuple(int(s) for s in z[name + ".size"])
        keep = [t.clone() for t in (xs, ys, ts, ps)]
        a = E.events_to_stack_polarity(xs, ys, ts, ps, B, sensor_size=ss)
        assert torch.equal(a, E.events_to_stack_polarity(xs, ys, ts, ps, B, sensor_size=ss)), name      # the same bits twice
        assert all(torch.equal(t, k) for t, k in zip((xs, ys, ts, ps), keep)), name
        assert torch.equal(a, E.events_to_stack(xs, ys, ts, ps, B, sensor_size=ss)), name
        assert torch.equal(a, expect(z[name + ".out"])), name


def test_the_capture_is_a_single_chain(E, uniform):
    """Every launch of a call goes onto the capturing stream, one after the other: the call leaves the capturing stream current
    and capturing, and the library source creates no stream and records no event of its own (tests/test_encodings_host.py reads
    the source for that), so the captured graph has no parallel branch."""
    v = uniform
    xs, ys, ts, ps = (dev(v[k]) for k in ("xs", "ys", "ts", "ps"))
    E.events_to_voxel_torch(xs, ys, ts, ps, v["B"], sensor_size=v["ss"])
    torch.cuda.synchronize()
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        main = torch.cuda.current_stream()
        E.events_to_voxel_torch(xs, ys, ts, ps, v["B"], sensor_size=v["ss"])
        assert torch.cuda.current_stream() == main and torch.cuda.is_current_stream_capturing()
    graph.replay()
    torch.cuda.synchronize()


def test_a_foreign_device_is_refused(E):
    z = torch.zeros(5, device="cuda")
    with pytest.raises(ValueError):
        E.events_to_voxel_torch(z, z, z, z, 4, device="cpu", sensor_size=(4, 4))
    with pytest.raises(ValueError):
        E.events_to_image_torch(z, z, z, device="cpu", sensor_size=(4, 4))
    assert E.events_to_voxel_torch(z, z, z, z, 4, device="cuda", sensor_size=(4, 4)).shape == (4, 4, 4)
