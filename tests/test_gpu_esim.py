"""The event simulator on the device (ebfi_amd.esim, csrc/esim.hip) against the float64 restatement of its law
(tests/esim_ref.py, itself held to hand-worked cases by test_esim_host.py): the same event count and the same bits in xs, ys, ts
and ps, on seeded byte frames with flat regions (exact ties in t), 0 <-> 255 jumps (the most crossings a step can have),
repeated frames and a stretch of dt = 1e-5 (the refractory rule); chunked and piecewise feeding (the state carry), BGR and
strided sources, the event-less sequence, repeatability, and generate_dataset/syn_gopro.py end to end.

Every shape is small: a single pixel, a ragged 5 x 7, 33 x 65 (pixels no multiple of the 64-lane wave or the 256-thread
workgroup, nine workgroups) and 2 x 130 (a row spanning three waves)."""
import os
import random

import numpy as np
import pytest
import torch

import esim_ref as R
from test_esim_host import TIE_FRAMES, TIE_PARAMS, TIE_TIMES, load_script

PARAMS = dict(Cp=0.31, Cn=0.23, refractory_period=1e-4, log_eps=1e-3, use_log=True)
SIZES = [(1, 1), (5, 7), (33, 65), (2, 130)]

_cache = {}


def make_sequence(m, H, W, seed=0):
    """uint8 [m, H, W] and m times.  Columns [0, W/3): one value per frame (ties in t across pixels); a checkerboard of the
    middle third flips 0 <-> 255 every frame; the rest is noise; frame 3 repeats frame 2; intervals 4..6 last 1e-5 s."""
    g = np.random.RandomState(1000 * seed + 100 * m + H * W)
    frames = g.randint(0, 256, size=(m, H, W)).astype(np.uint8)
    a, b = W // 3, 2 * W // 3
    yy, xx = np.mgrid[0:H, 0:W]
    board = ((yy + xx) % 2 == 0) & (xx >= a) & (xx < b)
    for k in range(m):
        frames[k, :, :a] = (37 * k * k + 11) % 256 if k % 4 else 255 * ((k // 4) % 2)
        frames[k][board] = 255 * (k % 2)
    if m > 3:
        frames[3] = frames[2]
    dts = [1e-5 if 4 <= k <= 6 else 1.0 / 240 for k in range(1, m)]
    times = np.concatenate([[0.0125], 0.0125 + np.cumsum(dts)]) if m > 1 else np.array([0.0125])
    return frames, times


def case(m, H, W, **over):
    """(frames, times, restated events) of a sequence, made once per session and never modified."""
    params = dict(PARAMS, **over)
    key = (m, H, W, tuple(sorted(params.items())))
    if key not in _cache:
        frames, times = make_sequence(m, H, W)
        frames.setflags(write=False)
        _cache[key] = (frames, times, R.simulate(frames, times, **params))
    return _cache[key]


def simulator(**over):
    from ebfi_amd.esim import EventSimulator
    return EventSimulator(**dict(PARAMS, **over))


def host(events):
    return tuple(v.cpu().numpy() for v in events)


def assert_same(got, want, what=""):
    """event count, dtypes and every bit of the four arrays"""
    for g, w, name, dt in zip(got, want, ("xs", "ys", "ts", "ps"), (np.int16, np.int16, np.float64, np.int8)):
        assert g.dtype == dt and w.dtype == dt, (what, name, g.dtype)
        assert g.shape == w.shape, (what, name, "event count", g.shape, w.shape)
        if name == "ts":
            assert np.array_equal(g.view(np.int64), w.view(np.int64)), (what, name, int((g != w).sum()), np.abs(g - w).max())
        else:
            assert np.array_equal(g, w), (what, name, int((g != w).sum()))


@pytest.mark.gpu
@pytest.mark.parametrize("m", [2, 9])
@pytest.mark.parametrize("H,W", SIZES)
def test_device_equals_restatement(H, W, m):
    frames, times, want = case(m, H, W)
    events = simulator().generate(torch.from_numpy(frames.copy()).cuda(), times)
    assert all(v.is_cuda for v in events)
    assert [v.dtype for v in events] == [torch.int16, torch.int16, torch.float64, torch.int8]
    got = host(events)
    print("esim %dx%d m=%d: %d events (restated %d)" % (H, W, m, len(got[2]), len(want[2])))
    assert len(want[2]) > 0 or (H, W, m) == (1, 1, 2)
    assert_same(got, want, (H, W, m))
    assert np.all(np.diff(got[2]) >= 0)
    if m == 9 and H * W > 1:
        assert (np.diff(got[2]) == 0).sum() > 0          # the flat columns do tie in t
        assert set(got[3].tolist()) == {-1, 1}


@pytest.mark.gpu
def test_linear_levels_and_other_thresholds():
    over = dict(Cp=0.2, Cn=0.5, use_log=False, refractory_period=0.0)
    frames, times, want = case(9, 5, 7, **over)
    assert_same(host(simulator(**over).generate(torch.from_numpy(frames.copy()).cuda(), times)), want)


@pytest.mark.gpu
@pytest.mark.parametrize("chunk", [1, 3, 8])
def test_chunking_carries_the_state(chunk):
    frames, times, want = case(9, 33, 65)
    dev = torch.from_numpy(frames.copy()).cuda()
    whole = host(simulator().generate(dev, times, chunk=16))
    got = host(simulator().generate(dev, times, chunk=chunk))
    assert_same(got, whole, chunk)
    assert_same(got, want, chunk)


@pytest.mark.gpu
def test_piecewise_feeding_equals_one_call():
    frames, times, want = case(9, 33, 65)
    dev = torch.from_numpy(frames.copy()).cuda()
    sim = simulator()
    a = host(sim.generate(dev[:4], times[:4]))
    b = host(sim.generate(dev[4:], times[4:], chunk=2))
    assert_same(tuple(np.concatenate([u, v]) for u, v in zip(a, b)), want)
    # a single first frame only initialises; reset() starts over
    sim.reset()
    assert all(v.numel() == 0 for v in sim.generate(dev[:1], times[:1]))
    assert_same(host(sim.generate(dev[1:], times[1:])), want)
    # parameters set after the first piece hold from the next frame on, the state is kept
    sim.reset()
    sim.setParameters(0.5, 0.5, 1e-4, 1e-3, True)
    sim.generate(dev[:1], times[:1])
    sim.setParameters(**PARAMS)
    assert_same(host(sim.generate(dev[1:], times[1:])), want)


@pytest.mark.gpu
@pytest.mark.parametrize("chunk", [1, 16])
def test_ties_across_a_frame_time_go_by_pixel(chunk):
    """test_esim_host.py's tie: an interval-1 event of pixel (0, 0) rounds onto the frame time at which pixel (0, 1) has an
    interval-0 event.  The law orders them by x; a sort on t alone over the [interval][y][x] layout would not."""
    from ebfi_amd.esim import EventSimulator
    want = R.simulate(TIE_FRAMES, TIE_TIMES, **TIE_PARAMS)
    assert want[2].tolist()[3:5] == [2.0, 2.0] and want[0].tolist()[3:5] == [0, 1]
    # tiled so that the tie also spans workgroups: 300 copies of the pair along x
    frames = np.tile(TIE_FRAMES, (1, 1, 300))
    tiled = R.simulate(frames, TIE_TIMES, **TIE_PARAMS)
    sim = EventSimulator(**TIE_PARAMS)
    assert_same(host(sim.generate(torch.from_numpy(TIE_FRAMES).cuda(), TIE_TIMES, chunk=chunk)), want, chunk)
    sim.reset()
    assert_same(host(sim.generate(torch.from_numpy(frames).cuda(), TIE_TIMES, chunk=chunk)), tiled, chunk)


@pytest.mark.gpu
def test_table_change_needs_reset():
    frames, times, want = case(2, 5, 7)
    dev = torch.from_numpy(frames.copy()).cuda()
    sim = simulator()
    sim.generate(dev[:1], times[:1])
    with pytest.raises(ValueError):
        sim.setParameters(0.31, 0.23, 1e-4, 1e-3, False)
    with pytest.raises(ValueError):
        sim.setParameters(0.31, 0.23, 1e-4, 2e-3, True)
    assert_same(host(sim.generate(dev[1:], times[1:])), want)          # the refused calls changed nothing
    sim.reset()
    sim.setParameters(0.31, 0.23, 1e-4, 1e-3, False)


@pytest.mark.gpu
def test_from_bgr_equals_mono_of_the_restated_gray():
    g = np.random.RandomState(3)
    bgr = g.randint(0, 256, size=(5, 6, 67, 3)).astype(np.uint8)
    bgr[2, :, :20] = (255, 0, 0)
    bgr[3, :, :20] = (0, 0, 255)
    times = 0.5 + np.arange(5) / 240.0
    gray = R.gray_from_bgr(bgr)
    want = R.simulate(gray, times, **PARAMS)
    from_bgr = host(simulator().generate(torch.from_numpy(bgr).cuda(), times, chunk=2))
    mono = host(simulator().generate(torch.from_numpy(gray).cuda(), times))
    assert len(want[2]) > 0
    assert_same(from_bgr, mono)
    assert_same(from_bgr, want)


@pytest.mark.gpu
def test_strided_source_equals_contiguous():
    frames, times, want = case(9, 33, 65)
    m, H, W = frames.shape
    big = torch.full((m + 1, H + 2, W + 13), 77, dtype=torch.uint8, device="cuda")
    view = big[1:, 1:1 + H, 5:5 + W]
    view.copy_(torch.from_numpy(frames.copy()))
    before = big.clone()
    assert view.stride() == ((H + 2) * (W + 13), W + 13, 1) and not view.is_contiguous()
    assert_same(host(simulator().generate(view, times, chunk=3)), want)
    assert torch.equal(big, before)


@pytest.mark.gpu
def test_equal_frames_give_empty_tensors():
    frames = torch.full((4, 5, 7), 93, dtype=torch.uint8, device="cuda")
    events = simulator().generate(frames, [0.1, 0.2, 0.3, 0.4], chunk=2)
    assert [tuple(v.shape) for v in events] == [(0,)] * 4
    assert [v.dtype for v in events] == [torch.int16, torch.int16, torch.float64, torch.int8] and all(v.is_cuda for v in events)
    assert all(v.numel() == 0 for v in simulator().generate(frames[:0], []))


@pytest.mark.gpu
def test_two_runs_are_bit_identical():
    frames, times, _ = case(9, 33, 65)
    dev = torch.from_numpy(frames.copy()).cuda()
    a = simulator().generate(dev, times, chunk=3)
    b = simulator().generate(dev, times, chunk=3)
    assert all(torch.equal(u, v) for u, v in zip(a, b))
    assert np.array_equal(dev.cpu().numpy(), frames)          # the frames are read, never written


@pytest.mark.gpu
def test_times_must_follow_what_was_fed():
    from ebfi_amd._native import EbfiNativeError
    frames, times, _ = case(2, 5, 7)
    sim = simulator()
    dev = torch.from_numpy(frames.copy()).cuda()
    sim.generate(dev, times)
    with pytest.raises(EbfiNativeError):
        sim.generate(dev, times)          # not later than the frames already consumed
    with pytest.raises(ValueError):
        sim.generate(dev[:, :4], times + 1.0)          # another frame size without reset()


@pytest.mark.gpu
def test_script_settles_a_tie_between_two_uploads(tmp_path):
    """The tie of test_ties_across_a_frame_time_go_by_pixel with the frame time falling between two uploaded chunks."""
    from PIL import Image
    from ebfi_amd.esim import EventSimulator
    S = load_script()
    paths = []
    for k, frame in enumerate(TIE_FRAMES):
        paths.append(str(tmp_path / ("%05d.png" % k)))
        Image.fromarray(frame).save(paths[-1])
    got = S.simulate_sequence(EventSimulator(**TIE_PARAMS), paths, TIE_TIMES, 2, torch.device("cuda", 0))
    assert_same(got, R.simulate(TIE_FRAMES, TIE_TIMES, **TIE_PARAMS))


@pytest.mark.gpu
def test_script_end_to_end(tmp_path):
    from PIL import Image
    from ebfi_amd import clipdata
    S = load_script()
    g = np.random.RandomState(8)
    H, W, n = 16, 24, 4
    root, out = tmp_path / "data", tmp_path / "clips"
    times = [k / 240.0 for k in range(n)]          # (the stored frames' own times: event_idx is then not trivial)
    stored = {}
    for name, with_mono in (("seq_a", True), ("seq_b", False)):
        rgb = g.randint(0, 256, size=(n, H, W, 3)).astype(np.uint8)
        rgb[:, :, :8] = (np.arange(n) % 2 * 255).astype(np.uint8)[:, None, None, None]
        mono = g.randint(0, 256, size=(n, H, W)).astype(np.uint8)
        os.makedirs(str(root / name / "rgb"))
        for k in range(n):
            Image.fromarray(rgb[k]).save(str(root / name / "rgb" / ("%05d.png" % k)))
        if with_mono:
            os.makedirs(str(root / name / "mono"))
            for k in range(n):
                Image.fromarray(mono[k]).save(str(root / name / "mono" / ("%05d.png" % k)))
        with open(str(root / name / "timestamps.txt"), "w") as f:
            f.writelines("%r\n" % t for t in times)
        bgr = np.ascontiguousarray(rgb[..., ::-1])
        stored[name] = (bgr, mono if with_mono else R.gray_from_bgr(bgr))

    assert S.main(["--root_data_path", str(root), "--path_to_h5", str(out), "--seed", "4"], chunk=3) == 0          # (two chunks)

    rng = random.Random(4)
    ct = open(str(out / "config" / "ct.txt")).read().split("\n")
    assert open(str(out / "config" / "config.txt")).read().startswith("Cp_init: 0.1 \nCn_init: 0.1 \nrefractory_period: 0.0001 \n")
    for i, name in enumerate(("seq_a", "seq_b")):
        Cp, Cn = S.draw_thresholds(rng)
        assert ct[i] == "%s:Cp=%s, Cn=%s" % (str(root / name), Cp, Cn)
        bgr, gray = stored[name]
        clip = clipdata.open_clip(str(out / (name + ".npz")))
        assert clip.num_imgs == n and clip.resolution == (H, W) and np.array_equal(clip.images, bgr)
        want = R.simulate(gray, times, Cp, Cn, 1e-4, 1e-3, True)
        assert len(want[2]) > 100
        assert_same((clip.xs, clip.ys, clip.ts, clip.ps), want, name)
        assert np.all(np.diff(clip.ts) >= 0)
        E = len(clip.ts)
        rule = [min(E - 1, max(0, int(np.searchsorted(clip.ts, k / 240.0, "left")) - 1)) for k in range(n)]
        assert clip.event_idx.dtype == np.int64 and clip.event_idx.tolist() == rule
        # the clip reader slices it as it slices every clip
        xs, ys, ts, ps = clip.events(0, n - 1)
        assert len(ts) == rule[-1] - rule[0] and rule[-1] > rule[1] > 0
