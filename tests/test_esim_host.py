"""Host half of the event simulator (no GPU): the float64 restatement of the law (tests/esim_ref.py) on hand-worked cases with the
events written out, the event_idx rule and the threshold draws of generate_dataset/syn_gopro.py, its flags, the new C symbols,
and the argument refusals of the entry points, none of which touches a GPU."""
import ctypes
import importlib.util
import math
import os
import random

import numpy as np
import pytest
import torch

from ebfi_amd import _native as N

import esim_ref as R

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SCRIPT = os.path.join(ROOT, "ebfi-be_amd", "generate_dataset", "syn_gopro.py")
ESIM_SYMBOLS = ["ebfi_esim_loop_bound", "ebfi_esim_init", "ebfi_esim_count", "ebfi_esim_emit"]


def load_script():
    spec = importlib.util.spec_from_file_location("syn_gopro_under_test", SCRIPT)
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod


def one_pixel(values, times, Cp, Cn, refractory, log_eps=1e-3, use_log=False):
    """events [(t, pol), ...] of a 1 x 1 sequence of bytes"""
    frames = np.array(values, dtype=np.uint8).reshape(-1, 1, 1)
    xs, ys, ts, ps = R.simulate(frames, times, Cp, Cn, refractory, log_eps, use_log)
    assert xs.dtype == np.int16 and ys.dtype == np.int16 and ts.dtype == np.float64 and ps.dtype == np.int8
    assert not xs.any() and not ys.any()
    return list(zip(ts.tolist(), ps.tolist()))


# ------------------------------------------------------------------------------------------------ the restatement, by hand
def test_rising_step_crosses_twice():
    # levels 0 -> 128/255 = 0.50196..., C = 0.2: crossings at 0.2 and 0.4 (0.6000000000000001 is past the new level)
    L = 128 / 255.0
    want = [(1.0 + (0.2 * 1.0) / L, 1), (1.0 + ((0.2 + 0.2) * 1.0) / L, 1)]
    assert want == [(1.3984375, 1), (1.796875, 1)]
    assert one_pixel([0, 128], [1.0, 2.0], 0.2, 0.3, 1e-4) == want


def test_reversal_crosses_from_ref_not_from_it():
    # 0 -> 76/255 = 0.298...: one crossing at 0.2, ref = 0.2 while it = 0.298.  Back to 0: the falling crossing is ref - Cn = 0.0
    # (from `it` it would be 0.098), reached exactly at the frame time: ((0.0 - it) * 1.0) / (0.0 - it) = 1.0
    L = 76 / 255.0
    want = [(1.0 + (0.2 * 1.0) / L, 1), (2.0 + ((0.0 - L) * 1.0) / (0.0 - L), -1)]
    assert want[1] == (3.0, -1)
    assert one_pixel([0, 76, 0], [1.0, 2.0, 3.0], 0.2, 0.2, 1e-4) == want
    # Cn != Cp: falling crossings step by Cn from ref = 0.2: 0.2 - 0.15 = 0.05 is crossed, -0.1 is not
    cross = 0.2 - 0.15
    assert one_pixel([0, 76, 0], [1.0, 2.0, 3.0], 0.2, 0.15, 1e-4)[1:] == [(2.0 + ((cross - L) * 1.0) / (0.0 - L), -1)]


def test_equal_frames_and_sub_tolerance_steps_emit_nothing():
    assert one_pixel([7, 7, 7, 7], [0.5, 1.0, 1.5, 2.0], 0.2, 0.2, 1e-4) == []
    assert one_pixel([200] * 3, [1.0, 2.0, 3.0], 0.2, 0.2, 1e-4, use_log=True) == []
    # a step of 8e-7 <= 1e-6 that WOULD cross ref + C = 0.5000005 is skipped, and `it` still moves
    s = R.PixelState(0.5)
    s.ref = 0.3000005
    assert R.step_pixel(s, 0.5000008, 1.0, 2.0, 0.2, 0.2, 1e-4) == []
    assert (s.it, s.ref, s.last_t) == (0.5000008, 0.3000005, 0.0)
    # just above the tolerance the same crossing is taken
    s = R.PixelState(0.5)
    s.ref = 0.3000005
    ev = R.step_pixel(s, 0.5000012, 1.0, 2.0, 0.2, 0.2, 1e-4)
    cross = 0.3000005 + 0.2
    assert ev == [(1.0 + ((cross - 0.5) * 1.0) / (0.5000012 - 0.5), 1)] and s.ref == cross
    # byte frames whose levels differ by less than the tolerance: log(1e4 + v / 255) moves by 3.9e-7 per step
    assert one_pixel([0, 1, 2, 1, 0], [1, 2, 3, 4, 5], 1e-3, 1e-3, 0.0, log_eps=1e4, use_log=True) == []


def test_refractory_suppression_consumes_the_crossing():
    # dt = 1e-5 per frame, refractory 1e-4.  0 -> 64: crossing 0.2, emitted (first event).  64 -> 128: crossing 0.4 comes 1.2e-5 after
    # it: NOT emitted, but ref moves to 0.4.  A second later 128 -> 192 (0.7529): the next crossing is 0.4 + 0.2, emitted; had ref
    # stayed at 0.2, the candidate 0.4 would lie below `it` and nothing would be emitted.
    L1, L2, L3 = 64 / 255.0, 128 / 255.0, 192 / 255.0
    t0, t1, t2, t3 = 1.0, 1.0 + 1e-5, 1.0 + 2e-5, 2.0 + 2e-5
    first = t0 + (0.2 * (t1 - t0)) / L1
    suppressed = t1 + (((0.2 + 0.2) - L1) * (t2 - t1)) / (L2 - L1)
    assert 0 < suppressed - first < 1e-4
    third = t2 + ((((0.2 + 0.2) + 0.2) - L2) * (t3 - t2)) / (L3 - L2)
    got = one_pixel([0, 64, 128, 192], [t0, t1, t2, t3], 0.2, 0.2, 1e-4)
    assert got == [(first, 1), (third, 1)]
    assert one_pixel([0, 64, 128, 192], [t0, t1, t2, t3], 0.2, 0.2, 0.0) == [(first, 1), (suppressed, 1), (third, 1)]


def test_last_t_zero_means_none_yet():
    # the first event is emitted however early it is: t = 0.5 with a refractory period of 10 s
    assert one_pixel([0, 102], [0.0, 1.0], 0.2, 0.2, 10.0) == [(0.0 + (0.2 * 1.0) / (102 / 255.0), 1)]
    assert (0.2 * 1.0) / (102 / 255.0) == 0.5
    # an event AT t = 0.0 leaves last_t == 0.0, so the next one is emitted too: the sentinel, as stated
    assert 0.2 + 0.2 == 102 / 255.0
    assert one_pixel([0, 102], [-1.0, 1.0], 0.2, 0.2, 10.0) == [(0.0, 1), (1.0, 1)]
    # ... while after an event at t = 0.25 the same second crossing is suppressed
    assert one_pixel([0, 102], [-0.75, 1.25], 0.2, 0.2, 10.0) == [(0.25, 1)]


def test_linear_and_log_levels():
    assert np.array_equal(R.level_table(1e-3, False), np.arange(256) / 255.0)
    assert R.level_table(1e-3, True)[0] == math.log(1e-3) and R.level_table(1e-3, True)[255] == math.log(1e-3 + 1.0)
    # 0 -> 255 in log levels with C = 0.3: floor((log 1.001 - log 0.001) / 0.3) = 23 crossings, evenly spaced in level
    lo, hi = math.log(1e-3), math.log(1.001)
    got = one_pixel([0, 255], [1.0, 2.0], 0.3, 0.3, 0.0, use_log=True)
    assert len(got) == 23 == int((hi - lo) / 0.3)
    cross, want = lo, []
    for _ in range(23):
        cross = cross + 0.3
        want.append((1.0 + ((cross - lo) * 1.0) / (hi - lo), 1))
    assert got == want
    # and down again with Cn = 0.5: 13 falling crossings from ref = lo + 23 * 0.3
    down = one_pixel([0, 255, 0], [1.0, 2.0, 3.0], 0.3, 0.5, 0.0, use_log=True)[23:]
    assert [p for _, p in down] == [-1] * 13
    # linear levels, C = 0.25: four crossings, the last exactly at the new level and the frame time
    assert one_pixel([0, 255], [1.0, 2.0], 0.25, 0.25, 0.0) == [(1.25, 1), (1.5, 1), (1.75, 1), (2.0, 1)]


def test_output_order_is_t_y_x_emission():
    # two pixels with identical histories tie in t: the order is by y, then x
    frames = np.zeros((2, 2, 2), dtype=np.uint8)
    frames[1] = 255
    xs, ys, ts, ps = R.simulate(frames, [1.0, 2.0], 0.25, 0.25, 0.0, 1e-3, False)
    assert ts.tolist() == [1.25] * 4 + [1.5] * 4 + [1.75] * 4 + [2.0] * 4
    assert ys.tolist() == [0, 0, 1, 1] * 4 and xs.tolist() == [0, 1, 0, 1] * 4 and ps.tolist() == [1] * 16
    # piecewise feeding restates the same events
    sim = R.Simulator(0.25, 0.25, 0.0, 1e-3, False)
    a = sim.generate(frames[:1], [1.0])
    b = sim.generate(frames[1:], [2.0])
    assert len(a[0]) == 0 and all(np.array_equal(u, v) for u, v in zip(b, (xs, ys, ts, ps)))


def test_gray_from_bgr_fixed_point():
    bgr = np.array([[0, 0, 0], [255, 255, 255], [255, 0, 0], [0, 255, 0], [0, 0, 255], [10, 20, 30]], dtype=np.uint8)
    # B = 255 -> (1868 * 255 + 8192) >> 14 = 29; G -> 150; R -> 76; (10, 20, 30) -> (4899 * 30 + 9617 * 20 + 1868 * 10 + 8192) >> 14
    assert R.gray_from_bgr(bgr).tolist() == [0, 255, 29, 150, 76, (146970 + 192340 + 18680 + 8192) >> 14]
    assert 4899 + 9617 + 1868 == 1 << 14


# ------------------------------------------------------------------------------------------------ the script's host logic
def test_event_idx_rule():
    S = load_script()
    ts = np.array([0.1, 0.2, 0.2, 0.2, 0.35, 0.5])
    frame_times = [0.0, 0.05, 0.1, 0.2, 0.21, 0.5, 0.6, 7.0]   # before the first event, on events, on a run of ties, after the last
    want = [min(len(ts) - 1, max(0, int(np.searchsorted(ts, t, "left")) - 1)) for t in frame_times]
    assert want == [0, 0, 0, 0, 3, 4, 5, 5]
    got = S.event_indices(ts, frame_times)
    assert got.dtype == np.int64 and got.tolist() == want
    assert R.event_indices(ts, frame_times).tolist() == want
    empty = S.event_indices(np.zeros(0), frame_times)
    assert empty.dtype == np.int64 and empty.tolist() == [0] * len(frame_times)
    assert S.event_indices(np.array([0.3]), frame_times).tolist() == [0] * len(frame_times)
    assert S.event_indices(ts, []).shape == (0,)


def test_threshold_draw_sequence():
    S = load_script()
    rng, mine = random.Random(5), random.Random(5)
    for _ in range(64):
        Cp = mine.uniform(0.2, 0.5)
        Cn = mine.gauss(1, 0.1) * Cp
        want = (min(max(Cp, 0.2), 0.5), min(max(Cn, 0.2), 0.5))
        got = S.draw_thresholds(rng)
        assert got == want and 0.2 <= got[0] <= 0.5 and 0.2 <= got[1] <= 0.5
    # the clamp is reached within a few hundred draws from seed 0 (Cn = gauss * Cp leaves [0.2, 0.5] near its ends)
    rng = random.Random(0)
    draws = [S.draw_thresholds(rng) for _ in range(400)]
    assert any(cn in (0.2, 0.5) for _, cn in draws)
    # the same seed gives the same sequence; another seed another
    assert [S.draw_thresholds(r) for r in [random.Random(0)] * 3] == draws[:3]
    assert S.draw_thresholds(random.Random(1)) != draws[0]


def test_config_block_and_files(tmp_path):
    S = load_script()
    assert S.settings == {"Cp_init": 0.1, "Cn_init": 0.1, "refractory_period": 1e-4, "log_eps": 1e-3, "use_log": True,
                          "CT_range": [0.2, 0.5], "max_CT": 0.5, "min_CT": 0.2, "mu": 1, "sigma": 0.1, "fps": 240}
    S.write_settings(str(tmp_path / "config.txt"))
    assert open(str(tmp_path / "config.txt")).read() == (
        "Cp_init: 0.1 \nCn_init: 0.1 \nrefractory_period: 0.0001 \nlog_eps: 0.001 \nuse_log: True \nCT_range: [0.2, 0.5] \n"
        "max_CT: 0.5 \nmin_CT: 0.2 \nmu: 1 \nsigma: 0.1 \nfps: 240 \n")
    records = [S.threshold_record("/data/a", (0.3, 0.25)), S.threshold_record("b", (0.27081442692123037, 0.2))]
    S.write_records(records, str(tmp_path / "ct.txt"))
    assert open(str(tmp_path / "ct.txt")).read() == "/data/a:Cp=0.3, Cn=0.25\nb:Cp=0.27081442692123037, Cn=0.2\n"


# Two pixels that tie across a frame time (linear levels, C = 0.2, times 1, 2, 2.5).  Pixel (0, 1): 0 -> 102 crosses 0.4 exactly at
# the frame time 2.0, in interval 0.  Pixel (0, 0): 0 -> 153 crosses 0.2 and 0.4 and leaves ref = 0.4 under it = 0.6; then
# 153 -> 255 crosses 0.6000000000000001, one ulp above `it`: ((cross - it) * 0.5) / 0.4 = 1.4e-16 vanishes against 2.0, so the
# event of interval 1 is AT 2.0 as well.  The law orders the tie by x: pixel (0, 0) of interval 1 before pixel (0, 1) of interval 0.
TIE_FRAMES = np.array([[[0, 0]], [[153, 102]], [[255, 102]]], dtype=np.uint8)
TIE_TIMES = [1.0, 2.0, 2.5]
TIE_PARAMS = dict(Cp=0.2, Cn=0.2, refractory_period=1e-4, log_eps=1e-3, use_log=False)


def test_tie_across_a_frame_time_goes_by_pixel():
    xs, ys, ts, ps = R.simulate(TIE_FRAMES, TIE_TIMES, **TIE_PARAMS)
    it = 153 / 255.0
    assert (0.2 + 0.2) + 0.2 == 0.6000000000000001 > it and 2.0 + ((0.6000000000000001 - it) * 0.5) / (1.0 - it) == 2.0
    assert ts.tolist() == [1.0 + (0.2 * 1.0) / it, 1.5, 1.0 + (0.4 * 1.0) / it, 2.0, 2.0, 2.25, 2.5]
    assert xs.tolist() == [0, 1, 0, 0, 1, 0, 0] and not ys.any() and ps.tolist() == [1] * 7


def test_settle_boundary_restores_the_order_between_pieces():
    S = load_script()
    whole = R.simulate(TIE_FRAMES, TIE_TIMES, **TIE_PARAMS)
    sim = R.Simulator(**TIE_PARAMS)
    a = sim.generate(TIE_FRAMES[:2], TIE_TIMES[:2])
    b = sim.generate(TIE_FRAMES[2:], TIE_TIMES[2:])
    naive = [np.concatenate([u, v]) for u, v in zip(a, b)]
    assert not np.array_equal(naive[0], whole[0])          # piece order puts pixel (0, 1) first at t = 2.0
    a2, b2 = S.settle_boundary(a, b)
    for i, dt in enumerate((np.int16, np.int16, np.float64, np.int8)):
        joined = np.concatenate([a2[i], b2[i]])
        assert joined.dtype == dt and np.array_equal(joined, whole[i]), i
    assert len(a2[2]) == len(a[2]) and len(b2[2]) == len(b[2])
    # nothing to do: no overlap, or an empty piece
    c, d = S.settle_boundary(a, tuple(v[1:] for v in b))
    assert all(u is v for u, v in zip(c, a))
    empty = tuple(v[:0] for v in a)
    assert S.settle_boundary(empty, b)[1] is b and S.settle_boundary(a, empty)[0] is a


def test_script_flags():
    S = load_script()
    f = S.get_flags([])
    assert (f.root_data_path, f.path_to_h5, f.seed) == ("/path/to/data", "/path/to/output", 0)
    f = S.get_flags(["--root_data_path", "in", "--path_to_h5", "out", "--seed", "11"])
    assert (f.root_data_path, f.path_to_h5, f.seed) == ("in", "out", 11)
    with pytest.raises(SystemExit):
        S.get_flags(["--seed", "x"])


# ------------------------------------------------------------------------------------------------ the C ABI, GPU untouched
@pytest.fixture(scope="module")
def lib():
    if not os.path.exists(N.LIB_PATH):
        N.build()
    return N.lib()


def test_symbols_declared_bound_exported(lib):
    declared = N.declared_symbols()
    h = ctypes.CDLL(N.LIB_PATH)
    for name in ESIM_SYMBOLS:
        assert name in declared and name in N.SIGNATURES and hasattr(h, name), name
    header = open(N.HEADER).read()
    assert "#define EBFI_ABI_VERSION 14" in header and "#define EBFI_ESIM_MAX_CHUNK 128" in header
    assert lib.ebfi_abi_version() == 14 == N.ABI_VERSION
    from ebfi_amd import esim
    assert esim.MAX_CHUNK == 128


def f64(values):
    return (ctypes.c_double * len(values))(*values)


def test_loop_bound_is_host_arithmetic(lib):
    from ebfi_amd.esim import level_table
    L = level_table(1e-3, True)
    assert np.array_equal(L, R.level_table(1e-3, True))
    assert lib.ebfi_esim_loop_bound(f64(L.tolist()), 0.3, 0.5) == math.ceil((L.max() - L.min()) / 0.3) + 1 == 25
    assert lib.ebfi_esim_loop_bound(f64(L.tolist()), 0.5, 0.2) == math.ceil((L.max() - L.min()) / 0.2) + 1
    lin = level_table(1e-3, False)
    assert lib.ebfi_esim_loop_bound(f64(lin.tolist()), 0.25, 0.25) == 5
    assert lib.ebfi_esim_loop_bound(f64(lin.tolist()), 1e-3, 1.0) == math.ceil(1.0 / 1e-3) + 1
    assert lib.ebfi_esim_loop_bound(f64(lin.tolist()), 0.9e-3, 1.0) == -1
    assert lib.ebfi_esim_loop_bound(f64(lin.tolist()), 0.2, float("nan")) == -1
    assert lib.ebfi_esim_loop_bound(f64(lin.tolist()), float("inf"), 0.2) == -1
    with np.errstate(all="ignore"):
        assert lib.ebfi_esim_loop_bound(f64(level_table(0.0, True).tolist()), 0.2, 0.2) == -1      # log(0) = -inf
        assert lib.ebfi_esim_loop_bound(f64(level_table(-0.5, True).tolist()), 0.2, 0.2) == -1     # log of a negative = nan
    assert lib.ebfi_esim_loop_bound(None, 0.2, 0.2) == -1


def test_argument_refusals_do_not_touch_the_gpu(lib):
    """Every pointer that would be a device pointer is the address 8: a call that got past its checks would fault."""
    fake = ctypes.c_void_p(8)
    L = f64(R.level_table(1e-3, True).tolist())
    strides = (ctypes.c_int64 * 2)(24, 6)
    times = f64([0.0, 0.1, 0.2])

    def count(frames=fake, st=strides, n=2, H=4, W=6, t=times, lv=L, Cp=0.3, Cn=0.3, refr=1e-4, state=fake, counts=fake):
        return lib.ebfi_esim_count(frames, st, 0, n, H, W, t, lv, Cp, Cn, refr, state, counts, None)

    def emit(frames=fake, st=strides, n=2, H=4, W=6, t=times, lv=L, Cp=0.3, Cn=0.3, refr=1e-4, state=fake, offsets=fake, cap=5,
             xs=fake, ys=fake, ts=fake, ps=fake):
        return lib.ebfi_esim_emit(frames, st, 0, n, H, W, t, lv, Cp, Cn, refr, state, offsets, cap, xs, ys, ts, ps, None)

    for call in (count, emit):
        assert call(Cp=0.9e-3) == -1 and b"1e-3" in lib.ebfi_last_error()
        assert call(Cn=0.0) == -1
        assert call(Cp=float("nan")) == -1 and call(Cn=float("inf")) == -1 and call(refr=float("nan")) == -1
        assert call(t=f64([0.0, 0.1, 0.1])) == -1 and b"increase" in lib.ebfi_last_error()
        assert call(t=f64([0.0, 0.2, 0.1])) == -1
        assert call(t=f64([0.0, float("nan"), 0.1])) == -1
        assert call(frames=None) == -1 and b"null" in lib.ebfi_last_error()
        assert call(state=None) == -1 and call(lv=None) == -1 and call(t=None) == -1 and call(st=None) == -1
        assert call(W=32768) == -1 and b"32767" in lib.ebfi_last_error()
        assert call(H=32768) == -1 and call(W=0) == -1 and call(H=0) == -1
        assert call(n=-1) == -1 and call(n=129) == -1
        assert call(st=(ctypes.c_int64 * 2)(-24, 6)) == -1
        with np.errstate(all="ignore"):
            assert call(lv=f64(R.level_table(0.0, True).tolist())) == -1
        assert call(n=0, t=f64([0.0])) == 0          # no-op: nothing is launched
    assert count(counts=None) == -1 and emit(offsets=None) == -1 and emit(ts=None) == -1 and emit(cap=-1) == -1

    def init(frame=fake, rs=6, H=4, W=6, lv=L, state=fake):
        return lib.ebfi_esim_init(frame, rs, 0, H, W, lv, state, None)

    assert init(frame=None) == -1 and init(state=None) == -1 and init(lv=None) == -1
    assert init(W=32768) == -1 and init(H=0) == -1 and init(rs=-1) == -1
    with np.errstate(all="ignore"):
        assert init(lv=f64(R.level_table(-1.0, True).tolist())) == -1


def test_wrapper_refuses_bad_parameters_and_cpu_tensors():
    from ebfi_amd.esim import EventSimulator
    for bad in [(0.9e-3, 0.2, 1e-4, 1e-3, True), (0.2, 0.0, 1e-4, 1e-3, True), (0.2, 0.2, 1e-4, 0.0, True),
                (0.2, 0.2, 1e-4, -1.0, True), (float("nan"), 0.2, 1e-4, 1e-3, True), (0.2, 0.2, float("inf"), 1e-3, False),
                (0.2, 0.2, -1e-4, 1e-3, True)]:
        with pytest.raises(ValueError):
            EventSimulator(*bad)
    sim = EventSimulator(0.2, 0.2, 1e-4, 0.0, False)          # log_eps is unused without use_log
    assert np.array_equal(sim.levels, np.arange(256) / 255.0)
    with pytest.raises(ValueError):
        sim.setParameters(0.2, 0.2, 1e-4, 0.0, True)
    with pytest.raises(NotImplementedError):
        sim.generate(torch.zeros((2, 4, 4), dtype=torch.uint8), [0.0, 0.1])
