"""Host half of the device noise law of the clip loaders (no GPU): the generator against its published known answer, the erfc
table, the law's class frequencies against the closed form -- beside the reference's own draw (clipdata.draw_noise) on the same
inputs --, independence across adjacent seeds and neighbouring cells, and the plumbing: config, flags, what `prepare` leaves out
in device mode, the two entry points' declaration, binding and argument refusals."""
import argparse
import ctypes
import math

import numpy as np
import pytest
import torch

import eventaug_ref as R
from ebfi_amd import _native as N
from ebfi_amd import clipdata, eventaug

SHAPE = (16, 2, 256, 256)
CELLS = 16 * 2 * 256 * 256
CASES = [(1.0, 0.05), (2.5, 0.05), (1.0, 1.0), (2.0, 0.001)]
SEEDS = [3, 126, 2 ** 32 + 8]
SIGMAS = 5.0


# ------------------------------------------------------------------------------------------------ generator and table
def test_philox_known_answers():
    """Random123's kat_vectors for philox4x32-10: the all-zero, the all-ones and the pi-digits counter / key."""
    hexs = lambda w: ["%08x" % int(v) for v in np.asarray(w).reshape(-1)]
    assert hexs(R.philox4x32_10((0, 0, 0, 0), (0, 0))) == ["6627e8d5", "e169c58d", "bc57ac4c", "9b00dbd8"]
    f = 0xFFFFFFFF
    assert hexs(R.philox4x32_10((f, f, f, f), (f, f))) == ["408f276d", "41c83b0e", "a20bc7c6", "6d5451fd"]
    assert hexs(R.philox4x32_10((0x243F6A88, 0x85A308D3, 0x13198A2E, 0x03707344), (0xA4093822, 0x299F31D0))) == \
        ["d16cfe09", "94fdcceb", "5001e420", "24126ea1"]
    # the law's layout: key = (seed low, seed high), counter = (group low, group high, stream, 0); arrays equal scalars
    seed, groups = 2 ** 32 * 7 + 5, np.array([0, 1, 2 ** 32 + 3], dtype=np.uint64)
    w = R.words(groups, 1, seed)
    assert w.shape == (3, 4)
    assert hexs(w[2]) == hexs(R.philox4x32_10((3, 1, 1, 0), (5, 7))) and hexs(w[0]) == hexs(R.philox4x32_10((0, 0, 1, 0), (5, 7)))
    assert hexs(R.words([0], 0, 0)) == ["6627e8d5", "e169c58d", "bc57ac4c", "9b00dbd8"]


@pytest.mark.parametrize("std,fraction", CASES + [(5.0, 1.0), (0.3, 0.5), (1.0, 7.0), (1.0, -2.0)])
def test_table_against_float64_erfc(std, fraction):
    t = eventaug.noise_table(std, fraction)
    f = min(max(fraction, 0.0), 1.0)
    assert list(t) == R.table(std, fraction) and len(t) <= eventaug.TABLE_MAX == R.TABLE_MAX
    for m, v in enumerate(t, start=1):
        assert v == math.floor(2.0 ** 32 * f * math.erfc(m / (std * math.sqrt(2.0)))) and 0 < v < 2 ** 32
    assert all(a > b for a, b in zip(t, t[1:]))                              # strictly decreasing
    assert math.floor(2.0 ** 32 * f * math.erfc((len(t) + 1) / (std * math.sqrt(2.0)))) == 0        # ends at the first zero entry
    if f == 0.0:
        assert t == ()


def test_table_refusals():
    assert eventaug.noise_table(1.0, 0.0) == () and eventaug.noise_table(3.0, 0) == ()
    assert len(eventaug.noise_table(5.0, 1.0)) <= 32
    with pytest.raises(ValueError, match="cap of 32"):
        eventaug.noise_table(8.0, 1.0)
    for bad in (0.0, -1.0, float("inf"), float("nan")):
        with pytest.raises(ValueError, match="std"):
            eventaug.noise_table(bad, 0.5)
    with pytest.raises(ValueError):
        eventaug.noise_table(1.0, float("nan"))
    header = open(N.HEADER).read()
    assert "#define EBFI_NOISE_TABLE_MAX %d" % eventaug.TABLE_MAX in header


# ------------------------------------------------------------------------------------------------ distribution
def _classes(k):
    k = np.asarray(k).reshape(-1)
    return np.bincount(np.minimum(k, 4), minlength=5)


@pytest.mark.parametrize("std,fraction", CASES)
def test_class_frequencies_of_both_laws_match_the_closed_form(std, fraction):
    """Every count of the classes k = 0, 1, 2, 3, >= 4 over N cells lies within 5 binomial standard deviations of N p, for the
    restated device law and for the reference's draw alike (the reference's draw alone stays within 2.91 on these inputs)."""
    p = np.array(R.class_probabilities(std, fraction))
    assert abs(p.sum() - 1.0) < 1e-12
    sd = np.sqrt(CELLS * p * (1.0 - p))
    tab = R.table(std, fraction)
    for seed in SEEDS:
        for law, k in (("device", R.noise_field(SHAPE, seed, tab)),
                       ("host", clipdata.draw_noise((1,) + SHAPE, seed, std, fraction).numpy())):
            z = (_classes(k) - CELLS * p) / sd
            print("std %g fraction %g seed %d %s law: z = %s" % (std, fraction, seed, law, np.round(z, 2).tolist()))
            assert np.all(np.abs(z) <= SIGMAS), (law, seed, z.tolist())


@pytest.mark.parametrize("std,fraction", [(1.0, 0.05), (1.0, 1.0)])
def test_adjacent_seeds_and_neighbouring_cells_are_independent(std, fraction):
    """The nonzero masks of seeds s and s + 1 -- adjacent seeds are what the loaders hand out -- coincide at a rate within 5
    standard deviations of p^2, and so does a cell with its lag-1 neighbour inside one field."""
    tab = R.table(std, fraction)
    p = 1.0 - R.class_probabilities(std, fraction)[0]
    q = p * p
    for seed in SEEDS:
        a = R.noise_field(SHAPE, seed, tab).reshape(-1) > 0
        b = R.noise_field(SHAPE, seed + 1, tab).reshape(-1) > 0
        for what, hits, n in (("seed", int(np.count_nonzero(a & b)), CELLS),
                              ("lag-1", int(np.count_nonzero(a[:-1] & a[1:])), CELLS - 1)):
            z = (hits - n * q) / math.sqrt(n * q * (1.0 - q))
            print("std %g fraction %g seed %d %s: z = %.2f" % (std, fraction, seed, what, z))
            assert abs(z) <= SIGMAS, (what, seed, z)


def test_noise_field_is_a_function_of_the_cell_alone():
    """A load of a multi-load item draws its own cells of the item's field, wherever it starts in a Philox group."""
    tab = R.table(2.5, 1.0)
    whole = R.noise_field((3, 2, 5, 7), 9, tab).reshape(-1)
    assert whole.max() >= 3
    for first in (0, 1, 2, 3, 70, 137, 140):
        assert np.array_equal(R.noise_field((2, 5, 7), 9, tab, first_cell=first).reshape(-1), whole[first:first + 70])


def test_hot_pixels_restated():
    img = R.hot_pixels(2, 2, 5, 2.0, 2.0)                       # eight pixels on four cells
    u = R.words(np.arange(8, dtype=np.uint64), 1, 5)
    amp = R.counts(u[:, 2], R.table(2.0, 1.0))
    assert R.hot_pixel_count(2.0, 2, 2) == eventaug.hot_pixel_count(2.0, 2, 2) == 8 and img.sum() == amp.sum() > 0
    assert R.hot_pixel_count(0.05, 19, 22) == eventaug.hot_pixel_count(0.05, 19, 22) == int(0.05 * 19 * 22) == 20
    assert R.hot_pixels(19, 22, 4, 2.0, 0.0).sum() == 0


# ------------------------------------------------------------------------------------------------ plumbing
def _section(**aug):
    base = {"enabled": True, "augment": ["RandomCrop", "CenterCrop", "HorizontalFlip", "VertivcalFlip", "Noise", "HotPixel"],
            "noise": {"enabled": True, "noise_std": 1.0, "noise_fraction": 0.05},
            "hot_pixel": {"enabled": True, "hot_pixel_std": 2.0, "hot_pixel_fraction": 0.01}}
    base.update(aug)
    return {"scale": 1, "ori_scale": "ori", "data_augment": base}


def test_dataset_args_from_config_hot_pixels_are_opt_in():
    assert "hot_pixels" not in clipdata.dataset_args_from_config(_section())                     # the default: as before
    got = clipdata.dataset_args_from_config(_section(), hot_pixels=True)
    assert got["hot_pixels"] == (2.0, 0.01) and got["noise"] == (1.0, 0.05)
    assert "hot_pixels" not in clipdata.dataset_args_from_config(
        _section(hot_pixel={"enabled": False, "hot_pixel_std": 2.0, "hot_pixel_fraction": 0.01}), hot_pixels=True)
    assert "hot_pixels" not in clipdata.dataset_args_from_config(_section(augment=["RandomCrop", "Noise"]), hot_pixels=True)
    assert "hot_pixels" not in clipdata.dataset_args_from_config(_section(enabled=False), hot_pixels=True)
    # the reference's defaults of add_hot_pixels where a key is absent
    assert clipdata.dataset_args_from_config(_section(hot_pixel={"enabled": True}), hot_pixels=True)["hot_pixels"] == (1.0, 0.001)


def test_flag_defaults_and_choices():
    import infer_ours
    import train_ours
    import train_ours_exposuredecision as stage1
    ap = argparse.ArgumentParser()
    train_ours.add_loader_arguments(ap)
    d = ap.parse_args([])
    assert d.event_noise == "host" and d.hot_pixels is False
    a = ap.parse_args(["--event-noise", "device", "--hot-pixels"])
    assert a.event_noise == "device" and a.hot_pixels is True
    with pytest.raises(SystemExit):
        ap.parse_args(["--event-noise", "gpu"])
    s = stage1.build_parser().parse_args(["--event-noise", "device"])
    assert s.event_noise == "device" and s.hot_pixels is False
    assert train_ours.get_args([]).event_noise == "host"
    f = infer_ours.get_flags([])
    assert f.event_noise == "host" and f.hot_pixels is False
    ds, _ = infer_ours.dataset_settings(f)
    assert ds["event_noise"] == "host" and ds["hot_pixels"] is None
    assert infer_ours.noise_law_name(ds) == "host law, std 1 on a fraction 0.05 of the cells"
    ds, _ = infer_ours.dataset_settings(infer_ours.get_flags(["--event-noise", "device", "--hot-pixels"]))
    assert ds["event_noise"] == "device" and ds["hot_pixels"] == (2.0, 0.001)          # the reference's own hot_pixel section
    assert infer_ours.noise_law_name(ds) == "device law, std 1 on a fraction 0.05 of the cells, hot pixels std 2 fraction 0.001"
    ds, _ = infer_ours.dataset_settings(infer_ours.get_flags(["--noise_enabled", "--event-noise", "device", "--hot-pixels"]))
    assert ds["hot_pixels"] is None and infer_ours.noise_law_name(ds) == "off"          # (store_false: noise and hot pixels OFF)


def test_trainers_hand_the_flags_to_the_dataset(tmp_path):
    import train_ours
    clipdata.write_synthetic_clip(str(tmp_path / "c.npz"), num_imgs=9, H=12, W=20, events_per_frame=20, seed=1)
    cfg = dict(_section(), NumFramePerPeriod=4, NumFramePerBlurry=2, ExposureMethod="Fixed")
    ds = train_ours.clip_dataset(str(tmp_path), cfg, 2, [2], "cpu", 1, "host")
    assert ds.noise_mode == "host" and ds.hot_pixels is None and ds.noise_table is None and ds.noise == (1.0, 0.05)
    ds = train_ours.clip_dataset(str(tmp_path), train_ours.with_noise_law(cfg, "device", True), 2, [2], "cpu", 1, "device")
    assert ds.noise_mode == "device" and ds.hot_pixels == (2.0, 0.01) and ds.noise_table == eventaug.noise_table(1.0, 0.05)
    ds = train_ours.clip_dataset(str(tmp_path), train_ours.with_noise_law(cfg, "device", False), 2, [2], "cpu", 1, "device")
    assert ds.noise_mode == "device" and ds.hot_pixels is None
    with pytest.raises(ValueError, match="noise_mode='device'"):          # --hot-pixels without --event-noise device
        train_ours.clip_dataset(str(tmp_path), train_ours.with_noise_law(cfg, "host", True), 2, [2], "cpu", 1, "host")
    assert cfg.get("event_noise") is None                                   # (the section itself is not written to)


def test_device_mode_prepares_no_noise(tmp_path, monkeypatch):
    path = clipdata.write_synthetic_clip(str(tmp_path / "c.npz"), num_imgs=9, H=12, W=20, events_per_frame=20, seed=1)
    kw = dict(time_bins=2, frames_per_period=4, frames_per_blurry=3, crop=[8, 12], flips=True, noise=(1.0, 0.5), device="cpu")
    host = clipdata.ClipDataset(path, frames="device", **kw)
    assert host.noise_mode == "host" and host.prepare(1, 5)["noise"].shape == (1, 2, 2, 8, 12)

    def boom(*a, **k):
        raise AssertionError("draw_noise called in device mode")

    monkeypatch.setattr(clipdata, "draw_noise", boom)
    for frames in ("device", "host"):
        ds = clipdata.ClipDataset(path, frames=frames, noise_mode="device", hot_pixels=(2.0, 0.05), **kw)
        p = ds.prepare(1, 5)
        assert "noise" not in p and ds.noise_table == eventaug.noise_table(1.0, 0.5) and ds.hot_pixels == (2.0, 0.05)
    assert clipdata.ClipDataset(path, noise_mode="device", device="cpu", frames_per_period=4, frames_per_blurry=2).noise_table == ()
    with pytest.raises(ValueError, match="noise_mode"):
        clipdata.ClipDataset(path, noise_mode="gpu", **kw)
    with pytest.raises(ValueError, match="noise_mode='device'"):
        clipdata.ClipDataset(path, hot_pixels=(1.0, 0.01), **kw)
    with pytest.raises(ValueError, match="cap of 32"):
        clipdata.ClipDataset(path, noise_mode="device", hot_pixels=(9.0, 0.01), **kw)
    real = clipdata.write_synthetic_clip(str(tmp_path / "r.npz"), num_imgs=5, H=12, W=20, events_per_frame=20, seed=2,
                                         exposure_stamps=True)
    with pytest.raises(ValueError, match="noise_mode='device'"):
        clipdata.RealBlurClipDataset(real, time_bins=2, hot_pixels=(1.0, 0.01), device="cpu")
    rb = clipdata.RealBlurClipDataset(real, time_bins=2, noise=(1.0, 0.05), noise_mode="device", hot_pixels=(1.0, 0.01), device="cpu")
    assert rb.noise_table == eventaug.noise_table(1.0, 0.05) and rb.hot_pixels == (1.0, 0.01)


def test_ops_refuse_cpu_tensors_and_bad_tables():
    x = torch.zeros(2, 3, 4, 4).transpose(0, 1)
    with pytest.raises(NotImplementedError):
        eventaug.augment_events(x, None, False, False, 0, ())
    with pytest.raises(NotImplementedError):
        eventaug.add_hot_pixels(torch.zeros(6, 4, 4), 0, 1.0, 0.1)


def test_entry_points_are_declared_bound_and_refuse_bad_arguments():
    for name in ("ebfi_event_augment", "ebfi_event_hot_pixels"):
        assert name in N.declared_symbols() and name in N.SIGNATURES
    assert "#define EBFI_ABI_VERSION 14" in open(N.HEADER).read() and N.ABI_VERSION == 14      # a pure addition
    lib = N.lib()
    assert lib.ebfi_abi_version() == 14
    # argument errors are refused before anything touches the GPU (none is needed here)
    src, dst = ctypes.c_void_p(1 << 20), ctypes.c_void_p(1 << 30)
    s3 = (ctypes.c_int64 * 3)(16, 48, 4)                                    # a transposed [2, 3, 4, 4] tensor
    tab = (ctypes.c_uint32 * 3)(900, 50, 2)
    ok = (3, 4, 4, 0, 0, 4, 4, 0, 0, 7, tab, 3, 0)

    def aug(src=src, s=s3, rest=ok, dst=dst):
        return lib.ebfi_event_augment(src, s, *rest, dst, None)

    assert aug(src=None) == -1 and b"null" in lib.ebfi_last_error()
    assert aug(dst=None) == -1 and b"null" in lib.ebfi_last_error()
    assert aug(s=None) == -1 and b"null" in lib.ebfi_last_error()
    assert aug(rest=(3, 4, 4, 0, 0, 4, 4, 0, 0, 7, None, 3, 0)) == -1 and b"null" in lib.ebfi_last_error()
    for win in ((0, 0, 5, 4), (1, 0, 4, 4), (0, 2, 4, 3), (-1, 0, 2, 2), (0, 0, 0, 4), (0, -1, 4, 4)):
        assert aug(rest=(3, 4, 4) + win + (0, 0, 7, tab, 3, 0)) == -1 and b"window" in lib.ebfi_last_error(), win
    assert aug(rest=(0,) + ok[1:]) == -1 and b"sizes" in lib.ebfi_last_error()
    for bad in ((-16, 48, 4), (16, -48, 4), (16, 48, -4)):
        assert aug(s=(ctypes.c_int64 * 3)(*bad)) == -1 and b"strides" in lib.ebfi_last_error(), bad
    assert aug(rest=ok[:11] + (33, 0)) == -1 and b"table_len" in lib.ebfi_last_error()
    assert aug(rest=ok[:11] + (-1, 0)) == -1 and b"table_len" in lib.ebfi_last_error()
    assert aug(rest=ok[:12] + (-4,)) == -1 and b"cell_offset" in lib.ebfi_last_error()
    # the source spans (3 - 1) * 16 + 48 + 3 * 4 + 4 = 96 floats, the destination 3 * 2 * 4 * 4 = 96: every way of overlapping
    base = 1 << 20
    for d in (base, base + 4 * 95, base - 4 * 95, base + 8):
        assert aug(dst=ctypes.c_void_p(d)) == -1 and b"overlap" in lib.ebfi_last_error(), d

    p = ctypes.c_void_p(1 << 20)
    assert lib.ebfi_event_hot_pixels(None, 6, 4, 4, 7, tab, 3, 2, None) == -1 and b"null" in lib.ebfi_last_error()
    assert lib.ebfi_event_hot_pixels(p, 6, 4, 4, 7, None, 3, 2, None) == -1 and b"null" in lib.ebfi_last_error()
    for planes, h, w in ((0, 4, 4), (6, 0, 4), (6, 4, 0), (6, 65536, 65536)):
        assert lib.ebfi_event_hot_pixels(p, planes, h, w, 7, tab, 3, 2, None) == -1 and b"sizes" in lib.ebfi_last_error()
    assert lib.ebfi_event_hot_pixels(p, 6, 4, 4, 7, tab, 3, -1, None) == -1 and b"n_hot" in lib.ebfi_last_error()
    assert lib.ebfi_event_hot_pixels(p, 6, 4, 4, 7, tab, 3, 1 << 40, None) == -1 and b"n_hot" in lib.ebfi_last_error()
    assert lib.ebfi_event_hot_pixels(p, 6, 4, 4, 7, tab, 40, 2, None) == -1 and b"table_len" in lib.ebfi_last_error()
    # nothing to add: a no-op that needs no GPU either
    assert lib.ebfi_event_hot_pixels(p, 6, 4, 4, 7, tab, 3, 0, None) == 0
    assert lib.ebfi_event_hot_pixels(p, 6, 4, 4, 7, None, 0, 5, None) == 0
