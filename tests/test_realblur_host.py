"""Host side of `infer_ours.py --real_blur`: ebfi_amd.clipdata.RealBlurClipDataset against a fixture produced by the
reference's own real-data H5Dataset (tests/golden/make_golden_realblur.py: dataloader/h5dataset_realdata.py run on an in-memory
exposure-stamped clip), and what the script's `dataset_settings` records for the flag.  No GPU: the frame and the event stack of
an item are device work (tests/test_gpu_realblur.py); here the event LIST of every load is binned by the oracle's
events_to_stack, itself pinned bit-exactly to the reference function."""
import importlib.util
import os

import numpy as np
import pytest
import torch

from ebfi_amd import clipdata

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
PKG = os.path.join(ROOT, "ebfi-be_amd")

CFGS = {"crop_noise": dict(crop=[16, 24], noise=(1.0, 0.05)), "plain": dict(crop=None, noise=None)}
# scripts/infer_ours.sh of the reference, its RealBlur block and its first block, argument for argument
REFERENCE_ARGS_REAL = ["--model_path", "/path/to/model", "--data_list", "/path/to/test.txt", "--output_path", "/path/to/output",
                       "--scale", "2", "--ori_scale", "down2", "--time_bins", "16", "--interp_num", "256", "--num_period_per_seq", "2",
                       "--sliding_window_seq", "2", "--num_period_per_load", "1", "--sliding_window_load", "1", "--noise_enabled",
                       "--real_blur"]
REFERENCE_ARGS = ["--model_path", "/path/to/model", "--data_list", "/path/to/test.txt", "--output_path", "/path/to/output",
                  "--scale", "2", "--ori_scale", "down2", "--time_bins", "16", "--num_frame_per_period", "16",
                  "--num_frame_per_blurry", "3", "--num_period_per_seq", "2", "--sliding_window_seq", "2",
                  "--num_period_per_load", "1", "--sliding_window_load", "1", "--exposure_method", "Fixed", "--noise_enabled"]


@pytest.fixture(scope="module")
def fixture(golden_dir, tmp_path_factory):
    z = np.load(os.path.join(golden_dir, "realblur_small.npz"))
    path = str(tmp_path_factory.mktemp("realclip") / "clip0.npz")
    np.savez(path, **{k[5:]: z[k] for k in z.files if k.startswith("clip.")})
    return z, path


@pytest.fixture(scope="module")
def cli():
    spec = importlib.util.spec_from_file_location("ebfi_infer_ours_real", os.path.join(PKG, "infer_ours.py"))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod


def _dataset(path, tag, device="cpu"):
    return clipdata.RealBlurClipDataset(path, time_bins=4, interp_num=5, periods_per_seq=2, sliding_window_seq=2, periods_per_load=1,
                                        sliding_window_load=1, device=device, **CFGS[tag])


@pytest.mark.parametrize("tag", ["crop_noise", "plain"])
def test_items_indices_duty_and_timestamps_are_the_references(fixture, tag):
    """8 frames -> 7 periods -> 3 sequences of 2 loads (the seventh period starts no full sequence); duty and timestamps bit for
    bit; the duty is (end - begin) / (next begin - begin) of the stamps."""
    z, path = fixture
    ds = _dataset(path, tag)
    assert ds.num_periods == 7 and len(ds) == int(z["%s.len" % tag]) == 3
    assert np.array_equal(np.array(ds.items, dtype=np.int64), z["%s.seq_indices" % tag])
    begin, end = z["clip.exposure_begin_t"], z["clip.exposure_end_t"]
    for i in range(len(ds)):
        frames, events, duty, rel_ts = ds.host_item(i)
        ref_duty, ref_ts = z["%s.%d.SeqExposureDuty" % (tag, i)], z["%s.%d.RelativeLatentTs" % (tag, i)]
        assert duty.dtype == torch.float32 and tuple(duty.shape) == ref_duty.shape == (2, 1, 1)
        assert np.array_equal(duty.numpy(), ref_duty), (tag, i)
        assert rel_ts.dtype == torch.float32 and tuple(rel_ts.shape) == ref_ts.shape == (2, 1, 5)
        assert np.array_equal(rel_ts.numpy(), ref_ts), (tag, i)
        for k, (left, right) in enumerate(ds.items[i]):
            assert left == right
            want = np.float32((end[left] - begin[left]) / (begin[left + 1] - begin[left]))
            assert duty[k, 0, 0].item() == want and 0 < want < 1
            # the frame is the stored array, channels as stored (the real-data GetFrames does not swap)
            assert frames.dtype == np.uint8 and np.array_equal(frames[k], z["clip.images"][left])
    assert np.array_equal(ds.timestamps().numpy(), np.array([0, 0.25, 0.5, 0.75, 1], dtype=np.float32))


@pytest.mark.parametrize("tag", ["crop_noise", "plain"])
def test_event_lists_are_what_the_reference_sliced(fixture, tag):
    """Events of load (left, right) run from event_idx[left] to event_idx[right + 1], normalised to (t - t0) / (tN - t0 + 1e-6);
    an interval without events is the single all-zero event.  Rebuilt here from the clip arrays; binned by the oracle, cropped and
    (for the noise config) given the reference's noise, they are the reference's SeqHREv bit for bit."""
    from oracle import events_ref
    z, path = fixture
    ds = _dataset(path, tag)
    idx, H, W = z["clip.event_idx"], 26, 34
    empty = 0
    for i in range(len(ds)):
        _, events, _, _ = ds.host_item(i)
        stacks = []
        for (left, right), (xs, ys, ts, ps) in zip(ds.items[i], events):
            a, b = int(idx[left]), int(idx[right + 1])
            if a == b:
                empty += 1
                assert all(np.array_equal(v, np.array([0.0])) for v in (xs, ys, ts, ps))
            else:
                t = z["clip.ts"][a:b]
                assert np.array_equal(ts, (t - t[0]) / (t[-1] - t[0] + 1e-6)) and ts.dtype == np.float64
                for got, key in ((xs, "xs"), (ys, "ys"), (ps, "ps")):
                    assert got.dtype == np.float64 and np.array_equal(got, z["clip." + key][a:b].astype(np.float64))
            stacks.append(torch.from_numpy(events_ref.events_to_stack(xs, ys, ts, ps.astype(np.float32), 4, (H, W))).transpose(0, 1))
        stack = torch.stack(stacks)
        win = ds.window()
        if tag == "crop_noise":
            assert win == (5, 5, 16, 24)
            stack = clipdata.add_noise(stack[..., 5:21, 5:29], 5 + 3, *ds.noise)
        else:
            assert win is None
        assert np.array_equal(stack.numpy(), z["%s.%d.SeqHREv" % (tag, i)]), (tag, i)
    assert empty == 1          # (frames 3 -> 4 of the fixture clip)


def test_clip_without_exposure_stamps_is_refused(fixture, tmp_path):
    z, _ = fixture
    bare = str(tmp_path / "bare.npz")
    np.savez(bare, **{k[5:]: z[k] for k in z.files if k.startswith("clip.") and "exposure" not in k})
    with pytest.raises(ValueError, match="exposure_begin_t"):
        clipdata.RealBlurClipDataset(bare, time_bins=4, interp_num=5)
    clipdata.ClipDataset(bare, time_bins=4, frames_per_period=4, frames_per_blurry=2, device="cpu")      # still a fine synthetic-blur clip
    short = str(tmp_path / "short.npz")
    np.savez(short, **dict({k[5:]: z[k] for k in z.files if k.startswith("clip.")}, exposure_end_t=z["clip.exposure_end_t"][:-1]))
    with pytest.raises(ValueError, match="one stamp per image"):
        clipdata.RealBlurClipDataset(short, time_bins=4, interp_num=5)


def test_real_blur_settings_and_notes(cli):
    ds, notes = cli.dataset_settings(cli.get_flags(REFERENCE_ARGS_REAL))
    assert ds["real_blur"] is True and ds["interp_num"] == 256
    assert any("real_blur" in n for n in notes)
    assert not any("interp_num only applies" in n for n in notes)
    assert any("nothing is scored" in n and "exposure-stamped" in n for n in notes)
    assert not any("synthetic-blur clips" in n for n in notes)
    assert (ds["NumPeriodPerSeq"], ds["SlidingWindowSeq"], ds["NumPeriodPerLoad"], ds["SlidingWindowLoad"]) == (2, 2, 1, 1)


def test_synthetic_blur_settings_are_unchanged(cli):
    ds, notes = cli.dataset_settings(cli.get_flags(REFERENCE_ARGS))
    assert notes == [] and ds["real_blur"] is False and ds["interp_num"] == 16
    ds, notes = cli.dataset_settings(cli.get_flags(REFERENCE_ARGS + ["--interp_num", "8"]))
    assert notes == ["interp_num only applies to --real_blur in the reference; ignored"] and ds["real_blur"] is False
    ds, notes = cli.dataset_settings(cli.get_flags(["--data_list", "x.txt", "--output_path", "o"]))
    assert len(notes) == 1 and "num_period_per_load" in notes[0]
    assert cli.get_flags(REFERENCE_ARGS).save_float is False and cli.get_flags(REFERENCE_ARGS_REAL + ["--save_float"]).save_float is True


def test_write_synthetic_clip_default_is_unchanged(tmp_path):
    """The stamps are an option: every array of the default clip is the same with the option off, on, and left out, and the
    default file gains no array."""
    paths = {k: str(tmp_path / (k + ".npz")) for k in ("default", "off", "on")}
    clipdata.write_synthetic_clip(paths["default"], num_imgs=9, H=12, W=14, events_per_frame=30, seed=4)
    clipdata.write_synthetic_clip(paths["off"], num_imgs=9, H=12, W=14, events_per_frame=30, seed=4, exposure_stamps=False)
    clipdata.write_synthetic_clip(paths["on"], num_imgs=9, H=12, W=14, events_per_frame=30, seed=4, exposure_stamps=True)
    z = {k: np.load(p) for k, p in paths.items()}
    assert sorted(z["default"].files) == sorted(z["off"].files) == ["event_idx", "images", "ps", "ts", "xs", "ys"]
    for k in z["default"].files:
        for other in ("off", "on"):
            assert z["default"][k].dtype == z[other][k].dtype and np.array_equal(z["default"][k], z[other][k]), (k, other)
    # pinned: the first values of the seeded default clip (unchanged by the option's existence)
    g = np.random.RandomState(4)
    assert np.array_equal(z["default"]["images"], g.randint(0, 256, size=(9, 12, 14, 3)).astype(np.uint8))
    begin, end = z["on"]["exposure_begin_t"], z["on"]["exposure_end_t"]
    assert begin.shape == end.shape == (9,) and (np.diff(begin) > 0).all() and (end > begin).all() and (end[:-1] < begin[1:]).all()
    ds = clipdata.RealBlurClipDataset(paths["on"], time_bins=4, interp_num=3, device="cpu")
    assert ds.num_periods == 8 and len(ds) == 4 and all(0 < ds.exposure_duty(i) < 1 for i in range(8))
