"""ClipDataset(frames="device") and the prefetching batch generators on the GPU: the items are the reference dataset's own
(tests/golden/clipdata_small.npz, produced by dataloader/h5dataset.py), equal the frames="host" items bit for bit under every
crop / flip / noise combination, arrive in the same batches with a worker thread preparing ahead, and train the same model:
`train_ours.py --data` with the defaults against `--loader host --prefetch 0`."""
import os
import re
import subprocess
import sys

import numpy as np
import pytest
import torch

from ebfi_amd import clipdata

KEYS = ("SeqLatentF", "SeqBlurryF", "SeqHREv", "RelativeLatentTs", "SeqExposureDuty")
# the configurations of tests/test_clipdata.py (those the fixture was produced with)
CFGS = {"fixed": dict(frames_per_period=8, frames_per_blurry=5, exposure_method="Fixed", exposure_time=[1], crop=None),
        "custom": dict(frames_per_period=6, frames_per_blurry=6, exposure_method="Custom", exposure_time=[3, 4, 6], crop=[16, 16]),
        "noise": dict(frames_per_period=8, frames_per_blurry=3, exposure_method="Fixed", exposure_time=[1], crop=[16, 24],
                      noise=(1.0, 0.05))}
# the synthetic clip: periods of 4 frames exposed for 1, 3 and 4 of them; every augmentation on
AUGMENTS = {"random_crop": dict(crop=[16, 16], crop_mode="random"),
            "random_then_centre": dict(crop=[16, 16], crop_mode="random", center_crop=[8, 8])}
SEEDS = (5, 1, 0, 3)          # with probabilities 0.5: no flip, horizontal only, vertical only, both


@pytest.fixture(scope="module")
def fixture(golden_dir, tmp_path_factory):
    z = np.load(os.path.join(golden_dir, "clipdata_small.npz"))
    path = str(tmp_path_factory.mktemp("clip") / "clip0.npz")
    np.savez(path, **{k[5:]: z[k] for k in z.files if k.startswith("clip.")})
    return z, path


@pytest.fixture(scope="module")
def synthetic(tmp_path_factory):
    return clipdata.write_synthetic_clip(str(tmp_path_factory.mktemp("synthetic") / "clip.npz"), num_imgs=17, H=32, W=32,
                                         events_per_frame=300, seed=3)


def _synthetic_dataset(path, frames, **augment):
    return clipdata.ClipDataset(path, time_bins=4, frames_per_period=4, exposure_method="Custom", exposure_time=[1, 3, 4],
                                flips=True, noise=(1.0, 0.1), device="cuda", frames=frames, **augment)


def _assert_same_item(a, b, what):
    assert sorted(a) == sorted(b) == sorted(KEYS)
    for k in KEYS:
        assert a[k].is_cuda and a[k].dtype == b[k].dtype and a[k].shape == b[k].shape, (what, k)
        assert torch.equal(a[k], b[k]), (what, k)


@pytest.mark.gpu
@pytest.mark.parametrize("tag", ["fixed", "custom", "noise"])
def test_device_items_match_the_reference_dataset(fixture, tag):
    z, path = fixture
    ds = clipdata.ClipDataset(path, time_bins=4, crop_mode="center", flips=False, device="cuda", frames="device", **CFGS[tag])
    assert len(ds) == int(z["%s.len" % tag]) > 1
    for i in range(len(ds)):
        item = ds.__getitem__(i, seed=5)
        for k in KEYS:
            assert item[k].is_cuda
            assert np.array_equal(item[k].cpu().numpy(), z["%s.%d.%s" % (tag, i, k)]), (tag, i, k)


@pytest.mark.gpu
@pytest.mark.parametrize("augment", sorted(AUGMENTS))
def test_device_items_equal_host_items_under_every_augmentation(synthetic, augment):
    dev, host = (_synthetic_dataset(synthetic, frames, **AUGMENTS[augment]) for frames in ("device", "host"))
    assert len(dev) == len(host) == 4 and [len(it[1]) for _, it in dev.items] == [1, 3, 4, 1]
    assert [dev.flip_decisions(s) for s in SEEDS] == [(False, False), (True, False), (False, True), (True, True)]
    size = 8 if "center_crop" in AUGMENTS[augment] else 16
    windows = set()
    for seed in SEEDS:
        for i in range(len(dev)):
            a, b = dev.__getitem__(i, seed=seed), host.__getitem__(i, seed=seed)
            assert a["SeqLatentF"].shape == (1, 1, 4, 3, size, size) and a["SeqHREv"].shape == (1, 4, 2, size, size)
            _assert_same_item(a, b, (augment, seed, i))
            _assert_same_item(dev.finish(dev.prepare(i, seed)), a, (augment, seed, i, "halves"))
        windows.add(dev.window((32, 32), seed))
    assert len(windows) > 1                                      # the seeds crop at different places
    assert dev.prepare(0, 5)["stage"].is_pinned() and "stage" not in host.prepare(0, 5)


@pytest.mark.gpu
def test_prefetched_batches_equal_the_synchronous_host_batches(synthetic):
    import threading
    before = threading.active_count()
    dev, host = (_synthetic_dataset(synthetic, frames, **AUGMENTS["random_crop"]) for frames in ("device", "host"))
    ref = list(clipdata.batches(host, 2, seed=1, epochs=2, prefetch=0))
    assert len(ref) == 4
    ref_eval = list(clipdata.eval_batches(host, 3, seed=1, prefetch=0))
    assert [b["SeqBlurryF"].shape[0] for b in ref_eval] == [3, 1]
    for prefetch in (1, 2):
        got = list(clipdata.batches(dev, 2, seed=1, epochs=2, prefetch=prefetch))
        assert len(got) == len(ref)
        for k, (a, b) in enumerate(zip(got, ref)):
            assert a["SeqLatentF"].shape == (2, 1, 1, 4, 3, 16, 16)
            _assert_same_item(a, b, ("batches", prefetch, k))
        got = list(clipdata.eval_batches(dev, 3, seed=1, prefetch=prefetch))
        assert len(got) == len(ref_eval)
        for k, (a, b) in enumerate(zip(got, ref_eval)):
            _assert_same_item(a, b, ("eval_batches", prefetch, k))
    assert not torch.equal(ref[0]["SeqBlurryF"], ref[2]["SeqBlurryF"])      # the second epoch draws other crops
    assert threading.active_count() == before


def _train(root, cfg_path, data, out_dir, extra):
    out = subprocess.run([sys.executable, os.path.join(root, "ebfi-be_amd", "train_ours.py"), "-c", cfg_path, "--data", data,
                          "--iterations", "3"] + extra, capture_output=True, text=True, timeout=600)
    assert out.returncode == 0, out.stderr[-2000:]
    losses = re.findall(r"Iteration: (\d+)/3 train_loss: (\S+)", out.stdout)
    saved = re.findall(r"^saved (\S+)$", out.stdout, flags=re.M)
    assert [k for k, _ in losses] == ["0", "1", "2"] and len(saved) == 1 and saved[0].startswith(out_dir)
    return [v for _, v in losses], torch.load(saved[0], map_location="cpu", weights_only=False)


@pytest.mark.gpu
def test_train_ours_is_the_same_run_with_either_loader(tmp_path):
    """Three optimiser steps on two small clips (the reduced model of test_train_ours_runs_on_recorded_clips), once with
    `--loader host --prefetch 0` and once with the defaults (device, prefetch 1): same printed losses, same saved tensors."""
    import yaml
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    data = tmp_path / "clips"
    data.mkdir()
    for k in range(2):
        clipdata.write_synthetic_clip(str(data / ("clip%d.npz" % k)), num_imgs=17, H=32, W=32, events_per_frame=300, seed=k)
    runs = []
    for name, extra in (("host", ["--loader", "host", "--prefetch", "0"]), ("default", [])):
        cfg = yaml.safe_load(open(os.path.join(root, "ebfi-be_amd", "config", "train_ours.yml")))
        cfg["model"]["args"].update(FrameBasech=16, EventBasech=16, InterCH=16, TB=4, step=2, channels=[4, 4, 8, 8])
        cfg["trainer"].update(batch_size=2, output_path=str(tmp_path / name))
        cfg["trainer"].setdefault("iteration_based_train", {})["train_log_step"] = 1
        cfg["train_dataloader"] = {"dataset": {"time_bins": 4, "NumFramePerPeriod": 4, "NumFramePerBlurry": 3, "ExposureMethod": "Fixed"}}
        cfg_path = str(tmp_path / ("cfg_%s.yml" % name))
        yaml.safe_dump(cfg, open(cfg_path, "w"))
        runs.append(_train(root, cfg_path, str(data), str(tmp_path / name), extra))
    (loss_a, ckpt_a), (loss_b, ckpt_b) = runs
    assert loss_a == loss_b, (loss_a, loss_b)
    states_a, states_b = ckpt_a["model"]["states"], ckpt_b["model"]["states"]
    assert sorted(states_a) == sorted(states_b) and len(states_a) > 10
    for k in states_a:
        assert torch.equal(states_a[k], states_b[k]), k
    moved = [k for k in states_a if states_a[k].dtype.is_floating_point and states_a[k].abs().sum() > 0]
    assert moved                                                    # (the runs trained something)
