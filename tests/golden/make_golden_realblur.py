#!/usr/bin/env python3
"""Golden fixture for ebfi_amd.clipdata.RealBlurClipDataset: RUNS THE REFERENCE'S OWN real-data H5Dataset
(/root/reference/dataloader/h5dataset_realdata.py; build container only) on a small random exposure-stamped clip and stores
what `__getitem__` returned.

    python tests/golden/make_golden_realblur.py        # rewrites tests/golden/realblur_small.npz

The class is run without HDF5 the way make_golden_clipdata.py runs the synthetic-blur one: placeholder modules for h5py / cv2
(never called: `gt_sensor_resolution` is set as a TUPLE, so `frame.shape[:-1] != self.gt_sensor_resolution` is false and no
frame goes through cv2.resize -- with the list set_data_scale stores, every frame would), and the in-memory mapping of that
script in place of the open file, each image carrying `exposure_begin_t` / `exposure_end_t` attributes.  Every index rule, the
event slice and its normalisation, the duty arithmetic, the timestamps, the crop, the noise and the (CPU) events_to_stack are
the reference's code.  Only data is written.

The clip: 8 frames of 26x34 (7 periods), about 50 events per frame interval, NONE between frames 3 and 4.  Two configs, both
NumPeriodPerSeq = SlidingWindowSeq = 2, one period per load, interp_num = 5, 4 time bins, every item at seed 5:
    crop_noise   centre crop [16, 24] (origin (5, 5)) and event noise (std 1.0 at 5 % of the cells)
    plain        no crop, no noise
3 sequences of 2 loads each; the seventh period starts no full sequence.
"""
import importlib.util
import os
import sys
import types

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
REF = "/root/reference"
sys.path.insert(0, HERE)

import make_golden_clipdata as M  # noqa: E402  (the in-memory file mapping and the import-path set-up)


def import_h5dataset_realdata():
    for n in ("h5py", "cv2"):
        sys.modules[n] = types.ModuleType(n)
    import matplotlib.pyplot as plt
    orig = plt.style.use

    def tolerant(style):               # 'seaborn-whitegrid' left matplotlib in 3.8
        try:
            orig(style)
        except Exception:
            pass
    plt.style.use = tolerant
    for name in ("dataloader", "dataloader.encodings", "dataloader.h5dataset_realdata"):
        sys.modules.pop(name, None)
    pkg = types.ModuleType("dataloader")
    pkg.__path__ = [os.path.join(REF, "dataloader")]
    sys.modules["dataloader"] = pkg
    mods = {}
    for name in ("encodings", "h5dataset_realdata"):
        spec = importlib.util.spec_from_file_location("dataloader." + name, os.path.join(REF, "dataloader", name + ".py"))
        mods[name] = importlib.util.module_from_spec(spec)
        sys.modules["dataloader." + name] = mods[name]
        spec.loader.exec_module(mods[name])
    return mods["h5dataset_realdata"]


def make_clip():
    g = np.random.RandomState(3)
    N, H, W = 8, 26, 34
    images = g.randint(0, 256, size=(N, H, W, 3)).astype(np.uint8)
    counts = g.poisson(50, size=N - 1)
    counts[3] = 0                                            # a frame interval without events
    event_idx = np.concatenate([[0], np.cumsum(counts)]).astype(np.int64)
    E = int(event_idx[-1])
    ts = np.sort(g.uniform(0, 1.0, size=E))
    clip = dict(images=images, event_idx=event_idx, xs=g.randint(0, W, size=E).astype(np.int16),
                ys=g.randint(0, H, size=E).astype(np.int16), ts=ts, ps=(g.randint(0, 2, size=E) * 2 - 1).astype(np.int8))
    begin = (np.arange(N) * 33000 + g.randint(0, 500, size=N)).astype(np.int64)      # microseconds, ~30 frames/s
    clip["exposure_begin_t"] = begin
    clip["exposure_end_t"] = begin + g.randint(3000, 30000, size=N)
    return clip


def main():
    R = import_h5dataset_realdata()
    clip = make_clip()
    N, H, W = clip["images"].shape[:3]
    out = {"clip." + k: v for k, v in clip.items()}
    cfgs = {"crop_noise": dict(crop=[16, 24], noise=True), "plain": dict(crop=None, noise=False)}
    for tag, c in cfgs.items():
        f = M.as_file(clip)
        for i in range(N):
            f["ori_images"]["image%09d" % i].attrs.update(exposure_begin_t=clip["exposure_begin_t"][i],
                                                          exposure_end_t=clip["exposure_end_t"][i])
        config = dict(scale=1, ori_scale="ori", time_bins=4, interp_num=5, NumPeriodPerSeq=2, SlidingWindowSeq=2,
                      NumPeriodPerLoad=1, SlidingWindowLoad=1,
                      data_augment=dict(enabled=True,
                                        augment=["RandomCrop", "CenterCrop", "HorizontalFlip", "VertivcalFlip", "Noise", "HotPixel"],
                                        random_crop=dict(enabled=False, size=[16, 16]),
                                        center_crop=dict(enabled=c["crop"] is not None, size=c["crop"] or [0, 0]),
                                        flip=dict(enabled=False, horizontal_prob=0.5, vertical_prob=0.5),
                                        noise=dict(enabled=c["noise"], noise_std=1.0, noise_fraction=0.05),
                                        hot_pixel=dict(enabled=c["noise"], hot_pixel_std=2.0, hot_pixel_fraction=0.001)))
        ds = R.H5Dataset.__new__(R.H5Dataset)
        ds.config, ds.h5_file_path, ds.h5_file = config, "<memory>", f
        ds.sensor_resolution = [H, W]
        ds.scale, ds.ori_scale = 1, "ori"
        ds.inp_sensor_resolution = ds.gt_sensor_resolution = (H, W)          # a tuple: see the module docstring
        ds.inp_prex = ds.gt_prex = "ori"
        ds.load_metadata()
        ds.set_items()
        out["%s.len" % tag] = np.array(len(ds))
        out["%s.seq_indices" % tag] = np.array(ds.SeqIndices, dtype=np.int64)          # [items, loads, 2 (left, right)]
        for i in range(len(ds)):
            item = ds.__getitem__(i, seed=5)
            assert sorted(item) == ["RelativeLatentTs", "SeqBlurryF", "SeqExposureDuty", "SeqHREv"]
            for k, v in item.items():
                out["%s.%d.%s" % (tag, i, k)] = v.numpy()
    path = os.path.join(HERE, "realblur_small.npz")
    np.savez_compressed(path, **out)
    print("wrote realblur_small.npz:", len(out), "arrays,", os.path.getsize(path), "bytes")


if __name__ == "__main__":
    main()
