"""Real-data entry of the hot path: recorded clips (frames + a raw event list) -> the tensors the model is fed.

What the reference's H5Dataset does between the file and the network (dataloader/h5dataset.py), minus HDF5 itself:

  * periods of `NumFramePerPeriod` consecutive sharp frames; the blurry input of a period is the MEAN of its first
    `exposure` frames and `ExposureDuty = exposure / NumFramePerPeriod` (set_period_items, h5dataset.py:118-166:
    Fixed / Custom exposure; 'Auto' draws the exposure with numpy's global generator there and with a seeded one here),
  * the events between the first and the last latent frame of the period, timestamps normalised to
    `(t - t0) / (tN - t0 + 1e-6)` (GetEventsIndex, :327-336; an empty slice becomes the single all-zero event), binned by
    `events_to_stack(..., B=time_bins)` and transposed to [TB, 2, H, W] (:349) -- here by the DEVICE kernel
    (ebfi_amd.encodings, bit-exact with the reference function),
  * `RelativeLatentTs[k] = k / NumFramePerPeriod` for the k-th latent frame (GetTimestamp, :354-366, NumPeriodPerLoad = 1),
  * frames stored BGR uint8 [H, W, 3], returned RGB float / 255 (GetFrames, :296-311),
  * crop (random, seeded / centre, both snapped to `scale` like AugmentData :368-411 with scale = 1) and the two flips,
    applied identically to frames and event stacks.

The frames take one of two routes to the same bits (ClipDataset(frames=...)): converted and averaged on the host at full
resolution, or -- what the trainers use -- the crop window's rows uploaded as uint8 and turned into the sharp planes and the
blurry mean by one device kernel (ebfi_amd.frameio.period_to_planar).  `batches(..., prefetch=k)` prepares the host half of the
next k batches on a worker thread while the current one trains.

One item = one period (NumPeriodPerLoad = NumPeriodPerSeq = 1, what config/train_ours.yml trains with); the
trainer then runs one optimiser pass per latent frame of the batch exactly like train_ours.py:237-251.

Storage.  A clip is either an `.npz` file with

    images      uint8 [N, H, W, 3]   BGR, like ori_images/image%09d
    event_idx   int64 [N]            index of the first event at / after frame i (the image attribute `<prex>_event_idx`)
    xs, ys      int16 / any [E]      pixel coordinates
    ts          float64 [E]          seconds, sorted
    ps          int8 / any [E]       polarity +-1

and, for an exposure-stamped recording of a real camera (RealBlurClipDataset below), two more arrays

    exposure_begin_t, exposure_end_t   any numeric type [N]   when frame i's shutter opened / closed (the image attributes
                                                              of the same names in the RealBlur-DAVIS files)

or, when `h5py` is importable (it is not part of the MI355X image: the import is optional and a missing module raises a
clear error only when an .h5 file is actually opened), an HDF5 file in the reference's own layout
(`ori_images/image%09d` + attrs `ori_event_idx`, `ori_events/{xs,ys,ts,ps}`), read at scale 1 ('ori').

Recordings of a real camera (`infer_ours.py --real_blur`) go through RealBlurClipDataset, the counterpart of the reference's
second dataset class (dataloader/h5dataset_realdata.py): every stored frame IS a blurry input with its own exposure stamps,
there is no sharp ground truth, and the frame reaches the device as uint8 (ebfi_amd.frameio).
"""
import os
import queue
import random
import threading

import numpy as np
import torch


# ------------------------------------------------------------------------------------------------ host logic (pure numpy)
def period_items(num_imgs, frames_per_period, frames_per_blurry=None, exposure_method="Fixed", exposure_time=None, seed=0):
    """h5dataset.py:118-166 -> list of (latent_indices, blurry_indices, exposure_duty).  The last, possibly incomplete period
    is dropped exactly like `candidates_indices[:-1]` does there (also when num_imgs is a multiple of the period)."""
    P = int(frames_per_period)
    assert P >= 1, "Number of frames per period must >= 1!"
    assert exposure_method in ("Fixed", "Auto", "Custom"), "Error exposure setting!"
    rng = np.random.RandomState(seed)
    starts = np.arange(0, int(num_imgs), P)[:-1]
    items = []
    for j, idx in enumerate(starts):
        if exposure_method == "Fixed":
            e = int(frames_per_blurry)
            assert 1 <= e <= P, "Number of frames per blurry must be in [1, frames per period]!"
        elif exposure_method == "Auto":
            e = int(rng.randint(1, P)) if P > 1 else 1
        else:
            e = int(exposure_time[j % len(exposure_time)])
            assert e <= P, "Number of frames per blurry must <= Number of frames per period!"
        items.append(([int(idx) + i for i in range(P)], [int(idx) + i for i in range(e)], e / P))
    return items


def sequence_items(num_periods, periods_per_seq=1, sliding_window_seq=1, periods_per_load=1, sliding_window_load=1):
    """set_items (h5dataset.py:166-186): the dataset's items are SEQUENCES of loads, a load = [first period, last period].
    Sequence starts step by `sliding_window_seq`; a sequence that would run past the last period is dropped; inside a sequence
    loads start every `sliding_window_load` periods and a load that would cross the sequence's end is dropped.  Returns the
    list of sequences, each a list of (left, right) period indices -- infer_ours.py walks them in this order."""
    S, ws, Lp, wl = int(periods_per_seq), int(sliding_window_seq), int(periods_per_load), int(sliding_window_load)
    assert S >= 1, "Number of period per seq must >= 1!"
    assert 0 <= ws <= S, "Sliding window seq must be in [0, number of period per seq]"
    assert Lp >= 1, "Number of period per Load must >= 1!"
    assert 0 <= wl <= Lp, "Sliding window Load must be in [0, number of period per Load]"
    assert Lp <= S, "Number of period per load must <= Number of period per seq"
    if ws == 0 or wl == 0:
        raise ValueError("a sliding window of 0 never advances (numpy.arange raises in the reference too)")
    seqs = []
    for start in range(0, int(num_periods), ws):
        end = start + S - 1
        if end <= num_periods - 1:
            seqs.append([(i, i + Lp - 1) for i in range(start, end + 1, wl) if i + Lp - 1 <= end])
    return seqs


def add_noise(data, seed, noise_std=1.0, noise_fraction=0.1):
    """add_noise of the reference (h5dataset.py:455-463) on an event stack: `|N(0, std)|` truncated to an integer at a
    `noise_fraction` of the cells, drawn on the HOST from a generator seeded like the reference seeds torch's global one
    (`torch.manual_seed(seed)`; same engine, same draw order: one normal and one uniform per cell over the contiguous shape) --
    bit-identical counts for the same seed (tests/test_clipdata.py, fixture case 'noise').  The sum is formed on data's device."""
    return data + draw_noise(tuple(data.shape), seed, noise_std, noise_fraction).to(data.device)


def draw_noise(shape, seed, noise_std=1.0, noise_fraction=0.1):
    """The host half of `add_noise`: the int32 noise counts of a stack of `shape`, a CPU tensor."""
    g = torch.Generator(device="cpu").manual_seed(int(seed))
    noise = (noise_std * torch.randn(tuple(shape), generator=g)).abs().int()
    if noise_fraction < 1.0:
        noise.masked_fill_(torch.rand(tuple(shape), generator=g) >= noise_fraction, 0)
    return noise


def normalise_events(xs, ys, ts, ps):
    """GetEventsIndex (h5dataset.py:327-336): an empty slice becomes the single event (0, 0, 0, 0); timestamps become
    (t - t0) / (tN - t0 + 1e-6).  Returns float64 arrays (the reference concatenates into one float64 [4, N] tensor)."""
    xs, ys, ts, ps = (np.asarray(v) for v in (xs, ys, ts, ps))
    if len(xs) == 0 or len(ys) == 0 or len(ts) == 0 or len(ps) == 0:
        xs = ys = ts = ps = np.array([0.0])
    ts = ts.astype(np.float64)
    ts = (ts - ts[0]) / (ts[-1] - ts[0] + 1e-6)
    return xs.astype(np.float64), ys.astype(np.float64), ts, ps.astype(np.float64)


def crop_window(h, w, size, mode, scale=1, seed=None):
    """(i, j, th, tw) of AugmentData's random_crop / center_crop (h5dataset.py:369-411); None when the crop is larger than
    the frame (the reference then returns the data unchanged)."""
    th, tw = int(size[0]), int(size[1])
    if th >= h or tw >= w:
        return None
    if mode == "random":
        r = random.Random(seed)
        i, j = r.randint(0, h - th), r.randint(0, w - tw)
    else:
        i, j = int((h - th) / 2), int((w - tw) / 2)
    i, j = int(i // scale) * scale, int(j // scale) * scale
    return i // scale, j // scale, th // scale, tw // scale


def noise_law(noise_mode, noise, hot_pixels):
    """The `noise_mode` / `hot_pixels` arguments of the datasets, checked -> (noise table or None, hot_pixels or None).
    "host" is the reference's draw (`draw_noise`); "device" the counter-based law of ebfi_amd.eventaug, whose table is made
    here once (an empty one when there is no noise: the kernel then only cuts and flips)."""
    if noise_mode not in ("host", "device"):
        raise ValueError("noise_mode must be 'host' or 'device', got %r" % (noise_mode,))
    if hot_pixels is not None:
        if noise_mode != "device":
            raise ValueError("hot_pixels come with the device noise law: pass noise_mode='device' (the reference's host law "
                             "never adds any, h5dataset.py:436)")
        hot_pixels = (float(hot_pixels[0]), float(hot_pixels[1]))
    if noise_mode == "host":
        return None, None
    from .eventaug import noise_table
    if hot_pixels is not None:
        noise_table(hot_pixels[0], 1.0)          # (refuses a bad std now, not at the first item)
    return (noise_table(*noise) if noise is not None else ()), hot_pixels


# ------------------------------------------------------------------------------------------------ storage
class _NpzClip:
    def __init__(self, path):
        z = np.load(path)
        self.images = z["images"]
        self.event_idx = np.asarray(z["event_idx"]).astype(np.int64)
        self.xs, self.ys, self.ts, self.ps = z["xs"], z["ys"], z["ts"], z["ps"]
        if self.images.ndim != 4 or self.images.shape[-1] != 3 or len(self.event_idx) != len(self.images):
            raise ValueError("%s: images must be [N,H,W,3] with one event_idx per image" % path)
        self.num_imgs = int(self.images.shape[0])
        self.resolution = (int(self.images.shape[1]), int(self.images.shape[2]))
        self.path = path
        self.exposure_begin_t, self.exposure_end_t = (np.asarray(z[k]) if k in z.files else None
                                                      for k in ("exposure_begin_t", "exposure_end_t"))
        for k, v in (("exposure_begin_t", self.exposure_begin_t), ("exposure_end_t", self.exposure_end_t)):
            if v is not None and v.shape != (self.num_imgs,):
                raise ValueError("%s: %s must hold one stamp per image, got shape %r" % (path, k, v.shape))

    def frame_bgr(self, i):
        return self.images[i]

    def has_exposure(self):
        return self.exposure_begin_t is not None and self.exposure_end_t is not None

    def exposure(self, i):
        """(exposure_begin_t, exposure_end_t) of frame i, in the stored type."""
        return self.exposure_begin_t[i], self.exposure_end_t[i]

    def events(self, i0, i1):
        a, b = int(self.event_idx[i0]), int(self.event_idx[i1])
        return self.xs[a:b], self.ys[a:b], self.ts[a:b], self.ps[a:b]


class _H5Clip:
    """The reference's file layout at scale 1 (h5dataset.py:31-40, :296-347)."""

    def __init__(self, path):
        try:
            import h5py
        except ImportError as e:          # (absent from the MI355X image)
            raise ImportError("reading %s needs h5py, which is not installed; convert the clip to .npz "
                              "(ebfi_amd.clipdata module docstring)" % path) from e
        self.f = h5py.File(path, "r")
        self.num_imgs = len(self.f["ori_images"].keys())
        self.resolution = tuple(int(v) for v in self.f.attrs["sensor_resolution"].tolist())
        self.path = path

    def frame_bgr(self, i):
        return self.f["ori_images"]["image%09d" % i][:]

    def events(self, i0, i1):
        a = self.f["ori_images"]["image%09d" % i0].attrs["ori_event_idx"]
        b = self.f["ori_images"]["image%09d" % i1].attrs["ori_event_idx"]
        g = self.f["ori_events"]
        return g["xs"][a:b], g["ys"][a:b], g["ts"][a:b], g["ps"][a:b]

    def has_exposure(self):
        attrs = self.f["ori_images"]["image%09d" % 0].attrs if self.num_imgs else {}
        return "exposure_begin_t" in attrs and "exposure_end_t" in attrs

    def exposure(self, i):
        attrs = self.f["ori_images"]["image%09d" % i].attrs          # (h5dataset_realdata.py:215-217)
        return attrs["exposure_begin_t"], attrs["exposure_end_t"]


def open_clip(path):
    return _H5Clip(path) if path.endswith((".h5", ".hdf5")) else _NpzClip(path)


def list_clips(path):
    """A directory (every .npz / .h5 in it, sorted), a text file with one clip path per line (the reference's datalist.txt),
    or one clip file."""
    if os.path.isdir(path):
        return sorted(os.path.join(path, f) for f in os.listdir(path) if f.endswith((".npz", ".h5", ".hdf5")))
    if path.endswith(".txt"):
        with open(path) as fh:
            return [ln.strip() for ln in fh if ln.strip()]
    return [path]


# ------------------------------------------------------------------------------------------------ dataset
class ClipDataset:
    """Items in the reference's key names and shapes for L = NumPeriodPerLoad = 1 (h5dataset.py:283-295):
        SeqLatentF [1, 1, NumF, 3, H, W]   SeqBlurryF [1, 1, 3, H, W]   SeqHREv [1, TB, 2, H, W]
        RelativeLatentTs [1, 1, NumF]      SeqExposureDuty [1, 1, 1]
    The event stack is binned on the device.  frames="host": the frames are converted and averaged at full resolution on the
    host, moved to `device` and cropped there.  frames="device": only the crop window's rows of the stored uint8 frames go up,
    and one kernel (ebfi_amd.frameio.period_to_planar) writes the sharp planes and the blurry mean with the channel reversal,
    the window and the flips folded into the read -- the same bits, at one byte per sample across the bus.

    noise_mode="device": crop, flips and noise of the event stack are one kernel of `finish` (ebfi_amd.eventaug: a counter-based
    law with the host draw's distribution, not its bits) and `prepare` draws nothing; hot_pixels=(std, fraction) then adds
    AugmentData's hot pixels with the item's seed + 4.

    An item is made in two halves: `prepare` is host work only (file reads, the staging buffer, the event list, the noise
    draw of the host law) and may run on a worker thread (`batches(..., prefetch=k)`); `finish` issues the uploads and kernels on the calling
    thread's current stream.  `__getitem__(i, seed)` is `finish(prepare(i, seed))`."""

    def __init__(self, paths, time_bins=16, frames_per_period=16, frames_per_blurry=16, exposure_method="Fixed",
                 exposure_time=None, crop=None, crop_mode="random", flips=False, device="cuda", seed=0,
                 flip_probs=(0.5, 0.5), center_crop=None, noise=None, frames="host", noise_mode="host", hot_pixels=None,
                 neighbours=False):
        """neighbours (the reference's NeedNeighborGT, h5dataset.py:138-147, 219-271): an item also carries
        SeqNeighborF [1, 1, NumF, 2, 3, H, W], the ground-truth neighbours of every latent frame -- what the STGAN adversarial
        loss takes as `input_frames`: neighbour 0 of latent i is latent max(i - 1, 0), neighbour 1 is latent min(i + 1, NumF - 1),
        of the same period.  The reference reads those frames a second time and augments them with the item's seed, i.e. with
        the window and flips of the latent frames; here they are gathers of the finished latent tensor on the device, in both
        loader modes: no extra frame is read or uploaded.
        crop / crop_mode: the first crop of AugmentData's list (RandomCrop when enabled, else CenterCrop); center_crop: a
        CenterCrop applied AFTER a random crop when the config enables both (the reference walks its `augment` list in order,
        h5dataset.py:410-433); flip_probs: (horizontal_prob, vertical_prob) of data_augment.flip; noise: None or
        (noise_std, noise_fraction) of data_augment.noise -- applied to the event stack after crops and flips with the item's
        seed + 3, like AugmentData does ('Noise' sits behind the crops and flips in the shipped `augment` order); noise_mode:
        "host" draws it as the reference does, "device" on the GPU (class docstring); hot_pixels: None or (hot_pixel_std,
        hot_pixel_fraction) of data_augment.hot_pixel, with noise_mode="device" only."""
        self.clips = [open_clip(p) for p in (list_clips(paths) if isinstance(paths, str) else list(paths))]
        if not self.clips:
            raise ValueError("no clips under %r" % (paths,))
        self.time_bins, self.P = int(time_bins), int(frames_per_period)
        self.crop, self.crop_mode, self.flips = crop, crop_mode, bool(flips)
        self.flip_probs, self.center_crop = (float(flip_probs[0]), float(flip_probs[1])), center_crop
        self.noise = None if noise is None else (float(noise[0]), float(noise[1]))
        self.device = torch.device(device)
        if frames not in ("host", "device"):
            raise ValueError("frames must be 'host' or 'device', got %r" % (frames,))
        self.frames = frames
        self.noise_mode = noise_mode
        self.neighbours = bool(neighbours)
        self.noise_table, self.hot_pixels = noise_law(noise_mode, self.noise, hot_pixels)
        self.items = []
        for ci, clip in enumerate(self.clips):
            for it in period_items(clip.num_imgs, frames_per_period, frames_per_blurry, exposure_method, exposure_time, seed + ci):
                self.items.append((ci, it))

    def __len__(self):
        return len(self.items)

    def event_list(self, index):
        """The period's normalised event list (host arrays) -- what GetEventsIndex returns."""
        ci, (latent, _, _) = self.items[index]
        return normalise_events(*self.clips[ci].events(latent[0], latent[-1]))

    def host_item(self, index):
        """Everything of an item that is host work: (sharp [NumF,3,H,W], blurry [3,H,W], normalised event list, duty)."""
        ci, (latent, blurry, duty) = self.items[index]
        clip = self.clips[ci]
        rgb = lambda i: np.ascontiguousarray(clip.frame_bgr(i)[:, :, ::-1])                       # BGR -> RGB
        sharp = torch.from_numpy(np.stack([rgb(i) for i in latent])).permute(0, 3, 1, 2).float() / 255      # [NumF,3,H,W]
        blur = torch.from_numpy(np.stack([rgb(i) for i in blurry]).mean(0)).permute(2, 0, 1).float() / 255   # [3,H,W]
        return sharp, blur, self.event_list(index), duty

    def augment(self, tensors, resolution, seed):
        """Crop and flips of AugmentData, the same window / decision for every tensor of the item."""
        H, W = resolution
        if self.crop is not None:
            win = crop_window(H, W, self.crop, self.crop_mode, 1, seed + 2)
            if win is not None:
                i, j, th, tw = win
                tensors = [v[..., i:i + th, j:j + tw] for v in tensors]
                H, W = th, tw
        if self.center_crop is not None:
            win = crop_window(H, W, self.center_crop, "center", 1, seed + 2)
            if win is not None:
                i, j, th, tw = win
                tensors = [v[..., i:i + th, j:j + tw] for v in tensors]
        if self.flips:
            if random.Random(seed).random() < self.flip_probs[0]:
                tensors = [v.flip(-1) for v in tensors]
            if random.Random(seed + 1).random() < self.flip_probs[1]:
                tensors = [v.flip(-2) for v in tensors]
        return tensors

    def assemble(self, sharp, blur, stack, duty):
        dev = stack.device
        rel_ts = (torch.arange(self.P) / self.P).to(dev)      # integer tensor / int on the HOST, like GetTimestamp (a device
        #                                                       division may differ in the last bit)
        item = {"SeqLatentF": sharp[None, None].contiguous(), "SeqBlurryF": blur[None, None].contiguous(),
                "SeqHREv": stack[None].contiguous(), "RelativeLatentTs": rel_ts[None, None],
                "SeqExposureDuty": torch.tensor([[[duty]]], dtype=torch.float32, device=dev)}
        if self.neighbours:
            item["SeqNeighborF"] = neighbour_frames(sharp)[None, None].contiguous()
        return item

    def window(self, resolution, seed):
        """(i, j, h, w): the crops `augment` applies for this seed, composed into one window of the frame (the whole frame
        when there is no crop or it is not smaller than the frame)."""
        H, W = resolution
        i0 = j0 = 0
        if self.crop is not None:
            win = crop_window(H, W, self.crop, self.crop_mode, 1, seed + 2)
            if win is not None:
                i0, j0, H, W = win
        if self.center_crop is not None:
            win = crop_window(H, W, self.center_crop, "center", 1, seed + 2)
            if win is not None:
                i0, j0, H, W = i0 + win[0], j0 + win[1], win[2], win[3]
        return i0, j0, H, W

    def flip_decisions(self, seed):
        """(horizontal, vertical) as `augment` decides them for this seed."""
        if not self.flips:
            return False, False
        return random.Random(seed).random() < self.flip_probs[0], random.Random(seed + 1).random() < self.flip_probs[1]

    def stage_frames(self, index, window):
        """The window's ROWS of the period's stored frames, uint8 [NumF, h, W, 3] as stored (BGR), gathered into a staging
        buffer: pinned when the device is a GPU (torch's pinned allocator owns it: a block whose upload is still in flight is
        not handed out again), ordinary memory otherwise."""
        ci, (latent, _, _) = self.items[index]
        clip = self.clips[ci]
        i, _, h, _ = window
        shape = (len(latent), h, clip.resolution[1], 3)
        if self.device.type == "cuda":
            with torch.cuda.device(self.device):          # (a worker thread starts on device 0: pin under the right one)
                stage = torch.empty(shape, dtype=torch.uint8, pin_memory=True)
        else:
            stage = torch.empty(shape, dtype=torch.uint8)
        rows = stage.numpy()
        for f, k in enumerate(latent):
            rows[f] = clip.frame_bgr(k)[i:i + h]
        return stage

    def prepare(self, index, seed=None):
        """The host half of an item: no upload, no launch, nothing on a stream (the pinned allocator's own bookkeeping aside),
        so it may run on a worker thread.  -> what `finish` takes.  The blurry frames are the first `num_blur` of the period's
        (period_items)."""
        if seed is None:
            seed = random.randint(0, 2 ** 32)
        ci, (_, blurry, duty) = self.items[index]
        res = self.clips[ci].resolution
        prepared = {"index": index, "seed": seed, "resolution": res, "duty": duty}
        if self.frames == "device":
            win = self.window(res, seed)
            prepared.update(stage=self.stage_frames(index, win), window=win, num_blur=len(blurry), events=self.event_list(index))
        else:
            sharp, blur, events, _ = self.host_item(index)
            prepared.update(sharp=sharp, blur=blur, events=events)
        if self.noise is not None and self.noise_mode == "host":          # (drawn over [L=1, TB, 2, h, w] like the reference)
            prepared["noise"] = draw_noise((1, self.time_bins, 2) + tuple(self.window(res, seed)[2:]), seed + 3, *self.noise)
        return prepared

    def finish(self, prepared):
        """The device half: uploads and kernels on the current stream of the calling thread -> the item dict."""
        from .encodings import events_to_stack
        seed, res, dev = prepared["seed"], prepared["resolution"], self.device
        xs, ys, ts, ps = prepared["events"]
        to = lambda a, dt: torch.from_numpy(a).to(dev, dt)
        stack = events_to_stack(to(xs, torch.float64), to(ys, torch.float64), to(ts, torch.float64), to(ps, torch.float32),
                                self.time_bins, sensor_size=res).transpose(0, 1)                # [TB,2,H,W]
        if self.frames == "device":
            from .frameio import period_to_planar
            _, j, h, w = prepared["window"]
            fh, fv = self.flip_decisions(seed)
            sharp, blur = period_to_planar(prepared["stage"].to(dev, non_blocking=True), prepared["num_blur"],
                                           window=(0, j, h, w), reverse_channels=True, flip_h=fh, flip_v=fv)
            if self.noise_mode == "host":
                stack, = self.augment([stack], res, seed)
        elif self.noise_mode == "host":
            sharp, blur, stack = self.augment([prepared["sharp"].to(dev), prepared["blur"].to(dev), stack], res, seed)
        else:
            sharp, blur = self.augment([prepared["sharp"].to(dev), prepared["blur"].to(dev)], res, seed)
        if self.noise_mode == "device":          # window, flips and noise in one launch; the hot pixels in place behind it
            from .eventaug import add_hot_pixels, augment_events
            stack = augment_events(stack, self.window(res, seed), *self.flip_decisions(seed), seed + 3, self.noise_table)
            if self.hot_pixels is not None:
                add_hot_pixels(stack, seed + 4, *self.hot_pixels)
        if "noise" in prepared:
            stack = (stack[None] + prepared["noise"].to(dev))[0]
        return self.assemble(sharp, blur, stack, prepared["duty"])

    def __getitem__(self, index, seed=None):
        return self.finish(self.prepare(index, seed))


class RealBlurClipDataset:
    """An exposure-stamped recording of a real camera, as the reference's second dataset class reads it
    (dataloader/h5dataset_realdata.py; `infer_ours.py --real_blur`).  A PERIOD is one recorded frame: frame i is the blurry
    input, the events between frame i and frame i + 1 are its event stream, and
    `ExposureDuty = (end_t[i] - begin_t[i]) / (begin_t[i + 1] - begin_t[i])` comes from the stamps (GetTimestamp, :211-223);
    the last frame only closes the last shutter period, so `num_periods = N - 1` (:113).  There is no sharp ground truth.

    One ITEM is one sequence of `sequence_items` -- L loads of one period each -- in the reference's keys and shapes
    (:169-176; no SeqLatentF):
        SeqBlurryF [L, 1, 3, H, W]   SeqHREv [L, TB, 2, H, W]   RelativeLatentTs [L, 1, interp_num]   SeqExposureDuty [L, 1, 1]
    The frame is the stored array WITHOUT channel reversal (GetFrames, :178-189, does not swap, unlike the synthetic-blur
    reader).  It goes to the device as uint8 and becomes planar float there (ebfi_amd.frameio.frames_to_planar), the centre
    crop's window handed to the kernel; the event stack is binned on the device and cropped as in ClipDataset.  Event noise is
    drawn once per item over the whole [L, TB, 2, H, W] stack with the item's seed + 3, as AugmentData does there; with
    noise_mode="device" by the device law (ebfi_amd.eventaug), one launch per load cutting the window and adding the load's part
    of the item's noise field, and hot_pixels=(std, fraction) then adds hot pixels with the item's seed + 4."""

    def __init__(self, path, time_bins=16, interp_num=16, periods_per_seq=2, sliding_window_seq=2, periods_per_load=1,
                 sliding_window_load=1, crop=None, noise=None, device="cuda", noise_mode="host", hot_pixels=None):
        """crop: the CenterCrop size or None; noise: None or (noise_std, noise_fraction) of data_augment.noise; noise_mode /
        hot_pixels: as for ClipDataset."""
        self.clip = open_clip(path) if isinstance(path, str) else path
        if not self.clip.has_exposure():
            raise ValueError("%s: a real-blur clip needs the per-frame stamps exposure_begin_t / exposure_end_t (arrays of the "
                             ".npz layout, image attributes of the HDF5 one); this clip has none" % self.clip.path)
        if int(periods_per_load) != 1:
            raise ValueError("RealBlurClipDataset: one period per load (the model takes one frame), got %r" % (periods_per_load,))
        self.time_bins, self.interp_num = int(time_bins), int(interp_num)
        self.crop = crop
        self.noise = None if noise is None else (float(noise[0]), float(noise[1]))
        self.noise_mode = noise_mode
        self.noise_table, self.hot_pixels = noise_law(noise_mode, self.noise, hot_pixels)
        self.device = torch.device(device)
        self.num_periods = self.clip.num_imgs - 1          # (the last frame only closes the last shutter period)
        self.items = sequence_items(self.num_periods, periods_per_seq, sliding_window_seq, periods_per_load, sliding_window_load)

    def __len__(self):
        return len(self.items)

    def event_list(self, left, right):
        """The load's normalised event list (host arrays): everything from frame `left` up to frame `right + 1`
        (GetEvents, :202-206: '+1 for get all events')."""
        return normalise_events(*self.clip.events(left, right + 1))

    def exposure_duty(self, i):
        """Exposure period over shutter period of frame i (GetTimestamp): the differences in the stored type, the quotient in
        float64 -- the reference's numpy scalars -- rounded to float32 once, by the caller."""
        begin, end = self.clip.exposure(i)
        return float(np.float64(end - begin) / np.float64(self.clip.exposure(i + 1)[0] - begin))

    def timestamps(self):
        return torch.linspace(0, 1, self.interp_num)       # on the HOST, like load_metadata (:112)

    def window(self):
        """(i, j, h, w) of the centre crop, or None when there is none (or it is not smaller than the frame)."""
        return None if self.crop is None else crop_window(*self.clip.resolution, self.crop, "center", 1)

    def host_item(self, index):
        """Everything of an item that is host work: (frames uint8 [L, H, W, 3] as stored, the normalised event list of every
        load, SeqExposureDuty float32 [L, 1, 1], RelativeLatentTs float32 [L, 1, interp_num])."""
        loads = self.items[index]
        frames = np.ascontiguousarray(np.stack([self.clip.frame_bgr(left) for left, _ in loads]))     # (no channel swap)
        duty = torch.tensor([[[self.exposure_duty(left)]] for left, _ in loads], dtype=torch.float64).float()
        return frames, [self.event_list(*ld) for ld in loads], duty, self.timestamps()[None, None].repeat(len(loads), 1, 1)

    def __getitem__(self, index, seed=None):
        from .encodings import events_to_stack
        from .frameio import frames_to_planar
        if seed is None:
            seed = random.randint(0, 2 ** 32)
        dev, res = self.device, self.clip.resolution
        frames, events, duty, rel_ts = self.host_item(index)
        win = self.window()
        blur = frames_to_planar(torch.from_numpy(frames).to(dev), window=win)                # [L,3,h,w]
        to = lambda a, dt: torch.from_numpy(a).to(dev, dt)
        stacks = [events_to_stack(to(xs, torch.float64), to(ys, torch.float64), to(ts, torch.float64), to(ps, torch.float32),
                                  self.time_bins, sensor_size=res).transpose(0, 1) for xs, ys, ts, ps in events]
        if self.noise_mode == "device":
            from .eventaug import add_hot_pixels, augment_events
            h, w = res if win is None else win[2:]
            stack = torch.empty((len(stacks), self.time_bins, 2, h, w), dtype=torch.float32, device=dev)
            for l, s in enumerate(stacks):          # (the noise field is one over the item: each load adds its own cells of it)
                augment_events(s, win, False, False, seed + 3, self.noise_table, out=stack[l], cell_offset=l * stack[l].numel())
            if self.hot_pixels is not None:
                add_hot_pixels(stack, seed + 4, *self.hot_pixels)
        else:
            stack = torch.stack(stacks)                                                      # [L,TB,2,H,W]
            if win is not None:
                i, j, th, tw = win
                stack = stack[..., i:i + th, j:j + tw]
            if self.noise is not None:
                stack = add_noise(stack, seed + 3, *self.noise)
        return {"SeqBlurryF": blur[:, None].contiguous(), "SeqHREv": stack.contiguous(), "RelativeLatentTs": rel_ts.to(dev),
                "SeqExposureDuty": duty.to(dev)}


SUPPORTED_AUGMENT_ORDER = ["RandomCrop", "CenterCrop", "HorizontalFlip", "VertivcalFlip", "Noise", "HotPixel"]


def neighbour_indices(num_frames):
    """[NumF, 2]: the latent indices of a period's neighbours -- (max(i - 1, 0), min(i + 1, NumF - 1)) for latent i
    (h5dataset.py:138-147)."""
    i = torch.arange(int(num_frames))
    return torch.stack([(i - 1).clamp_min(0), (i + 1).clamp_max(int(num_frames) - 1)], 1)


def neighbour_frames(sharp):
    """sharp [NumF, 3, H, W] (a period's latent frames, cropped and flipped) -> [NumF, 2, 3, H, W], gathered where `sharp` lives."""
    idx = neighbour_indices(sharp.shape[0]).to(sharp.device)
    return sharp.index_select(0, idx.reshape(-1)).reshape((sharp.shape[0], 2) + tuple(sharp.shape[1:]))


def dataset_args_from_config(ds_cfg, hot_pixels=False):
    """The reference's `train_dataloader.dataset` keys (config/train_ours.yml:115-150) -> ClipDataset keyword arguments.
    Everything the keys can ask for that this reader does NOT do is refused here instead of being ignored silently
    (round-4 advisory): another `augment` order than the shipped one (crops, then flips, then noise) and scale / ori_scale pairs whose ground truth is not the 'ori' groups of a clip.  Hot pixels are opt-in: the
    reference's own test `type == [...]` (h5dataset.py:436) is never true, so it never adds any and the default skips the
    `hot_pixel` keys; with hot_pixels=True, 'HotPixel' in the `augment` list and `hot_pixel.enabled`, the result carries
    `hot_pixels=(hot_pixel_std, hot_pixel_fraction)` -- the law add_hot_pixels describes, which the datasets draw on the
    device (noise_mode="device")."""
    aug = ds_cfg.get("data_augment") or {}
    out = dict(crop=None, crop_mode="random", center_crop=None, flips=False, flip_probs=(0.5, 0.5), noise=None)
    if ds_cfg.get("NeedNeighborGT"):
        # (the key is only handed on when set: the other dataset classes these arguments reach have no neighbours)
        if ds_cfg.get("DeblurPretrain"):
            raise NotImplementedError("dataset.NeedNeighborGT with DeblurPretrain: the reference then keeps one latent frame per "
                                      "period but the neighbours of all of them; that combination is not implemented")
        out["neighbours"] = True
    # the tensors the model sees come from the reference's `gt_prex` groups (h5dataset.py:36-100): 'ori' exactly when `scale`
    # equals the factor `ori_scale` names -- the shipped pair (2, 'down2') and (1, 'ori') among them; any other pair reads
    # down-scaled groups this reader does not open
    scale, ori = int(ds_cfg.get("scale", 2)), str(ds_cfg.get("ori_scale", "down2"))
    factor = {"ori": 1, "down2": 2, "down4": 4, "down8": 8, "down16": 16}.get(ori)
    if factor is None or scale != factor:
        raise NotImplementedError("dataset.scale %r with ori_scale %r selects the reference's %s ground-truth groups; this reader "
                                  "opens the 'ori' groups only (scale == the factor ori_scale names)" % (scale, ori, "down-scaled"))
    if not aug.get("enabled", False):
        return out
    order = list(aug.get("augment") or SUPPORTED_AUGMENT_ORDER)
    known = [m for m in order if m in SUPPORTED_AUGMENT_ORDER]
    if known != [m for m in SUPPORTED_AUGMENT_ORDER if m in known] or len(known) != len(order):
        raise NotImplementedError("data_augment.augment %r: supported is the shipped order %r (crops before flips) or a "
                                  "sub-list of it" % (order, SUPPORTED_AUGMENT_ORDER))
    hp = aug.get("hot_pixel") or {}
    if hot_pixels and hp.get("enabled") and "HotPixel" in order:          # (defaults of add_hot_pixels, h5dataset.py:446)
        out["hot_pixels"] = (float(hp.get("hot_pixel_std", 1.0)), float(hp.get("hot_pixel_fraction", 0.001)))
    nz = aug.get("noise") or {}
    if nz.get("enabled") and "Noise" in order:          # (h5dataset.py:432-433: defaults of add_noise where a key is absent)
        out["noise"] = (float(nz.get("noise_std", 1.0)), float(nz.get("noise_fraction", 0.1)))
    rc, cc = aug.get("random_crop") or {}, aug.get("center_crop") or {}
    if rc.get("enabled") and "RandomCrop" in order:
        out["crop"], out["crop_mode"] = rc["size"], "random"
        if cc.get("enabled") and "CenterCrop" in order:
            out["center_crop"] = cc["size"]
    elif cc.get("enabled") and "CenterCrop" in order:
        out["crop"], out["crop_mode"] = cc["size"], "center"
    fl = aug.get("flip") or {}
    if fl.get("enabled"):
        ph = float(fl.get("horizontal_prob", 0.5)) if "HorizontalFlip" in order else 0.0
        pv = float(fl.get("vertical_prob", 0.5)) if "VertivcalFlip" in order else 0.0
        out["flips"], out["flip_probs"] = True, (ph, pv)
    return out


def collate(samples):
    return {k: torch.stack([s[k] for s in samples]) for k in samples[0]}


def _prefetched(dataset, plan, depth):
    """Batches of `plan` (an iterator of [(index, item seed), ...] lists) with the host half of up to `depth` batches made
    ahead by ONE worker thread (`dataset.prepare`); the calling thread runs `dataset.finish` and collates, so every GPU call
    stays on the caller's thread and stream.  An exception in the worker is re-raised here at the batch it belongs to; closing
    or exhausting the generator joins the worker."""
    ready, slots, stop = queue.SimpleQueue(), threading.Semaphore(int(depth)), threading.Event()

    def work():
        try:
            for idx in plan:
                slots.acquire()               # one slot per batch in flight, released when the consumer takes the batch
                if stop.is_set():
                    return
                ready.put(([dataset.prepare(i, seed) for i, seed in idx], None))
            ready.put((None, None))
        except BaseException as e:            # (handed over: the consumer raises it after the batches made before it)
            ready.put((None, e))

    worker = threading.Thread(target=work, name="clipdata-prefetch", daemon=True)
    worker.start()
    try:
        while True:
            prepared, err = ready.get()
            if err is not None:
                raise err
            if prepared is None:
                return
            slots.release()
            yield collate([dataset.finish(p) for p in prepared])
    finally:
        stop.set()
        slots.release()
        worker.join()


def _train_plan(n, batch_size, rank, world, seed, epochs, shuffle, drop_last):
    epoch = 0
    while epochs is None or epoch < epochs:
        order = list(range(n))
        if shuffle:
            random.Random(seed + epoch).shuffle(order)
        order = order[rank::world]
        for k in range(0, len(order), batch_size):
            idx = order[k:k + batch_size]
            if len(idx) < batch_size and drop_last:
                break
            yield [(i, seed + 7919 * epoch + i) for i in idx]
        epoch += 1


def batches(dataset, batch_size, rank=0, world=1, seed=0, epochs=None, shuffle=True, drop_last=True, prefetch=0):
    """Per-rank batches: a seeded permutation per epoch split round-robin over ranks (what DistributedSampler does,
    h5dataloader.py:47-57); yields collated dicts [B, L=1, ...].  prefetch = k >= 1: the host half of up to k batches is made
    ahead on a worker thread (`_prefetched`; the dataset needs `prepare` / `finish`); 0: everything on this thread, through
    `dataset.__getitem__`.  The batches are the same either way."""
    plan = _train_plan(len(dataset), batch_size, rank, world, seed, epochs, shuffle, drop_last)
    if prefetch:
        yield from _prefetched(dataset, plan, prefetch)
        return
    for idx in plan:
        yield collate([dataset.__getitem__(i, seed=s) for i, s in idx])


def shard_indices(n, rank, world):
    """Indices of rank `rank` out of `n` items in order, as DistributedSampler(shuffle=False, drop_last=False) deals them: the
    order is padded by wrapping around to ceil(n / world) * world entries and rank r takes every world-th one from r.  Every
    rank gets the same count (so every rank makes the same number of collective calls over its shard) and the union covers
    every index; n = 0 gives no items on any rank."""
    n, rank, world = int(n), int(rank), int(world)
    if not 0 <= rank < world:
        raise ValueError("rank %d outside world %d" % (rank, world))
    if n <= 0:
        return []
    per = -(-n // world)
    return [(rank + k * world) % n for k in range(per)]


def eval_batches(dataset, batch_size, rank=0, world=1, seed=0, drop_last=False, prefetch=0):
    """One pass over `dataset` in file order for validation (the reference's valid_dataloader: no shuffle, DistributedSampler
    shards, h5dataloader.py:47-57): this rank's `shard_indices` in batches of `batch_size`; yields collated dicts [B, L=1, ...].
    The item seeds depend on the index only, so every pass produces the same tensors.  prefetch: as for `batches`."""
    order = shard_indices(len(dataset), rank, world)
    plan = ([(i, seed + i) for i in order[k:k + batch_size]] for k in range(0, len(order), batch_size)
            if not (len(order) - k < batch_size and drop_last))
    if prefetch:
        yield from _prefetched(dataset, plan, prefetch)
        return
    for idx in plan:
        yield collate([dataset.__getitem__(i, seed=s) for i, s in idx])


def model_inputs(batch):
    """The reference's loop over one collated batch (train_ours.py:226-251, L = NumP = 1): yields
    (Frame [B,3,H,W], Event [B,TB,2,H,W], T [B,1], GTEx [B,1], LatentF [B,3,H,W]) per latent frame -- and, when the batch carries
    SeqNeighborF (dataset.NeedNeighborGT), NeighborF [B,2,3,H,W] as a sixth item: the slice the reference's loop keeps commented
    out (train_ours.py:228, 239, 247), the `input_frames` of its Adversarial."""
    latent = batch["SeqLatentF"][:, 0, 0]                 # [B, NumF, 3, H, W]
    neighbour = batch["SeqNeighborF"][:, 0, 0] if "SeqNeighborF" in batch else None       # [B, NumF, 2, 3, H, W]
    frame = batch["SeqBlurryF"][:, 0, 0].contiguous()
    event = batch["SeqHREv"][:, 0].contiguous()
    ts = batch["RelativeLatentTs"][:, 0, 0]               # [B, NumF]
    duty = batch["SeqExposureDuty"][:, 0, 0].contiguous()  # [B, 1]
    for i in range(ts.shape[-1]):
        item = (frame, event, ts[:, [i]].contiguous(), duty, latent[:, i].contiguous())
        yield item if neighbour is None else item + (neighbour[:, i].contiguous(),)


def write_synthetic_clip(path, num_imgs=33, H=64, W=64, events_per_frame=400, seed=0, exposure_stamps=False):
    """A small random clip in the .npz layout (tests, smoke runs of `train_ours.py --data`).  exposure_stamps: also store
    `exposure_begin_t` / `exposure_end_t` (int64 microseconds: a shutter period of about 1/240 s, each frame exposed for 10 to
    90 % of it), which makes the clip readable by RealBlurClipDataset; every other array is the same with and without."""
    g = np.random.RandomState(seed)
    images = g.randint(0, 256, size=(num_imgs, H, W, 3)).astype(np.uint8)
    counts = g.poisson(events_per_frame, size=num_imgs - 1)
    event_idx = np.concatenate([[0], np.cumsum(counts)]).astype(np.int64)
    E = int(event_idx[-1])
    ts = np.sort(g.uniform(0.0, (num_imgs - 1) / 240.0, size=E))
    arrays = dict(images=images, event_idx=event_idx, xs=g.randint(0, W, size=E).astype(np.int16),
                  ys=g.randint(0, H, size=E).astype(np.int16), ts=ts, ps=(g.randint(0, 2, size=E) * 2 - 1).astype(np.int8))
    if exposure_stamps:          # (drawn after everything else, from a generator of their own: the other arrays do not move)
        e = np.random.RandomState(seed + 1)
        period = 1000000 // 240
        begin = (np.arange(num_imgs) * period + e.randint(0, period // 20, size=num_imgs)).astype(np.int64)
        arrays.update(exposure_begin_t=begin,
                      exposure_end_t=begin + e.randint(period // 10, period * 9 // 10, size=num_imgs).astype(np.int64))
    np.savez(path, **arrays)
    return path
