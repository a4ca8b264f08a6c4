"""ebfi_amd.eventaug on the device (csrc/eventaug.hip: ebfi_event_augment, ebfi_event_hot_pixels) against the numpy restatement
of the law (tests/eventaug_ref.py), bit for bit: the law is integer arithmetic after the host-made table, so there is no
tolerance anywhere in this file.  The source is what the loaders hand over -- the transposed, non-contiguous view of a
[2, TB, H, W] tensor of small integer counts -- at sizes where the kernel takes each of its paths: 16-byte and scalar loads,
quads that straddle rows and planes, a scalar tail, more than one block, both words of the key."""
import numpy as np
import pytest
import torch

import eventaug_ref as R
from ebfi_amd import clipdata, eventaug

pytestmark = pytest.mark.gpu

TB, H, W = 3, 37, 53
WINDOWS = {"whole": None,                        # 53 columns: every row starts at another alignment, quads straddle rows
           "odd_origin": (5, 7, 19, 22),         # odd origin, width not a multiple of 4, Philox groups straddling rows
           "aligned": (4, 8, 16, 32)}            # the 16-byte load path
FLIPS = [(False, False), (True, False), (False, True), (True, True)]
SEEDS = [0, 2 ** 32 + 5]                         # the second reaches the high key word
NOISE = {"sparse": (1.0, 0.05), "dense": (2.5, 1.0), "none": None}


@pytest.fixture(scope="module")
def source():
    """(the device view [TB, 2, H, W] of a [2, TB, H, W] tensor, the same view as a numpy array); never written to."""
    g = np.random.RandomState(7)
    a = g.poisson(0.6, size=(2, TB, H, W)).astype(np.float32)
    dev = torch.from_numpy(a).cuda().transpose(0, 1)
    assert not dev.is_contiguous()
    return dev, a.transpose(1, 0, 2, 3)


def _same_bits(got, want):
    got = got.cpu().numpy()
    assert got.dtype == np.float32 and want.dtype == np.float32 and got.shape == want.shape
    assert np.array_equal(got.view(np.uint32), want.view(np.uint32))


@pytest.mark.parametrize("noise", list(NOISE))
@pytest.mark.parametrize("seed", SEEDS)
@pytest.mark.parametrize("flips", FLIPS)
@pytest.mark.parametrize("window", list(WINDOWS))
def test_augment_kernel_equals_the_restatement(source, window, flips, seed, noise):
    dev, host = source
    win, (fh, fv) = WINDOWS[window], flips
    tab = eventaug.noise_table(*NOISE[noise]) if NOISE[noise] else ()
    before = dev.clone()
    out = eventaug.augment_events(dev, win, fh, fv, seed, tab)
    assert out.is_contiguous() and torch.equal(dev, before)                 # the view was read in place, and only read
    want = R.augment(host, win, fh, fv, seed, list(tab))
    _same_bits(out, want)
    if NOISE[noise]:
        assert (want != R.augment(host, win, fh, fv, seed, [])).any()       # (the case does add noise)
    else:                                    # no table: the slice, the flip copies and .contiguous() of the torch path, bit for bit
        ref = dev if win is None else dev[..., win[0]:win[0] + win[2], win[1]:win[1] + win[3]]
        ref = ref.flip(-1) if fh else ref
        ref = ref.flip(-2) if fv else ref
        assert torch.equal(out, ref.contiguous())


def test_augment_equals_clipdataset_augment_with_crops_and_flips(source):
    """The composed window and the flip decisions of a dataset with both crops, through the kernel with an empty table, against
    ClipDataset.augment on the same view."""
    dev, _ = source
    ds = clipdata.ClipDataset.__new__(clipdata.ClipDataset)
    ds.crop, ds.crop_mode, ds.center_crop, ds.flips, ds.flip_probs = [24, 40], "random", [17, 22], True, (0.5, 0.5)
    seen = set()
    for seed in (5, 1, 0, 3):
        ref, = ds.augment([dev], (H, W), seed)
        out = eventaug.augment_events(dev, ds.window((H, W), seed), *ds.flip_decisions(seed), seed + 3, ())
        assert out.shape == (TB, 2, 17, 22) and torch.equal(out, ref.contiguous())
        seen.add(ds.flip_decisions(seed))
    assert len(seen) == 4


@pytest.mark.parametrize("first", [0, 1, 2, 3, 4098])
def test_a_load_draws_its_own_cells_of_the_items_field(source, first):
    """cell_offset: the first cell's index in the item; a destination that is only 4-byte aligned takes the scalar stores."""
    dev, host = source
    tab = eventaug.noise_table(2.5, 1.0)
    win = (5, 7, 19, 22)
    want = R.augment(host, win, True, False, 11, list(tab), first_cell=first)
    _same_bits(eventaug.augment_events(dev, win, True, False, 11, tab, cell_offset=first), want)
    n = want.size
    buf = torch.full((n + 5,), -1.0, device="cuda")
    out = buf[1:n + 1].view(want.shape)
    assert out.data_ptr() % 16 == 4
    assert eventaug.augment_events(dev, win, True, False, 11, tab, out=out, cell_offset=first) is out
    _same_bits(out, want)
    assert buf[0].item() == -1.0 and (buf[n + 1:] == -1.0).all()             # nothing outside the destination


def test_augment_refuses_what_it_cannot_read(source):
    dev, _ = source
    with pytest.raises(ValueError, match="float32"):
        eventaug.augment_events(dev.double(), None, False, False, 0, ())
    with pytest.raises(ValueError, match="float32"):
        eventaug.augment_events(dev[:, :1], None, False, False, 0, ())
    with pytest.raises(ValueError, match="out must be"):
        eventaug.augment_events(dev, None, False, False, 0, (), out=torch.empty(TB, 2, H, W + 1, device="cuda"))
    with pytest.raises(ValueError, match="strictly decreasing"):
        eventaug.augment_events(dev, None, False, False, 0, (5, 5))
    from ebfi_amd._native import EbfiNativeError
    with pytest.raises(EbfiNativeError, match="window"):
        eventaug.augment_events(dev, (30, 0, 8, 8), False, False, 0, ())
    flat = dev.contiguous()
    with pytest.raises(EbfiNativeError, match="overlap"):
        eventaug.augment_events(flat, None, False, False, 0, (), out=flat)


@pytest.mark.parametrize("shape,fraction", [((6, 19, 22), 0.05), ((6, 2, 2), 2.0)])
def test_hot_pixels_equal_the_restatement(shape, fraction):
    """[6, 2, 2] at fraction 2.0 is eight pixels on four cells: repeated positions are certain, and must accumulate."""
    planes, h, w = shape
    base = np.random.RandomState(3).poisson(0.6, size=shape).astype(np.float32)
    for seed in (4, 2 ** 32 + 9):
        img = R.hot_pixels(h, w, seed, 2.0, fraction)
        amp = R.counts(R.words(np.arange(R.hot_pixel_count(fraction, h, w)), 1, seed)[:, 2], R.table(2.0))
        assert img.sum() == amp.sum() > 0
        if fraction > 1.0:          # more nonzero amplitudes than cells that hold one: some cell holds the sum of two
            assert np.count_nonzero(amp) > np.count_nonzero(img)
        want = base + img.astype(np.float32)[None]
        runs = []
        for _ in range(2):
            stack = torch.from_numpy(base).cuda()
            assert eventaug.add_hot_pixels(stack, seed, 2.0, fraction) is stack
            runs.append(stack)
            _same_bits(stack, want)
        assert torch.equal(runs[0], runs[1])
    stack = torch.from_numpy(base).cuda()
    eventaug.add_hot_pixels(stack, 4, 2.0, 0.0)                              # no pixel: untouched
    _same_bits(stack, base)
    with pytest.raises(ValueError, match="contiguous"):
        eventaug.add_hot_pixels(torch.zeros(6, 4, 8, device="cuda")[..., ::2], 0, 1.0, 0.1)


CLIP = dict(time_bins=3, frames_per_period=4, frames_per_blurry=3, crop=[19, 22], flips=True)


@pytest.mark.parametrize("frames", ["device", "host"])
def test_clip_dataset_in_device_mode(tmp_path, frames):
    path = clipdata.write_synthetic_clip(str(tmp_path / "c.npz"), num_imgs=9, H=37, W=53, events_per_frame=300, seed=1)
    clean = clipdata.ClipDataset(path, frames=frames, **CLIP)
    ds = clipdata.ClipDataset(path, frames=frames, noise=(1.0, 0.05), noise_mode="device", hot_pixels=(2.0, 0.05), **CLIP)
    only_noise = clipdata.ClipDataset(path, frames=frames, noise=(1.0, 0.05), noise_mode="device", **CLIP)
    bare = clipdata.ClipDataset(path, frames=frames, noise_mode="device", **CLIP)
    tab = R.table(1.0, 0.05)
    for index, seed in ((0, 5), (1, 1), (1, 2 ** 32)):
        item, ref = ds.__getitem__(index, seed), clean.__getitem__(index, seed)
        assert sorted(item) == sorted(ref)
        for k in ref:
            if k != "SeqHREv":
                assert torch.equal(item[k], ref[k]), k
        shape = tuple(ref["SeqHREv"].shape)
        assert shape == (1, 3, 2, 19, 22) and item["SeqHREv"].is_contiguous()
        noise = R.noise_field(shape, seed + 3, tab).astype(np.float32)
        hot = R.hot_pixels(19, 22, seed + 4, 2.0, 0.05).astype(np.float32)
        assert noise.any() and hot.any()
        _same_bits(item["SeqHREv"], ref["SeqHREv"].cpu().numpy() + noise + hot)
        _same_bits(only_noise.__getitem__(index, seed)["SeqHREv"], ref["SeqHREv"].cpu().numpy() + noise)
        assert torch.equal(bare.__getitem__(index, seed)["SeqHREv"], ref["SeqHREv"])
        assert torch.equal(ds.__getitem__(index, seed)["SeqHREv"], item["SeqHREv"])              # the same seed: the same item
    a, b = ds.__getitem__(1, 7)["SeqHREv"], ds.__getitem__(1, 8)["SeqHREv"]
    assert a.shape == b.shape and not torch.equal(a, b)                                          # another seed: another stack
    # through the prefetching generator: the halves compose to the same items
    got = list(clipdata.eval_batches(ds, 2, seed=3, prefetch=1))
    want = list(clipdata.eval_batches(ds, 2, seed=3, prefetch=0))
    assert len(got) == len(want) == 1 and all(torch.equal(got[0][k], want[0][k]) for k in want[0])


def test_real_blur_dataset_in_device_mode(tmp_path):
    """Two loads per item: one noise field over [L, TB, 2, h, w], each load adding its own cells of it."""
    path = clipdata.write_synthetic_clip(str(tmp_path / "r.npz"), num_imgs=5, H=37, W=53, events_per_frame=300, seed=2,
                                         exposure_stamps=True)
    kw = dict(time_bins=3, interp_num=4, crop=[19, 21])
    clean = clipdata.RealBlurClipDataset(path, **kw)
    ds = clipdata.RealBlurClipDataset(path, noise=(2.5, 0.5), noise_mode="device", hot_pixels=(2.0, 0.05), **kw)
    assert len(ds) == 2
    for index, seed in ((0, 5), (1, 2 ** 32 + 1)):
        item, ref = ds.__getitem__(index, seed), clean.__getitem__(index, seed)
        for k in ref:
            if k != "SeqHREv":
                assert torch.equal(item[k], ref[k]), k
        shape = tuple(ref["SeqHREv"].shape)
        assert shape == (2, 3, 2, 19, 21)                                     # 2394 cells a load: the second starts mid-group
        want = ref["SeqHREv"].cpu().numpy() + R.noise_field(shape, seed + 3, R.table(2.5, 0.5)).astype(np.float32) \
            + R.hot_pixels(19, 21, seed + 4, 2.0, 0.05).astype(np.float32)
        _same_bits(item["SeqHREv"], want)
