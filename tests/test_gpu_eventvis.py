"""The event-count images on the device (ebfi_amd.eventvis, csrc/eventvis.hip): every output equals the REFERENCE'S OWN
plot_event_cnt bit for bit, through the fixture its function produced (tests/golden/eventvis_small.npz); batches, strided
views, `out=`, repeatability and the C ABI's refusals; seed-generated cases against the numpy restatement that
test_eventvis_host.py holds to the same fixture; and `infer_ours.py --event_png` end to end."""
import ctypes
import importlib.util
import os

import numpy as np
import pytest
import torch

from ebfi_amd import _native as N

import eventvis_ref as R
from test_eventvis_host import CASES

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
PKG = os.path.join(ROOT, "ebfi-be_amd")


@pytest.fixture(scope="module")
def golden(golden_dir):
    return np.load(os.path.join(golden_dir, "eventvis_small.npz"))


def dev(hw2):
    """reference layout H x W x 2 -> contiguous device tensor [1, 2, H, W]"""
    return torch.from_numpy(np.ascontiguousarray(hw2.transpose(2, 0, 1))[None]).cuda()


def images(ev, scheme, black, norm, **kw):
    from ebfi_amd.eventvis import event_count_images
    return event_count_images(ev, color_scheme=scheme, black_background=black, is_norm=norm, **kw)


@pytest.mark.gpu
@pytest.mark.parametrize("name", CASES)
def test_every_fixture_case_in_all_eight_modes(golden, name):
    x = golden[name + "__in"]
    ev = dev(x)
    for scheme, black, norm in R.MODES:
        got = images(ev, scheme, black, norm)
        assert got.dtype == torch.uint8 and tuple(got.shape) == (1,) + x.shape[:2] + (3,) and got.is_cuda
        want = golden[R.mode_key(name, scheme, black, norm)]
        got = got[0].cpu().numpy()
        assert np.array_equal(got, want), (name, scheme, black, norm, int((got != want).sum()), got[got != want][:8], want[got != want][:8])
    assert np.array_equal(ev.cpu().numpy()[0].transpose(1, 2, 0), x)           # the input is read, never written


@pytest.mark.gpu
def test_use_opencv_omits_the_channel_reversal(golden):
    ev = dev(golden["dense8x12__in"])
    a = images(ev, "green_red", False, True).cpu().numpy()
    b = images(ev, "green_red", False, True, use_opencv=True).cpu().numpy()
    assert np.array_equal(a, b[..., ::-1]) and not np.array_equal(a, b)


@pytest.mark.gpu
def test_shim_returns_the_reference_array_and_saves_it(golden, tmp_path):
    from PIL import Image
    from myutils.vis_events.matplotlib_plot_events import event_visualisation
    x = golden["t5x7__in"]
    path = str(tmp_path / "e.png")
    got = event_visualisation().plot_event_cnt(torch.from_numpy(x).cuda(), is_save=True, path=path, color_scheme="blue_red",
                                               is_black_background=False, is_norm=True)
    assert isinstance(got, np.ndarray) and np.array_equal(got, golden[R.mode_key("t5x7", "blue_red", False, True)])
    assert np.array_equal(np.asarray(Image.open(path)), got)
    got = event_visualisation().plot_event_cnt(torch.from_numpy(x).cuda(), is_save=False)      # the reference's defaults
    assert np.array_equal(got, golden[R.mode_key("t5x7", "green_red", True, True)])
    with pytest.raises(NotImplementedError):
        event_visualisation().plot_event_cnt(torch.from_numpy(x).cuda(), is_save=False, color_scheme="gray")


@pytest.mark.gpu
def test_batch_equals_per_image_calls(golden):
    """Four different 8 x 12 pairs in one call (every plane has its own histograms, prefixes and percentiles)."""
    names = ("dense8x12", "negmax8x12", "posmax8x12")
    ev = torch.cat([dev(golden[n + "__in"]) for n in names] + [dev(golden["dense8x12__in"][:, :, ::-1].copy())])
    for scheme, black, norm in R.MODES:
        got = images(ev, scheme, black, norm).cpu().numpy()
        for i, n in enumerate(names):
            assert np.array_equal(got[i], golden[R.mode_key(n, scheme, black, norm)]), (n, scheme, black, norm)
        assert np.array_equal(got[3], images(ev[3:4], scheme, black, norm).cpu().numpy()[0])


@pytest.mark.gpu
def test_strided_views_equal_the_contiguous_result(golden):
    x = golden["sparse136x200__in"]
    want = golden[R.mode_key("sparse136x200", "blue_red", False, True)]
    # a window of a larger tensor: rows start at odd columns, so no row is 16-byte aligned (the scalar path on a wide plane)
    big = torch.full((1, 2, 140, 207), 77.0, device="cuda")
    big[:, :, 3:139, 5:205] = dev(x)
    view = big[:, :, 3:139, 5:205]
    assert not view.is_contiguous() and view.data_ptr() % 16 != 0
    assert np.array_equal(images(view, "blue_red", False, True)[0].cpu().numpy(), want)
    # a [TB, 2, H, W] slice of a [L, TB, 2, H, W] stack, read in place: the pair, an all-zero bin and the polarity-swapped pair
    stack = torch.zeros(2, 3, 2, 136, 200, device="cuda")
    stack[1, 2] = dev(x)[0]
    stack[1, 0] = dev(golden["sparse136x200__in"][:, :, ::-1].copy())[0]
    got = images(stack[1], "blue_red", False, True).cpu().numpy()
    assert np.array_equal(got[2], want)
    assert np.array_equal(got[1], R.plot_event_cnt_numpy(np.zeros_like(x), "blue_red", False, False, True))
    assert np.array_equal(got[0], R.plot_event_cnt_numpy(x[:, :, ::-1], "blue_red", False, False, True))
    # every second bin: an image stride that is not the plane pair's size
    got = images(stack[1, ::2], "green_red", True, True).cpu().numpy()
    assert got.shape[0] == 2 and np.array_equal(got[1], golden[R.mode_key("sparse136x200", "green_red", True, True)])


@pytest.mark.gpu
def test_out_is_written_in_place_and_nothing_behind_it(golden):
    x = golden["t5x7__in"]                                   # 105 bytes: the output ends off every alignment
    buf = torch.full((5 * 7 * 3 + 16,), 0xA5, dtype=torch.uint8, device="cuda")
    out = buf[:105].view(1, 5, 7, 3)
    for norm in (True, False):
        r = images(dev(x), "blue_red", False, norm, out=out)
        assert r.data_ptr() == out.data_ptr() == buf.data_ptr()
        assert np.array_equal(out[0].cpu().numpy(), golden[R.mode_key("t5x7", "blue_red", False, norm)])
        assert (buf[105:] == 0xA5).all()
    big = golden["sparse136x200__in"]                        # the dword-store path
    nb = 136 * 200 * 3
    buf = torch.full((nb + 16,), 0xA5, dtype=torch.uint8, device="cuda")
    images(dev(big), "blue_red", False, True, out=buf[:nb].view(1, 136, 200, 3))
    assert np.array_equal(buf[:nb].view(136, 200, 3).cpu().numpy(), golden[R.mode_key("sparse136x200", "blue_red", False, True)])
    assert (buf[nb:] == 0xA5).all()
    with pytest.raises(ValueError):
        images(dev(x), "blue_red", False, True, out=torch.empty(1, 5, 7, 4, dtype=torch.uint8, device="cuda"))


def _counts_with_noise(rng, h, w):
    ev = rng.poisson(0.35, size=(h, w, 2)).astype(np.float32)
    noisy = rng.random(ev.shape) < 0.05
    ev[noisy] += np.abs(rng.normal(0.0, 1.0, size=int(noisy.sum()))).astype(np.float32)      # fractional counts, like event noise
    return ev


@pytest.mark.gpu
@pytest.mark.parametrize("kind", ["counts72x100", "reals136x200"])
def test_seed_generated_cases_equal_the_host_restatement(kind):
    rng = np.random.default_rng(7)
    if kind == "counts72x100":
        x = _counts_with_noise(rng, 72, 100)
    else:
        x = (10.0 ** rng.uniform(-30.0, 6.0, size=(136, 200, 2))).astype(np.float32)
        x[rng.random(x.shape) < 0.03] *= -1.0
    ev = dev(x)
    for scheme, black, norm in R.MODES:
        got = images(ev, scheme, black, norm)[0].cpu().numpy()
        want = R.plot_event_cnt_numpy(x, scheme, False, black, norm)
        assert np.array_equal(got, want), (kind, scheme, black, norm, int((got != want).sum()))
    again = images(ev, "blue_red", False, True)[0].cpu().numpy()                              # integer counts: repeatable
    assert np.array_equal(again, images(ev, "blue_red", False, True)[0].cpu().numpy())
    assert np.array_equal(again, R.plot_event_cnt_numpy(x, "blue_red", False, False, True))


@pytest.mark.gpu
def test_argument_errors_return_their_codes_and_a_valid_call_still_succeeds(golden):
    lib = N.lib()
    x = golden["dense8x12__in"]
    ev = dev(x)
    out = torch.zeros(1, 8, 12, 3, dtype=torch.uint8, device="cuda")
    need = lib.ebfi_event_cnt_image_workspace(1, 8, 12, 1)
    ws = torch.zeros(need // 8 + 1, dtype=torch.float64, device="cuda")
    st = (ctypes.c_int64 * 3)(*ev.stride()[:3])
    stream = N.stream_ptr(ev.device)
    call = lambda e, s, n, h, w, scheme, o, wsp, nbytes: lib.ebfi_event_cnt_image(e, s, n, h, w, scheme, 0, 1, 0, o, wsp, nbytes, stream)
    assert call(None, st, 1, 8, 12, 0, N.ptr(out), N.ptr(ws), need) == -1
    assert call(N.ptr(ev), st, 1, 8, 12, 0, None, N.ptr(ws), need) == -1
    assert call(N.ptr(ev), st, 1, 0, 12, 0, N.ptr(out), N.ptr(ws), need) == -1
    assert call(N.ptr(ev), st, 1, 8, 0, 0, N.ptr(out), N.ptr(ws), need) == -1
    assert call(N.ptr(ev), st, -1, 8, 12, 0, N.ptr(out), N.ptr(ws), need) == -1
    assert call(N.ptr(ev), st, 1, 8, 12, 0, N.ptr(out), N.ptr(ws), need - 4) == -4
    assert call(N.ptr(ev), st, 1, 8, 12, 0, N.ptr(out), None, 0) == -4
    assert call(N.ptr(ev), st, 1, 8, 12, 2, N.ptr(out), N.ptr(ws), need) == N.EBFI_ERR_UNSUPPORTED
    assert b"gray" in lib.ebfi_last_error()
    torch.cuda.synchronize()
    assert not out.any()                                     # nothing was launched
    assert call(N.ptr(ev), st, 0, 8, 12, 0, N.ptr(out), None, 0) == 0 and not out.any()
    assert call(N.ptr(ev), st, 1, 8, 12, 0, N.ptr(out), N.ptr(ws), need) == 0
    assert np.array_equal(out[0].cpu().numpy(), golden[R.mode_key("dense8x12", "blue_red", False, True)])
    from ebfi_amd.eventvis import event_count_images
    with pytest.raises(N.EbfiNativeError):
        event_count_images(ev, color_scheme="gray")
    assert tuple(event_count_images(ev[:0]).shape) == (0, 8, 12, 3)


# ------------------------------------------------------------------ infer_ours.py --event_png
@pytest.fixture(scope="module")
def cli():
    spec = importlib.util.spec_from_file_location("ebfi_infer_ours_gpu_eventvis", os.path.join(PKG, "infer_ours.py"))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod


@pytest.mark.gpu
def test_infer_ours_event_png_writes_the_fourth_directory(cli, golden_dir, tmp_path):
    """The clip and flags of the metrics CLI test (2 loads, TB = 4): --png --event_png gives the reference's four-directory tree,
    TB files per load in event/, each the native image of that load's stack bin; --png alone has no event/."""
    from PIL import Image
    from ebfi_amd import clipdata
    from ebfi_amd.eventvis import event_count_images
    from test_gpu_infer_metrics import _setup
    clip, args = _setup(tmp_path, golden_dir)
    out = str(tmp_path / "out")
    cli.main(args + ["--output_path", out, "--no-metrics", "--png", "--event_png"])
    img = os.path.join(out, "clip0.npz", "img")
    assert sorted(os.listdir(img)) == ["blurry_frame", "event", "gt_frame", "restored_frame"]
    assert sorted(os.listdir(os.path.join(img, "event"))) == ["%d_TB%09d.png" % (load, b) for load in (0, 1) for b in range(4)]
    data = clipdata.ClipDataset(clip, time_bins=4, frames_per_period=8, frames_per_blurry=3, exposure_method="Fixed", crop=None,
                                crop_mode="center", device="cuda", seed=123, noise=None)
    for load, period in enumerate((0, 1)):
        stack = data.__getitem__(period, seed=123 + period)["SeqHREv"][0]
        assert tuple(stack.shape[:2]) == (4, 2)
        want = event_count_images(stack, "blue_red", black_background=False, is_norm=True).cpu().numpy()
        ref = R.plot_event_cnt_numpy(stack[3].cpu().numpy().transpose(1, 2, 0), "blue_red", False, False, True)
        assert np.array_equal(want[3], ref) and len(np.unique(ref.reshape(-1, 3), axis=0)) > 2        # (a real picture)
        for b in range(4):
            got = np.asarray(Image.open(os.path.join(img, "event", "%d_TB%09d.png" % (load, b))))
            assert np.array_equal(got, want[b]), (load, b)
    out2 = str(tmp_path / "out2")
    cli.main(args + ["--output_path", out2, "--no-metrics", "--png"])
    assert sorted(os.listdir(os.path.join(out2, "clip0.npz", "img"))) == ["blurry_frame", "gt_frame", "restored_frame"]


@pytest.mark.gpu
def test_infer_ours_event_png_with_real_blur(cli, golden_dir, tmp_path):
    """--real_blur --event_png without --png: only event/, TB files for each of the 6 loads."""
    from test_gpu_realblur import _small_checkpoint
    from ebfi_amd.engine import DEFAULT_MODEL_ARGS
    z = np.load(os.path.join(golden_dir, "realblur_small.npz"))
    clip = str(tmp_path / "clip0.npz")
    np.savez(clip, **{k[5:]: z[k] for k in z.files if k.startswith("clip.")})
    lst = str(tmp_path / "test.txt")
    open(lst, "w").write(clip + "\n")
    cfg = dict(DEFAULT_MODEL_ARGS, FrameBasech=16, EventBasech=16, InterCH=16, TB=4, step=2, channels=[4, 4, 8, 8])
    ckpt, _ = _small_checkpoint(tmp_path, cfg)
    out = str(tmp_path / "out")
    cli.main(["--model_path", ckpt, "--data_list", lst, "--output_path", out, "--scale", "1", "--ori_scale", "ori", "--time_bins", "4",
              "--num_period_per_seq", "2", "--sliding_window_seq", "2", "--num_period_per_load", "1", "--sliding_window_load", "1",
              "--center_crop_size", "16", "24", "--real_blur", "--interp_num", "5", "--event_png"])
    img = os.path.join(out, "clip0.npz", "img")
    assert os.listdir(img) == ["event"]
    names = sorted(os.listdir(os.path.join(img, "event")))
    assert names == sorted("%d_TB%09d.png" % (load, b) for load in range(6) for b in range(4))
    from PIL import Image
    assert np.asarray(Image.open(os.path.join(img, "event", names[0]))).shape == (16, 24, 3)
