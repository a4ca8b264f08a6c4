"""`infer_ours.py --real_blur` on the device: RealBlurClipDataset's items against the fixture the reference's own real-data
H5Dataset produced (tests/golden/make_golden_realblur.py), bit for bit, and the script end to end on the fixture clip -- the
restored frames against the CPU oracle at the project's 1e-3 bar, the uint8 output against the download kernel, and the files a
real-blur run must and must not write."""
import importlib.util
import os

import numpy as np
import pytest
import torch

from ebfi_amd import clipdata

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
PKG = os.path.join(ROOT, "ebfi-be_amd")

CFGS = {"crop_noise": dict(crop=[16, 24], noise=(1.0, 0.05)), "plain": dict(crop=None, noise=None)}


@pytest.fixture(scope="module")
def fixture(golden_dir, tmp_path_factory):
    z = np.load(os.path.join(golden_dir, "realblur_small.npz"))
    path = str(tmp_path_factory.mktemp("realclip") / "clip0.npz")
    np.savez(path, **{k[5:]: z[k] for k in z.files if k.startswith("clip.")})
    return z, path


@pytest.fixture(scope="module")
def cli():
    spec = importlib.util.spec_from_file_location("ebfi_infer_ours_real_gpu", os.path.join(PKG, "infer_ours.py"))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod


@pytest.mark.gpu
@pytest.mark.parametrize("tag", ["crop_noise", "plain"])
def test_items_match_the_reference_dataset_on_the_device(fixture, tag):
    """Frame (uint8 upload + the device kernel, crop window included), event stack (device binning, crop, noise over the whole
    sequence at seed + 3), duty and timestamps of every item: the reference's tensors, bit for bit."""
    z, path = fixture
    ds = clipdata.RealBlurClipDataset(path, time_bins=4, interp_num=5, periods_per_seq=2, sliding_window_seq=2, device="cuda",
                                      **CFGS[tag])
    assert len(ds) == int(z["%s.len" % tag]) == 3
    for i in range(len(ds)):
        item = ds.__getitem__(i, seed=5)
        assert sorted(item) == ["RelativeLatentTs", "SeqBlurryF", "SeqExposureDuty", "SeqHREv"]          # no SeqLatentF
        for k, v in item.items():
            ref = z["%s.%d.%s" % (tag, i, k)]
            assert v.is_cuda and v.dtype == torch.float32 and tuple(v.shape) == ref.shape, (k, v.shape, ref.shape)
            assert np.array_equal(v.cpu().numpy(), ref), (tag, i, k)
    if tag == "crop_noise":       # the noise is there, and only adds counts
        clean = clipdata.RealBlurClipDataset(path, time_bins=4, interp_num=5, device="cuda", crop=[16, 24]).__getitem__(0, seed=5)
        assert (item["SeqHREv"] >= 0).all() and ds.__getitem__(0, seed=5)["SeqHREv"].sum() > clean["SeqHREv"].sum()


def _small_checkpoint(tmp_path, cfg):
    from ebfi_amd.model import EVFIAutoEx
    torch.manual_seed(3)
    net = EVFIAutoEx(**cfg)
    with torch.no_grad():
        for p in net.parameters():
            if p.dim() > 1:
                p.copy_(torch.randn_like(p) * (1.2 / p[0].numel() ** 0.5))
            else:
                p.add_(0.05 * torch.randn_like(p))
    path = str(tmp_path / "checkpoint-iteration9.pth")
    torch.save({"model": {"name": "EVFIAutoEx", "states": net.state_dict()}, "config": {"model": {"name": "EVFIAutoEx", "args": cfg}},
                "trainer": {"training_mode": "iteration_based_train", "iteration": 9, "monitor_best": None}}, path)
    return path, {k: v.clone() for k, v in net.state_dict().items()}


@pytest.mark.gpu
def test_infer_ours_real_blur_end_to_end(cli, fixture, tmp_path, capsys):
    """The RealBlur block of the reference's script on the fixture clip (8 frames -> 3 sequences of 2 loads, 5 timestamps per
    load, centre crop 16x24, event noise on): restored.npz holds the uint8 frames, which are the download kernel's cast of the
    float frames; the float frames equal the CPU oracle's `Final` for the same (Frame, Event, T, GTEx) within 1e-3 at the
    timestamps 0, 0.5 and 1 of every load; nothing is scored, so no yml and no gt_frame/."""
    from oracle import model_ref
    from ebfi_amd.engine import DEFAULT_MODEL_ARGS
    from ebfi_amd.frameio import planar_to_u8
    z, clip = fixture
    lst = str(tmp_path / "test.txt")
    open(lst, "w").write(clip + "\n")
    cfg = dict(DEFAULT_MODEL_ARGS, FrameBasech=16, EventBasech=16, InterCH=16, TB=4, step=2, channels=[4, 4, 8, 8])
    ckpt, sd = _small_checkpoint(tmp_path, cfg)
    out = str(tmp_path / "out")
    args = ["--model_path", ckpt, "--data_list", lst, "--output_path", out, "--scale", "1", "--ori_scale", "ori", "--time_bins", "4",
            "--num_period_per_seq", "2", "--sliding_window_seq", "2", "--num_period_per_load", "1", "--sliding_window_load", "1",
            "--center_crop_size", "16", "24", "--real_blur", "--interp_num", "5", "--save_float", "--png"]
    cli.main(args)
    err = capsys.readouterr().err
    assert err.count("real_blur:") == 1 and "nothing is scored" in err
    root = os.path.join(out, "clip0.npz")
    res = np.load(os.path.join(root, "restored.npz"))
    assert sorted(res.files) == ["blurry_u8", "exposure_duty", "period", "restored", "restored_u8", "timestamps"]
    assert res["restored_u8"].shape == (6, 5, 16, 24, 3) and res["restored_u8"].dtype == np.uint8
    assert res["restored"].shape == (6, 5, 3, 16, 24) and res["restored"].dtype == np.float32
    assert res["blurry_u8"].shape == (6, 16, 24, 3) and res["period"].tolist() == [0, 1, 2, 3, 4, 5]
    assert np.array_equal(res["timestamps"], np.tile(np.linspace(0, 1, 5, dtype=np.float32), (6, 1)))
    begin, end = z["clip.exposure_begin_t"], z["clip.exposure_end_t"]
    assert np.array_equal(res["exposure_duty"], ((end[:6] - begin[:6]) / (begin[1:7] - begin[:6])).astype(np.float32))
    # nothing is scored: no yml (or its JSON stand-in) anywhere, no gt_frame/
    written = [f for _, _, files in os.walk(out) for f in files]
    assert not [f for f in written if f.endswith((".yml", ".json"))], written
    img = os.path.join(root, "img")
    assert sorted(os.listdir(img)) == ["blurry_frame", "restored_frame"]
    assert sorted(os.listdir(os.path.join(img, "restored_frame")))[:2] == ["000000000_0.png", "000000001_0.png"]
    assert len(os.listdir(os.path.join(img, "restored_frame"))) == 30 and len(os.listdir(os.path.join(img, "blurry_frame"))) == 6
    from PIL import Image
    assert np.array_equal(np.asarray(Image.open(os.path.join(img, "restored_frame", "000000007_1.png"))), res["restored_u8"][1, 2])
    assert np.array_equal(np.asarray(Image.open(os.path.join(img, "blurry_frame", "000000003.png"))), res["blurry_u8"][3])
    # the uint8 frames are the download kernel's cast of the float frames, exactly
    for load in range(6):
        assert np.array_equal(planar_to_u8(torch.from_numpy(res["restored"][load]).cuda()).cpu().numpy(), res["restored_u8"][load])
    # the same items, rebuilt with the seeds the script uses, through the CPU oracle: one batch of 6 loads x 3 timestamps
    data = clipdata.RealBlurClipDataset(clip, time_bins=4, interp_num=5, periods_per_seq=2, sliding_window_seq=2, crop=[16, 24],
                                        noise=(1.0, 0.05), device="cuda")
    frames, events, duties, stamps, index = [], [], [], [], []
    for si, seq in enumerate(data.items):
        item = data.__getitem__(si, seed=123 + 7919 * si + seq[0][0])
        for idxL in range(len(seq)):
            load = 2 * si + idxL
            frame = item["SeqBlurryF"][idxL].cpu()
            assert np.array_equal(res["blurry_u8"][load], (frame[0].numpy().transpose(1, 2, 0) * 255).astype("uint8"))
            for k in (0, 2, 4):
                frames.append(frame)
                events.append(item["SeqHREv"][idxL:idxL + 1].cpu())
                duties.append(item["SeqExposureDuty"][idxL].cpu())
                stamps.append(torch.full((1, 1), k / 4))
                index.append((load, k))
    ref = model_ref.evfi_forward(sd, cfg, torch.cat(frames), torch.cat(events), torch.cat(stamps), torch.cat(duties))[-1]
    for r, (load, k) in zip(ref, index):
        err = (torch.from_numpy(res["restored"][load, k]) - r).abs().max().item() / r.abs().max().item()
        assert err < 1e-3, (load, k, err)
    assert res["restored"].std() > 1e-3 and res["restored_u8"].std() > 1
    # a second run into the same output directory refuses to overwrite, like the reference's os.makedirs(exist_ok=False)
    with pytest.raises(FileExistsError):
        cli.main(args)
