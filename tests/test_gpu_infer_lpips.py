"""infer_ours.py with --lpips_lin / --lpips_backbone: LPIPS scored as the reference's fourth metric, on the clip of the clipdata
fixture with every pixel repeated 2 x 2 (48 x 64: AlexNet's trunk needs H, W >= 31) and the flags and checkpoint recipe of
test_gpu_infer_metrics; every value checked against the float64 restatement applied to restored.npz and to the sharp frames
rebuilt through clipdata with the script's seeds, and psnr / ssim / mse checked equal to a run without the flags."""
import importlib.util
import os

import numpy as np
import pytest
import torch
import yaml

from test_infer_cli import _small_checkpoint
from test_lpips_host import ref_lpips, write_weights

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
PKG = os.path.join(ROOT, "ebfi-be_amd")


@pytest.fixture(scope="module")
def cli():
    spec = importlib.util.spec_from_file_location("ebfi_infer_ours_gpu_lpips", os.path.join(PKG, "infer_ours.py"))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod


def _setup(tmp_path, golden_dir):
    from ebfi_amd.engine import DEFAULT_MODEL_ARGS
    z = np.load(os.path.join(golden_dir, "clipdata_small.npz"))
    c = {k[5:]: z[k] for k in z.files if k.startswith("clip.")}
    c["images"] = np.repeat(np.repeat(c["images"], 2, axis=1), 2, axis=2)
    c["xs"], c["ys"] = c["xs"] * 2, c["ys"] * 2
    clip = str(tmp_path / "clip0.npz")
    np.savez(clip, **c)
    lst = str(tmp_path / "test.txt")
    open(lst, "w").write(clip + "\n")
    cfg = dict(DEFAULT_MODEL_ARGS, FrameBasech=16, EventBasech=16, InterCH=16, TB=4, step=2, channels=[4, 4, 8, 8])
    ckpt, _ = _small_checkpoint(tmp_path, cfg)
    args = ["--model_path", ckpt, "--data_list", lst, "--scale", "1", "--ori_scale", "ori", "--time_bins", "4",
            "--num_frame_per_period", "8", "--num_frame_per_blurry", "3", "--num_period_per_seq", "2", "--sliding_window_seq", "2",
            "--num_period_per_load", "1", "--sliding_window_load", "1", "--exposure_method", "Fixed", "--noise_enabled"]
    return clip, args


@pytest.mark.gpu
def test_infer_ours_scores_lpips(cli, golden_dir, tmp_path, capsys):
    from ebfi_amd import clipdata
    clip, args = _setup(tmp_path, golden_dir)
    lin_path, backbone_path, (ws, bs, heads) = write_weights(tmp_path)
    out = str(tmp_path / "out")
    cli.main(args + ["--output_path", out, "--lpips_lin", lin_path, "--lpips_backbone", backbone_path])
    assert "LPIPS is not computed" not in capsys.readouterr().err
    plain = str(tmp_path / "plain")
    cli.main(args + ["--output_path", plain])
    assert "LPIPS is not computed" in capsys.readouterr().err

    res = np.load(os.path.join(out, "clip0.npz", "restored.npz"))
    ref = np.load(os.path.join(plain, "clip0.npz", "restored.npz"))
    assert res["restored"].shape == (2, 8, 3, 48, 64) and res["lpips"].shape == (2, 8)
    assert "lpips" not in ref.files
    for k in ("restored", "psnr", "ssim", "mse"):
        assert np.array_equal(res[k], ref[k]), k

    data = clipdata.ClipDataset(clip, time_bins=4, frames_per_period=8, frames_per_blurry=3, exposure_method="Fixed", crop=None,
                                crop_mode="center", device="cuda", seed=123, noise=None)
    want = np.concatenate([ref_lpips(torch.from_numpy(res["restored"][load]),
                                     data.__getitem__(period, seed=123 + period)["SeqLatentF"][0, 0].cpu(), ws, bs, heads)[0].numpy()
                           for load, period in enumerate((0, 1))])
    got = res["lpips"].ravel().astype(np.float64)
    assert np.all(want > 0) and want.std() > 0
    assert np.all(np.abs(got - want) <= 1e-5 + 1e-4 * np.abs(want)), (got, want)

    doc = yaml.safe_load(open(os.path.join(out, "clip0.npz", "inference.yml")))
    doc0 = yaml.safe_load(open(os.path.join(plain, "clip0.npz", "inference.yml")))
    assert set(doc["evaluation results"]) == {"mse", "psnr", "ssim", "lpips"}
    assert abs(doc["evaluation results"]["lpips"] - want.mean()) <= 1e-5 + 1e-4 * want.mean()
    for k in ("mse", "psnr", "ssim"):
        assert doc["evaluation results"][k] == doc0["evaluation results"][k]
    assert doc["evaluation step results"] == doc0["evaluation step results"]

    all_ = yaml.safe_load(open(os.path.join(out, "inference_all.yml")))
    assert all_["breakdown results for each data"]["lpips"] == {"clip0.npz": doc["evaluation results"]["lpips"]}
    assert all_["mean results for the whole data"] == pytest.approx(doc["evaluation results"])
    all0 = yaml.safe_load(open(os.path.join(plain, "inference_all.yml")))
    assert "lpips" not in all0["mean results for the whole data"]
    all_step = yaml.safe_load(open(os.path.join(out, "inference_all_step.yml")))
    assert all_step["breakdown results for each data"] == \
        yaml.safe_load(open(os.path.join(plain, "inference_all_step.yml")))["breakdown results for each data"]


@pytest.mark.gpu
def test_no_metrics_leaves_the_lpips_flags_unused(cli, golden_dir, tmp_path, capsys):
    _, args = _setup(tmp_path, golden_dir)
    out = str(tmp_path / "out")
    cli.main(args + ["--output_path", out, "--no-metrics", "--lpips_lin", "missing.pth", "--lpips_backbone", "missing.pth"])
    assert "unused" in capsys.readouterr().err
    res = np.load(os.path.join(out, "clip0.npz", "restored.npz"))
    assert "lpips" not in res.files and "psnr" not in res.files
