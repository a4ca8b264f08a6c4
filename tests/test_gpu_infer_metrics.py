"""infer_ours.py scoring its restored frames (PSNR / SSIM / MSE, the reference's inference.yml / inference_all.yml /
inference_all_step.yml) on the clip of the clipdata fixture, with the flags and checkpoint recipe of
test_infer_ours_writes_what_the_oracle_computes; every value checked against the float64 restatement applied to restored.npz
and to the sharp frames rebuilt through clipdata with the script's seeds."""
import importlib.util
import os

import numpy as np
import pytest
import yaml

from test_infer_cli import _small_checkpoint
from test_metrics_host import ref_metrics

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
PKG = os.path.join(ROOT, "ebfi-be_amd")


@pytest.fixture(scope="module")
def cli():
    spec = importlib.util.spec_from_file_location("ebfi_infer_ours_gpu_metrics", os.path.join(PKG, "infer_ours.py"))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod


def _setup(tmp_path, golden_dir):
    from ebfi_amd.engine import DEFAULT_MODEL_ARGS
    z = np.load(os.path.join(golden_dir, "clipdata_small.npz"))
    clip = str(tmp_path / "clip0.npz")
    np.savez(clip, **{k[5:]: z[k] for k in z.files if k.startswith("clip.")})
    lst = str(tmp_path / "test.txt")
    open(lst, "w").write(clip + "\n")
    cfg = dict(DEFAULT_MODEL_ARGS, FrameBasech=16, EventBasech=16, InterCH=16, TB=4, step=2, channels=[4, 4, 8, 8])
    ckpt, _ = _small_checkpoint(tmp_path, cfg)
    args = ["--model_path", ckpt, "--data_list", lst, "--scale", "1", "--ori_scale", "ori", "--time_bins", "4",
            "--num_frame_per_period", "8", "--num_frame_per_blurry", "3", "--num_period_per_seq", "2", "--sliding_window_seq", "2",
            "--num_period_per_load", "1", "--sliding_window_load", "1", "--exposure_method", "Fixed", "--noise_enabled"]
    return clip, args


@pytest.mark.gpu
def test_infer_ours_writes_the_reference_metrics(cli, golden_dir, tmp_path):
    from ebfi_amd import clipdata
    clip, args = _setup(tmp_path, golden_dir)
    out = str(tmp_path / "out")
    cli.main(args + ["--output_path", out])
    res = np.load(os.path.join(out, "clip0.npz", "restored.npz"))
    assert res["psnr"].shape == res["ssim"].shape == res["mse"].shape == (2, 8)
    # the sharp frames of the two loads, rebuilt with the script's seeds
    data = clipdata.ClipDataset(clip, time_bins=4, frames_per_period=8, frames_per_blurry=3, exposure_method="Fixed", crop=None,
                                crop_mode="center", device="cuda", seed=123, noise=None)
    want = [ref_metrics(res["restored"][load], data.__getitem__(period, seed=123 + period)["SeqLatentF"][0, 0].cpu().numpy())
            for load, period in enumerate((0, 1))]
    psnr, ssim, mse = (np.concatenate([w[i] for w in want]) for i in range(3))
    assert np.all(np.isfinite(psnr)) and ssim.std() > 0
    assert np.abs(res["psnr"].ravel() - psnr).max() <= 1e-3
    assert np.abs(res["ssim"].ravel() - ssim).max() <= 1e-4
    assert (np.abs(res["mse"].ravel() - mse) / mse).max() <= 1e-5

    doc = yaml.safe_load(open(os.path.join(out, "clip0.npz", "inference.yml")))
    assert set(doc) == {"info", "evaluation results", "evaluation step results"}
    assert set(doc["evaluation results"]) == {"mse", "psnr", "ssim"}
    step = doc["evaluation step results"]["psnr"]
    assert len(step) == 16
    assert np.abs(np.array(step) - psnr).max() <= 1e-3
    for k, v in (("psnr", psnr), ("ssim", ssim)):
        assert abs(doc["evaluation results"][k] - v.mean()) <= (1e-3 if k == "psnr" else 1e-4)
    assert abs(doc["evaluation results"]["mse"] - mse.mean()) <= 1e-5 * mse.mean()

    all_ = yaml.safe_load(open(os.path.join(out, "inference_all.yml")))
    assert set(all_) == {"info", "breakdown results for each data", "mean results for the whole data"}
    assert all_["breakdown results for each data"]["psnr"] == {"clip0.npz": doc["evaluation results"]["psnr"]}
    assert all_["mean results for the whole data"] == pytest.approx(doc["evaluation results"])
    all_step = yaml.safe_load(open(os.path.join(out, "inference_all_step.yml")))
    assert set(all_step) == {"info", "breakdown results for each data", "mean results for the whole data (based on min length)"}
    assert all_step["breakdown results for each data"]["psnr"]["clip0.npz"] == step
    assert all_step["mean results for the whole data (based on min length)"]["psnr"] == pytest.approx(step)

    # a refused second run leaves the summaries of the first as they were
    before = open(os.path.join(out, "inference_all.yml")).read()
    with pytest.raises(FileExistsError):
        cli.main(args + ["--output_path", out])
    assert open(os.path.join(out, "inference_all.yml")).read() == before


@pytest.mark.gpu
def test_no_metrics_writes_none_of_them(cli, golden_dir, tmp_path):
    _, args = _setup(tmp_path, golden_dir)
    out = str(tmp_path / "out")
    cli.main(args + ["--output_path", out, "--no-metrics"])
    res = np.load(os.path.join(out, "clip0.npz", "restored.npz"))
    assert res["restored"].shape == (2, 8, 3, 24, 32) and "psnr" not in res.files
    assert not os.path.exists(os.path.join(out, "clip0.npz", "inference.yml"))
    assert not any(f.startswith("inference_all") for f in os.listdir(out))
