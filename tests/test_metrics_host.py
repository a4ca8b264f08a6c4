"""Evaluation metrics (ebfi_amd.metrics, ebfi_image_metrics): the numpy float64 restatement of their definitions -- the
reference's psnr_loss / ssim_loss (loss/restore.py:43-92, scikit-image's PSNR and structural_similarity defaults) and
nn.MSELoss -- checked against hand-derivable answers, plus what needs no GPU: the entry points' argument errors, the workspace
query, the per-step aggregation and result files of infer_ours.py and its --no-metrics flag.

`ref_metrics` is the restatement the GPU tests compare the kernel with (no scipy / scikit-image: box sums via cumulative sums)."""
import ctypes
import importlib.util
import json
import os
import sys

import numpy as np
import pytest
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
PKG = os.path.join(ROOT, "ebfi-be_amd")


# ------------------------------------------------------------------ the restatement
def box7(a):
    """Sums of every 7x7 window lying fully inside the 2-D array a: [H - 6, W - 6]."""
    c = np.zeros((a.shape[0] + 1, a.shape[1] + 1))
    c[1:, 1:] = np.cumsum(np.cumsum(a, 0), 1)
    return c[7:, 7:] - c[:-7, 7:] - c[7:, :-7] + c[:-7, :-7]


def ssim_parts(x, y, data_range=2.0):
    """Luminance and contrast-structure maps of scikit-image's SSIM (7x7 uniform window, sample covariance) over the interior
    pixels [3, H-3) x [3, W-3) of one plane; the SSIM map is their product."""
    x, y = np.asarray(x, np.float64), np.asarray(y, np.float64)
    c1, c2 = (0.01 * data_range) ** 2, (0.03 * data_range) ** 2
    ux, uy = box7(x) / 49, box7(y) / 49
    norm = 49.0 / 48.0
    vx = norm * (box7(x * x) / 49 - ux * ux)
    vy = norm * (box7(y * y) / 49 - uy * uy)
    vxy = norm * (box7(x * y) / 49 - ux * uy)
    return (2 * ux * uy + c1) / (ux * ux + uy * uy + c1), (2 * vxy + c2) / (vx + vy + c2)


def ref_metrics(pred, target, data_range=2.0):
    """(psnr, ssim, mse), float64 arrays [N], of pred vs target [N, C, H, W] as the reference scores one frame per call."""
    pred, target = np.asarray(pred, np.float64), np.asarray(target, np.float64)
    N, C = pred.shape[:2]
    psnr, ssim, mse = np.zeros(N), np.zeros(N), np.zeros(N)
    with np.errstate(divide="ignore", invalid="ignore"):
        for n in range(N):
            x, y = pred[n], target[n]
            ssim[n] = np.mean([np.mean(np.prod(ssim_parts(x[c], y[c], data_range), axis=0)) for c in range(C)])
            mse[n] = np.mean((x - y) ** 2)
            if C == 1:
                psnr[n] = 10 * np.log10(1.0 / np.mean((np.clip(y[0], 0, 1) - np.clip(x[0], 0, 1)) ** 2))
            else:
                tmin = y.min()
                psnr[n] = np.mean([10 * np.log10((y[c].max() - tmin) ** 2 / np.mean((y[c] - x[c]) ** 2)) for c in range(C)])
    return psnr, ssim, mse


# ------------------------------------------------------------------ the restatement against hand-derived answers
def test_identical_images():
    t = np.random.default_rng(0).random((2, 3, 12, 15))
    psnr, ssim, mse = ref_metrics(t, t)
    assert np.all(np.isposinf(psnr)) and np.allclose(ssim, 1.0, atol=1e-12) and np.all(mse == 0)


def test_constant_offset():
    rng = np.random.default_rng(1)
    t = rng.random((1, 3, 16, 20))
    d = 0.05
    psnr, ssim, mse = ref_metrics(t + d, t)
    assert np.isclose(mse[0], d * d, rtol=1e-12)
    dr = t[0].reshape(3, -1).max(1) - t[0].min()
    assert np.isclose(psnr[0], np.mean(10 * np.log10(dr ** 2 / d ** 2)), rtol=1e-12)
    for c in range(3):
        lum, cs = ssim_parts(t[0, c] + d, t[0, c])
        assert np.allclose(cs, 1.0, atol=1e-12)            # same variance, covariance = variance: structure/contrast exactly 1
        assert np.all(lum < 1.0)
        ux = box7(t[0, c]) / 49
        assert np.allclose(lum, (2 * (ux + d) * ux + 4e-4) / ((ux + d) ** 2 + ux ** 2 + 4e-4), atol=1e-12)


def test_psnr_data_range_mixes_channel_max_with_all_channel_min():
    t = np.zeros((1, 3, 8, 8))
    t[0, 0] = 0.5
    t[0, 0, 0, 0] = 0.9               # channel 0: max 0.9
    t[0, 1] = 0.4                      # channel 1: max 0.4
    t[0, 2] = 0.3
    t[0, 2, 1, 1] = 0.1                # the all-channel min 0.1 sits in channel 2; channel 2 max 0.3
    p = t.copy()
    p[0, :, 4, 4] += 0.2               # one pixel off by 0.2 in every channel: mse_c = 0.04 / 64
    psnr, _, _ = ref_metrics(p, t)
    mse_c = 0.04 / 64
    want = np.mean([10 * np.log10(dr ** 2 / mse_c) for dr in (0.9 - 0.1, 0.4 - 0.1, 0.3 - 0.1)])
    assert np.isclose(psnr[0], want, rtol=1e-12)


def test_one_channel_branch_clips_and_uses_range_one():
    t = np.full((1, 1, 9, 9), 0.5)
    p = t.copy()
    p[0, 0, 2, 2] = 1.7                # clipped to 1: error 0.5 for PSNR, 1.2 for MSE
    p[0, 0, 3, 3] = -0.4               # clipped to 0: error 0.5 for PSNR, 0.9 for MSE
    psnr, _, mse = ref_metrics(p, t)
    assert np.isclose(psnr[0], 10 * np.log10(1.0 / (2 * 0.25 / 81)), rtol=1e-12)
    assert np.isclose(mse[0], (1.2 ** 2 + 0.9 ** 2) / 81, rtol=1e-12)


def test_nan_reaches_only_its_frame():
    rng = np.random.default_rng(2)
    t = rng.random((3, 3, 10, 10))
    p = t + 0.01 * rng.standard_normal(t.shape)
    p[1, 2, 5, 5] = np.nan
    got = ref_metrics(p, t)
    for v in got:
        assert np.isnan(v[1]) and np.all(np.isfinite(v[[0, 2]]))


# ------------------------------------------------------------------ the C ABI without a device
@pytest.fixture(scope="module")
def lib():
    from ebfi_amd import _native as N
    if not os.path.exists(N.LIB_PATH):
        N.build()
    return N.lib()


def test_workspace_query_is_host_arithmetic(lib):
    # one 48-byte partial per (plane, strip of 128 columns, strip of <= 48 rows)
    assert lib.ebfi_image_metrics_workspace(16, 3, 720, 1280) == 16 * 3 * 10 * 15 * 48
    assert lib.ebfi_image_metrics_workspace(1, 1, 7, 7) == 48
    assert lib.ebfi_image_metrics_workspace(5, 3, 37, 129) == 5 * 3 * 2 * 1 * 48
    assert lib.ebfi_image_metrics_workspace(1, 0, 7, 7) == 0


def test_argument_errors_do_not_touch_the_gpu(lib):
    from ebfi_amd import _native as N
    st = N.i64x4((3 * 64, 64, 8, 1))
    fake = ctypes.c_void_p(4096)                       # never dereferenced: every check below fails before a launch
    big = 1 << 20

    def call(pred=fake, target=fake, H=8, W=8, ws=fake, ws_bytes=big, out=fake, strides=st, R=2.0):
        return lib.ebfi_image_metrics(pred, strides, target, strides, 1, 3, H, W, R, ws, ws_bytes, out, out, out, None)

    assert call(pred=None) == -1 and b"null" in lib.ebfi_last_error()
    assert call(target=None) == -1
    assert call(ws=None) == -1
    assert call(out=None) == -1
    assert call(H=6) == -1 and b"H, W >= 7" in lib.ebfi_last_error()
    assert call(W=6) == -1
    assert call(R=0.0) == -1
    assert call(strides=N.i64x4((3 * 64, 64, 8, 2))) == -3          # non-unit column stride: EBFI_ERR_UNSUPPORTED
    assert call(ws_bytes=lib.ebfi_image_metrics_workspace(1, 3, 8, 8) - 1) == -4
    assert b"workspace" in lib.ebfi_last_error()


def test_frame_metrics_refuses_cpu_tensors():
    from ebfi_amd.metrics import frame_metrics
    with pytest.raises(NotImplementedError):
        frame_metrics(torch.rand(1, 3, 8, 8), torch.rand(1, 3, 8, 8))


def test_perceptual_loss_says_why():
    from loss import perceptual_loss
    with pytest.raises(NotImplementedError, match="LPIPS"):
        perceptual_loss(net="alex")


def test_metric_tracker_averages_like_the_reference():
    from ebfi_amd.metrics import MetricTracker
    t = MetricTracker(["mse", "psnr"])
    for v in (30.0, 32.0, 37.0):
        t.update("psnr", v)
    t.update("mse", 0.5, n=3)
    assert t.result() == {"mse": 0.5, "psnr": 33.0} and t.avg("psnr") == 33.0


# ------------------------------------------------------------------ infer_ours.py: flags, aggregation, result files
@pytest.fixture(scope="module")
def cli():
    spec = importlib.util.spec_from_file_location("ebfi_infer_ours_metrics", os.path.join(PKG, "infer_ours.py"))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod


def test_no_metrics_flag_and_reference_command_line(cli):
    from test_infer_cli import REFERENCE_ARGS
    f = cli.get_flags(REFERENCE_ARGS)
    assert f.no_metrics is False
    assert cli.dataset_settings(f)[1] == []
    assert cli.get_flags(REFERENCE_ARGS + ["--no-metrics"]).no_metrics is True


def test_mean_per_step_over_the_shortest_list(cli):
    assert cli.mean_per_step([[1.0, 2.0, 3.0], [3.0, 4.0], [5.0, 6.0, 7.0, 8.0]]) == [3.0, 4.0]
    assert cli.mean_per_step([]) == []


def test_summaries_and_writer(cli, tmp_path, monkeypatch):
    results = [("a.npz", {"mse": 0.01, "psnr": 30.0, "ssim": 0.9}, {"psnr": [29.0, 31.0, 33.0]}),
               ("b.npz", {"mse": 0.03, "psnr": 26.0, "ssim": 0.7}, {"psnr": [25.0, 27.0]})]
    all_, all_step = cli.summarise_clips(results, "inference x")
    assert all_["breakdown results for each data"]["psnr"] == {"a.npz": 30.0, "b.npz": 26.0}
    assert all_["mean results for the whole data"] == pytest.approx({"mse": 0.02, "psnr": 28.0, "ssim": 0.8})
    assert all_step["breakdown results for each data"]["psnr"]["b.npz"] == [25.0, 27.0]
    assert all_step["mean results for the whole data (based on min length)"] == {"psnr": [27.0, 29.0]}
    import yaml
    path = cli.write_results(str(tmp_path / "inference_all.yml"), all_)
    assert path.endswith(".yml") and yaml.safe_load(open(path)) == all_
    monkeypatch.setitem(sys.modules, "yaml", None)            # PyYAML missing: the same dict as JSON
    path = cli.write_results(str(tmp_path / "inference_all_step.yml"), all_step)
    assert path.endswith("inference_all_step.json") and json.load(open(path)) == all_step
