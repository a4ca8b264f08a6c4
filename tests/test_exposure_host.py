"""Host-side checks of the stage-1 (ExposureDecision pre-training) path: the duty-head entries of the C ABI, the command line and
the shipped config of train_ours_exposuredecision.py, its settings helpers, the refused names, and the checkpoint contract with
stage 2 (EVFIAutoEx(LoadPretrainEX=True)).  No GPU.  `ref_duty_head` is the float64 restatement the GPU tests import."""
import ctypes
import math
import os

import numpy as np
import pytest
import torch
import yaml

from ebfi_amd import _native as N

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CONFIG = os.path.join(ROOT, "ebfi-be_amd", "config", "train_ours_exposuredecision.yml")
DUTY_SYMBOLS = ("ebfi_duty_head_workspace", "ebfi_duty_head_forward", "ebfi_duty_head_backward")


def ref_duty_head(ex, duty=None, scale=1.0):
    """float64 restatement of the duty head and its loss (reference model_singleframe.py:75-76 + nn.MSELoss / accu_step):
    ex [B, 1, H, W], duty [B] or [B, 1] -> (Ex [B], loss) with Ex = sigmoid(mean over H, W), loss = scale * mean((Ex - duty)^2);
    loss is None without a duty."""
    ex = np.asarray(ex, dtype=np.float64)
    mean = ex.reshape(ex.shape[0], -1).mean(axis=1)
    Ex = 1.0 / (1.0 + np.exp(-mean))
    if duty is None:
        return Ex, None
    d = np.asarray(duty, dtype=np.float64).reshape(-1)
    return Ex, float(scale) * np.mean((Ex - d) ** 2)


def ref_duty_head_grad(ex, duty, scale, g):
    """d(g * loss) / d ex of `ref_duty_head` in float64: constant over each plane."""
    ex = np.asarray(ex, dtype=np.float64)
    B, hw = ex.shape[0], ex.shape[2] * ex.shape[3]
    Ex, _ = ref_duty_head(ex, duty, scale)
    d = np.asarray(duty, dtype=np.float64).reshape(-1)
    coef = g * scale * 2.0 * (Ex - d) / B * Ex * (1.0 - Ex) / hw
    return np.broadcast_to(coef[:, None, None, None], ex.shape).copy()


def test_ref_duty_head_matches_torch_autograd():
    """The restatement against torch's own float64 pooling + sigmoid + MSELoss and its autograd."""
    g = torch.Generator().manual_seed(3)
    ex = (torch.rand(3, 1, 5, 7, generator=g, dtype=torch.float64) * 8 - 4).requires_grad_(True)
    duty = torch.tensor([[0.25], [0.5], [0.9375]], dtype=torch.float64)
    Ex = torch.sigmoid(torch.nn.AdaptiveAvgPool2d(1)(ex).view(-1, 1))
    loss = torch.nn.MSELoss()(Ex, duty) * 0.5
    (loss * 2.5).backward()
    rEx, rloss = ref_duty_head(ex.detach().numpy(), duty.numpy(), 0.5)
    assert np.allclose(rEx, Ex.detach().numpy().ravel(), rtol=1e-14, atol=0)
    assert math.isclose(rloss, loss.item(), rel_tol=1e-13)
    assert np.allclose(ref_duty_head_grad(ex.detach().numpy(), duty.numpy(), 0.5, 2.5), ex.grad.numpy(), rtol=1e-12, atol=0)
    assert ref_duty_head(ex.detach().numpy())[1] is None


# ------------------------------------------------------------------------------------------------ C ABI
def test_duty_head_symbols_declared_bound_and_exported():
    declared = N.declared_symbols()
    for name in DUTY_SYMBOLS:
        assert name in declared and name in N.SIGNATURES, name
    if not os.path.exists(N.LIB_PATH):
        N.build()
    h = ctypes.CDLL(N.LIB_PATH)
    for name in DUTY_SYMBOLS:
        assert hasattr(h, name), name
    header = open(os.path.join(ROOT, "include", "ebfi_hip.h")).read()
    assert "#define EBFI_ABI_VERSION 14" in header and N.ABI_VERSION == 14 and N.lib().ebfi_abi_version() == 14


def test_duty_head_workspace_and_argument_errors():
    """Pure host arithmetic: one fp64 partial per tile of ceil(4096 / W) rows; bad arguments are refused before any launch."""
    lib = N.lib()
    assert lib.ebfi_duty_head_workspace(1, 1, 1) == 8
    assert lib.ebfi_duty_head_workspace(2, 64, 64) == 2 * 1 * 8
    assert lib.ebfi_duty_head_workspace(2, 720, 1280) == 2 * 180 * 8          # R = 4 rows
    assert lib.ebfi_duty_head_workspace(3, 37, 129) == 3 * 2 * 8              # R = 32 rows
    assert lib.ebfi_duty_head_workspace(-1, 4, 4) == 0 and lib.ebfi_duty_head_workspace(1, 0, 4) == 0
    p = ctypes.c_void_p(16)
    st = N.i64x4((16, 16, 4, 1))
    assert lib.ebfi_duty_head_forward(None, st, p, 1, 4, 4, 1.0, p, 64, p, p, None) == -1
    assert b"null" in lib.ebfi_last_error()
    assert lib.ebfi_duty_head_forward(p, N.i64x4((16, 16, 4, 2)), p, 1, 4, 4, 1.0, p, 64, p, p, None) == -3
    assert b"column stride" in lib.ebfi_last_error()
    assert lib.ebfi_duty_head_forward(p, st, p, 1, 4, 4, 1.0, p, 0, p, p, None) == -4
    assert lib.ebfi_duty_head_forward(p, st, p, 1, 4, 4, 1.0, ctypes.c_void_p(8), 64, p, p, None) == -1
    assert lib.ebfi_duty_head_forward(p, st, p, 1, 4, 4, 1.0, p, 64, p, None, None) == -1      # a duty without loss_out
    assert lib.ebfi_duty_head_backward(p, p, None, 1, 4, 4, 1.0, p, None) == -1
    assert lib.ebfi_duty_head_backward(p, p, p, 1, 0, 4, 1.0, p, None) == -1


def test_duty_loss_refuses_cpu_tensors():
    from ebfi_amd.loss import DutyMSELoss, duty_head
    with pytest.raises(NotImplementedError):
        DutyMSELoss()(torch.zeros(2, 1, 4, 4), torch.zeros(2, 1))
    with pytest.raises(NotImplementedError):
        duty_head(torch.zeros(2, 1, 4, 4))


# ------------------------------------------------------------------------------------------------ entry point
def _entry():
    import train_ours_exposuredecision as entry
    return entry


def test_entry_point_parses_the_reference_command_line():
    entry = _entry()
    a = entry.build_parser().parse_args(["-c", "cfg.yml", "-id", "ex1", "-seed", "7", "-r", "ckpt.pth", "--reset", "--limited_memory"])
    assert (a.config, a.runid, a.seed, a.resume, a.reset, a.limited_memory) == ("cfg.yml", "ex1", 7, "ckpt.pth", True, True)
    d = entry.build_parser().parse_args([])
    assert d.config == entry.DEFAULT_CONFIG and d.seed == 123 and d.resume is None and not d.reset and not d.limited_memory
    b = entry.build_parser().parse_args(["--data", "clips", "--valid-data", "v", "--iterations", "6", "--precision", "fp32", "--graph"])
    assert (b.data, b.valid_data, b.iterations, b.precision, b.graph) == ("clips", "v", 6, "fp32", True)


def test_shipped_config_and_settings():
    entry = _entry()
    cfg = yaml.safe_load(open(CONFIG))
    assert cfg["model"]["name"] == "ExposureDecision"
    assert cfg["model"]["BlurryFashion"] in entry.BLURRY_FASHIONS
    assert cfg["model"]["args"]["EventInch"] == 2 * cfg["TIME_BINS"]
    assert cfg["model"]["args"]["BLInch"] == entry.BLURRY_FASHIONS[cfg["model"]["BlurryFashion"]]
    es = entry.exposure_settings(cfg)
    assert es["name"] == "ExposureDecision" and es["fashion"] == "RGBLap" and es["TB"] == 16
    assert es["model_args"] == dict(EventInch=32, BLInch=4, InterCH=64, Group=4, norm=None, activation="LeakyReLU")
    assert es["exposure_time"] == list(range(1, 16)) and es["frames_per_period"] == 16
    assert (es["batch_size"], es["height"], es["width"]) == (4, 128, 128)          # the reference's stage-1 shape
    st = entry.trainer_settings(cfg, None)
    assert st == {"iterations": 100, "save_period": 1000, "lr_change_rate": 1, "lr_min": 1e-6, "accu_step": 1, "log_step": 10}
    assert entry.trainer_settings(cfg, 6)["iterations"] == 6
    vs = entry.validation_settings(cfg, None)
    assert vs["do_validation"] is False and vs["monitor"] == "min valid_loss" and vs["early_stop"] == 10.0
    assert vs["valid_step"] == 5000 and vs["valid_batches"] == 2 and vs["batch_size"] == 2 and vs["valid_data"] is None
    assert entry.validation_settings(cfg, "clips")["valid_data"] == "clips"
    sched = entry.build_lr_scheduler(cfg, torch.optim.Adam([torch.nn.Parameter(torch.zeros(1))], lr=1e-4))
    assert isinstance(sched, torch.optim.lr_scheduler.StepLR) and sched.step_size == 200000 and sched.gamma == 0.5
    # the model section builds the module
    from ebfi_amd.model import ExposureDecision
    net = ExposureDecision(**es["model_args"])
    assert net.EventFeatExtract.conv2d.in_channels == 32 and net.BLFeatExtract.conv2d.in_channels == 4


def test_unknown_fashion_and_no_events_model_raise():
    entry = _entry()
    from ebfi_amd.exposure_engine import ExposureEngine, blurry_level
    cfg = yaml.safe_load(open(CONFIG))
    cfg["model"]["BlurryFashion"] = "Sobel"
    with pytest.raises(Exception, match="Wrong blurry convertion fashion!!"):
        entry.exposure_settings(cfg)
    with pytest.raises(Exception, match="Wrong blurry convertion fashion!!"):
        blurry_level(torch.rand(1, 3, 8, 8), "Sobel")
    with pytest.raises(Exception, match="Wrong blurry convertion fashion!!"):
        ExposureEngine(fashion="Sobel", device="cpu")
    cfg = yaml.safe_load(open(CONFIG))
    cfg["model"]["name"] = "ExposureDecisionNoEvents"
    with pytest.raises(NotImplementedError, match="not defined by the reference either"):
        entry.exposure_settings(cfg)
    with pytest.raises(NotImplementedError, match="not defined by the reference either"):
        ExposureEngine(device="cpu", name="ExposureDecisionNoEvents")
    with pytest.raises(ValueError, match="BLInch"):
        ExposureEngine(dict(BLInch=4), fashion="DarkCh", device="cpu")
    with pytest.raises(ValueError, match="precision"):
        ExposureEngine(device="cpu", precision="bf16")


def test_both_trainers_build_recorded_clips_through_one_function_and_the_loader_arrives(tmp_path):
    """train_ours.clip_dataset is the dataset call of both trainers: every dataset section that reaches it (stage 1's train and
    valid_dataloader sections, stage 2's) gives a dataset on the asked-for loader, absent keys take the calling script's
    defaults, and real_data_periods hands its `loader` through (it once did not: --data died before the first step).  Drawing an
    item needs the device: tests/test_gpu_exposure.py::test_entry_point_trains_on_recorded_clips_with_both_loaders."""
    import inspect
    import re
    import train_ours
    from ebfi_amd import clipdata
    entry = _entry()
    assert entry.clip_dataset is train_ours.clip_dataset
    clipdata.write_synthetic_clip(str(tmp_path / "clip0.npz"))          # 33 frames of 64 x 64: two periods of 16
    cfg1, cfg2 = yaml.safe_load(open(CONFIG)), yaml.safe_load(open(os.path.join(os.path.dirname(CONFIG), "train_ours.yml")))
    es = entry.exposure_settings(cfg1)
    stage1, stage2 = (es["TB"], entry.DEFAULT_EXPOSURE_TIME), (int(cfg2["model"]["args"]["TB"]), train_ours.DEFAULT_EXPOSURE_TIME)
    assert stage1 == (16, list(range(1, 16))) and stage2 == (16, [9, 10, 11, 12, 13, 14, 15])
    sections = {"stage 1 train": (cfg1["train_dataloader"]["dataset"], stage1, [1 / 16, 2 / 16]),
                "stage 1 valid": (entry.validation_settings(cfg1)["dataset"], stage1, [1 / 16, 2 / 16]),
                "stage 1 no keys": ({}, stage1, [1 / 16, 2 / 16]),
                "stage 2 train": ((cfg2.get("train_dataloader") or {}).get("dataset") or {}, stage2, [9 / 16, 10 / 16]),
                "stage 2 valid": (train_ours.validation_settings(cfg2)["dataset"], stage2, [9 / 16, 10 / 16])}
    for tag, (ds_cfg, (tb, times), duties) in sections.items():
        ds = train_ours.clip_dataset(str(tmp_path), ds_cfg, tb, times, "cpu", 123, "host")
        assert ds.frames == "host" and len(ds) == 2 and ds.time_bins == 16 and ds.device.type == "cpu", tag
        assert [item[2] for _, item in ds.items] == duties, tag
    with pytest.raises(ValueError, match="frames must be"):
        train_ours.clip_dataset(str(tmp_path), {}, 16, [9], "cpu", 123, "pinned")
    # the one ClipDataset( of the two scripts, and every caller passes its loader on
    sources = {m: inspect.getsource(m) for m in (train_ours, entry)}
    assert sum(src.count("ClipDataset(") for src in sources.values()) == 1
    for fn, loader in ((entry.real_data_periods, "loader"), (entry.validation_batches, "args.loader"),
                       (train_ours.real_data_passes, "loader"), (train_ours.validation_batches, "args.loader")):
        calls = re.findall(r"clip_dataset\((.*?)\)\n", inspect.getsource(fn), flags=re.S)
        assert len(calls) == 1 and calls[0].split(",")[-1].strip() == loader, (fn.__name__, calls)


def test_synthetic_exposure_batch_host_draw():
    from ebfi_amd.exposure_engine import synthetic_exposure_batch
    frame, event, duty = synthetic_exposure_batch(5, 8, 12, TB=4, exposure_time=[9, 12, 15], num_frame_per_period=16,
                                                  device="cpu", seed=11)
    assert frame.shape == (5, 3, 8, 12) and event.shape == (5, 4, 2, 8, 12) and duty.shape == (5, 1)
    assert 0 <= frame.min() and frame.max() <= 1 and torch.equal(event, event.round()) and event.min() >= 0
    assert set(duty.reshape(-1).tolist()) <= {9 / 16, 12 / 16, 15 / 16}
    again = synthetic_exposure_batch(5, 8, 12, TB=4, exposure_time=[9, 12, 15], num_frame_per_period=16, device="cpu", seed=11)
    assert all(torch.equal(a, b) for a, b in zip((frame, event, duty), again))
    other = synthetic_exposure_batch(5, 8, 12, TB=4, exposure_time=[9, 12, 15], device="cpu", seed=11, rank=1)
    assert not torch.equal(frame, other[0])


def test_stage1_checkpoint_loads_into_stage2_model(tmp_path):
    """A checkpoint written by the stage-1 helpers from a CPU ExposureDecision is what EVFIAutoEx(LoadPretrainEX=True,
    PretrainedEXPath=...) loads: every ExposureDecision.* tensor bit-equal, FrozenEX leaves them without gradient."""
    entry = _entry()
    from ebfi_amd.engine import DEFAULT_MODEL_ARGS
    from ebfi_amd.exposure_engine import ExposureEngine
    from ebfi_amd.model import EVFIAutoEx, ExposureDecision
    cfg = yaml.safe_load(open(CONFIG))
    eng = ExposureEngine(cfg["model"]["args"], fashion=cfg["model"]["BlurryFashion"], device="cpu", seed=5)
    with torch.no_grad():
        for p in eng.model.parameters():
            p.add_(0.01 * torch.randn_like(p))              # (not the initial values a fresh stage-2 model would have anyway)
    sched = entry.build_lr_scheduler(cfg, eng.optimizer.inner)
    path = str(tmp_path / "models" / "checkpoint-iteration5.pth")
    paths = entry.save_checkpoint(path, eng, sched, cfg, 5, monitor_best=0.125, save_best=True)
    assert [os.path.basename(p) for p in paths] == ["checkpoint-iteration5.pth", "model_best_until_iteration5.pth"]
    for p in paths:
        cpt = torch.load(p, map_location="cpu", weights_only=False)
        assert tuple(cpt) == entry.CHECKPOINT_KEYS == ("model", "lr_scheduler", "optimizer", "config", "trainer")
        assert cpt["model"]["name"] == "ExposureDecision" and cpt["optimizer"]["name"] == "Adam"
        assert cpt["trainer"] == {"training_mode": "iteration_based_train", "iteration": 5, "monitor_best": 0.125}
        assert list(cpt["model"]["states"]) == list(ExposureDecision(**cfg["model"]["args"]).state_dict())
    want = {k: v.clone() for k, v in eng.model.state_dict().items()}
    for frozen in (False, True):
        net = EVFIAutoEx(**dict(DEFAULT_MODEL_ARGS, LoadPretrainEX=True, PretrainedEXPath=paths[1], FrozenEX=frozen))
        got = {k[len("ExposureDecision."):]: v for k, v in net.state_dict().items() if k.startswith("ExposureDecision.")}
        assert list(got) == list(want)
        for k in want:
            assert got[k].dtype == want[k].dtype and torch.equal(got[k], want[k]), k
        assert all(p.requires_grad == (not frozen) for p in net.ExposureDecision.parameters())
        assert any(p.requires_grad for n, p in net.named_parameters() if not n.startswith("ExposureDecision."))
        if frozen:
            assert not net.ExposureDecision.training
    # ... and the stage-1 resume path restores the counters (model, optimiser, monitor)
    eng2 = ExposureEngine(cfg["model"]["args"], fashion="RGBLap", device="cpu", seed=6)
    mon = entry.Monitor("min valid_loss", 10)
    start = entry.resume_checkpoint(paths[0], eng2, entry.build_lr_scheduler(cfg, eng2.optimizer.inner), cfg, monitor=mon)
    assert start == 6 and eng2.iteration == 6 and mon.best == 0.125
    for k, v in eng2.model.state_dict().items():
        assert torch.equal(v, want[k]), k
