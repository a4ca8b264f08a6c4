"""Validation of train_ours.py without a GPU: the Charbonnier entry points' host side (workspace arithmetic, argument errors
before any launch), the float64 restatement of the loss the GPU tests compare the kernel with, the monitor / early-stop logic
(eval_model_performance of the reference trainer, train_ours.py:392-435), monitor_best through checkpoint and resume, the
rank sharding of the validation order, and the validation keys of the config."""
import ctypes
import importlib.util
import math
import os

import numpy as np
import pytest
import torch
import yaml

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
PKG = os.path.join(ROOT, "ebfi-be_amd")

SMALL = dict(FrameBasech=8, EventBasech=8, InterCH=8, TB=4, step=2, channels=[4, 4, 8, 8])


def ref_charbonnier(x, y, eps=1e-3):
    """Per-sample sums [N] of sqrt((x - y)^2 + eps) over C, H, W in float64 (loss/restore.py:95-105: a sum, eps under the root)."""
    x, y = np.asarray(x, np.float64), np.asarray(y, np.float64)
    d = x - y
    return np.sqrt(d * d + eps).reshape(d.shape[0], -1).sum(1)


def _trainer():
    spec = importlib.util.spec_from_file_location("ebfi_train_ours_validation", os.path.join(PKG, "train_ours.py"))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod


def _config():
    cfg = yaml.safe_load(open(os.path.join(PKG, "config", "train_ours.yml")))
    cfg["model"]["args"].update(SMALL)
    return cfg


# ------------------------------------------------------------------ the restatement against hand-derived answers
def test_restatement_identical_inputs_and_constant_offset():
    rng = np.random.default_rng(0)
    x = rng.random((2, 3, 5, 7))
    n = 3 * 5 * 7
    assert np.allclose(ref_charbonnier(x, x), n * math.sqrt(1e-3), rtol=1e-14)
    d = 0.25
    assert np.allclose(ref_charbonnier(x + d, x), n * math.sqrt(d * d + 1e-3), rtol=1e-12)
    assert np.allclose(ref_charbonnier(x, x + d, eps=0.5), n * math.sqrt(d * d + 0.5), rtol=1e-12)
    # eps is NOT squared: with d = 0 and eps = 1e-3 a term is 0.0316..., not 1e-3
    assert abs(ref_charbonnier(np.zeros((1, 1, 1, 1)), np.zeros((1, 1, 1, 1)))[0] - 0.03162277660168379) < 1e-15
    y = x.copy()
    y[1, 2, 3, 4] = np.nan
    got = ref_charbonnier(x, y)
    assert np.isfinite(got[0]) and np.isnan(got[1])


# ------------------------------------------------------------------ the C ABI without a device
@pytest.fixture(scope="module")
def lib():
    from ebfi_amd import _native as N
    if not os.path.exists(N.LIB_PATH):
        N.build()
    return N.lib()


def test_charbonnier_workspace_is_host_arithmetic(lib):
    # one 8-byte partial per (sample, strip of R = ceil(4096 / W) of the sample's C * H rows)
    assert lib.ebfi_charbonnier_workspace(8, 3, 720, 1280) == 8 * (3 * 720 // 4) * 8
    assert lib.ebfi_charbonnier_workspace(2, 3, 128, 128) == 2 * 12 * 8
    assert lib.ebfi_charbonnier_workspace(5, 1, 37, 129) == 5 * 2 * 8            # R = 32: 37 rows -> 2 strips
    assert lib.ebfi_charbonnier_workspace(1, 1, 1, 1) == 8
    assert lib.ebfi_charbonnier_workspace(0, 3, 8, 8) == 0
    assert lib.ebfi_charbonnier_workspace(1, 0, 8, 8) == 0 and lib.ebfi_charbonnier_workspace(1, 3, 0, 8) == 0
    assert lib.ebfi_charbonnier_workspace(-1, 3, 8, 8) == 0


def test_charbonnier_argument_errors_do_not_touch_the_gpu(lib):
    from ebfi_amd import _native as N
    st = N.i64x4((3 * 64, 64, 8, 1))
    fake = ctypes.c_void_p(4096)                       # never dereferenced: every check below fails before a launch
    big = 1 << 20

    def fwd(x=fake, y=fake, C=3, ws=fake, ws_bytes=big, out=fake, strides=st, eps=1e-3):
        return lib.ebfi_charbonnier_forward(x, strides, y, strides, 1, C, 8, 8, eps, ws, ws_bytes, out, None)

    def bwd(x=fake, y=fake, C=3, g=fake, gx=fake, strides=st, eps=1e-3):
        return lib.ebfi_charbonnier_backward(x, strides, y, strides, 1, C, 8, 8, eps, g, gx, None)

    assert fwd(x=None) == -1 and b"null" in lib.ebfi_last_error()
    assert fwd(y=None) == -1 and fwd(ws=None) == -1 and fwd(out=None) == -1
    assert fwd(C=0) == -1 and b"bad shape" in lib.ebfi_last_error()
    assert fwd(eps=0.0) == -1 and b"eps" in lib.ebfi_last_error()
    assert fwd(eps=-1e-3) == -1 and fwd(eps=float("nan")) == -1
    assert fwd(strides=N.i64x4((3 * 64, 64, 8, 2))) == -3 and b"column stride" in lib.ebfi_last_error()   # EBFI_ERR_UNSUPPORTED
    assert fwd(ws_bytes=lib.ebfi_charbonnier_workspace(1, 3, 8, 8) - 1) == -4 and b"workspace" in lib.ebfi_last_error()
    assert fwd(ws=ctypes.c_void_p(4096 + 8)) == -1 and b"aligned" in lib.ebfi_last_error()
    assert bwd(x=None) == -1 and b"null" in lib.ebfi_last_error()
    assert bwd(y=None) == -1 and bwd(g=None) == -1 and bwd(gx=None) == -1
    assert bwd(C=0) == -1 and bwd(eps=0.0) == -1
    assert bwd(strides=N.i64x4((3 * 64, 64, 8, 2))) == -3


def test_charbonnier_loss_refuses_cpu_tensors_and_is_exported_like_the_reference():
    from ebfi_amd.loss import CharbonnierLoss, charbonnier_per_sample
    with pytest.raises(NotImplementedError):
        CharbonnierLoss()(torch.rand(1, 3, 8, 8), torch.rand(1, 3, 8, 8))
    with pytest.raises(NotImplementedError):
        charbonnier_per_sample(torch.rand(1, 3, 8, 8), torch.rand(1, 3, 8, 8))
    import loss as shim
    from loss.restore import CharbonnierLoss as exported
    assert exported is CharbonnierLoss and shim.CharbonnierLoss is CharbonnierLoss
    assert exported().eps == 1e-3 and exported(eps=1e-6).eps == 1e-6


# ------------------------------------------------------------------ monitor: best / early stop
MONITOR_TABLE = [
    # (monitor, early_stop, logs, best flags, stop flags, final best)
    ("min valid_loss", math.inf, [5.0, 4.0, 4.5, 3.0], [True, True, False, True], [False] * 4, 3.0),
    ("max valid_psnr", math.inf, [30.0, 29.0, 31.0], [True, False, True], [False] * 3, 31.0),
    ("min valid_loss", 2, [5.0, 5.0, 6.0, 7.0, 8.0], [True, True, False, False, False], [False, False, False, False, True], 5.0),  # a tie improves
    ("max valid_psnr", 1, [30.0, 30.0, 29.0, 28.0], [True, True, False, False], [False, False, False, True], 30.0),
    ("min valid_loss", 0, [5.0, 4.0, 4.1], [True, True, False], [False, False, True], 4.0),        # early_stop 0: the first miss stops
    ("min valid_loss", 1, [5.0, None, 6.0, None, 7.0], [True, False, False, False, False], [False, False, False, False, True], 5.0),
    ("off", 0, [5.0, 6.0, 7.0], [False] * 3, [False] * 3, None),
]


@pytest.mark.parametrize("monitor,early_stop,values,want_best,want_stop,final", MONITOR_TABLE)
def test_monitor_table(monitor, early_stop, values, want_best, want_stop, final):
    T = _trainer()
    warnings = []
    m = T.Monitor(monitor, early_stop, warn=warnings.append)
    key = monitor.split()[1] if monitor != "off" else "valid_loss"
    assert m.best == (None if monitor == "off" else (math.inf if monitor.startswith("min") else -math.inf))
    got_best, got_stop, counts = [], [], []
    for v in values:
        stop, best = m.evaluate({"other": 1.0} if v is None else {key: v, "other": 1.0})     # None = the key is missing
        got_best.append(best), got_stop.append(stop), counts.append(m.not_improved_count)
    assert got_best == want_best and got_stop == want_stop and m.best == final
    missing = [i for i, v in enumerate(values) if v is None]
    assert len(warnings) == (len(missing) if monitor != "off" else 0) and all("is not found" in w for w in warnings)
    for i in missing:                                  # a missing key moves no counter
        assert counts[i] == counts[i - 1]


def test_monitor_refuses_a_malformed_setting_and_words_the_stop_like_the_reference():
    T = _trainer()
    for bad in ("valid_loss", "lowest valid_loss", "min"):
        with pytest.raises(ValueError):
            T.Monitor(bad)
    assert T.Monitor("min valid_loss", 10).stop_message() == "Validation performance didn't improve for 10 stamps. Training stops."


# ------------------------------------------------------------------ config
def test_shipped_config_has_the_validation_keys_and_validation_off():
    T = _trainer()
    cfg = yaml.safe_load(open(os.path.join(PKG, "config", "train_ours.yml")))
    vs = T.validation_settings(cfg)
    assert vs["do_validation"] is False and vs["valid_step"] == 5000 and vs["valid_data"] is None
    assert cfg["trainer"]["do_validation"] is False and "valid_step" in cfg["trainer"]["iteration_based_train"]
    # absent keys = off, the reference's defaults
    vs = T.validation_settings({"trainer": {}})
    assert vs["do_validation"] is False and vs["monitor"] == "off" and vs["early_stop"] == math.inf and vs["valid_data"] is None
    vs = T.validation_settings({"trainer": {"do_validation": True, "monitor": "max valid_psnr", "early_stop": 3,
                                            "iteration_based_train": {"valid_step": 7.0}},
                                "valid_dataloader": {"path_to_datalist_txt": "a.txt", "batch_size": 2}}, cli_valid_data="b.npz")
    assert vs["do_validation"] and vs["valid_step"] == 7 and vs["early_stop"] == 3 and vs["valid_data"] == "b.npz"
    assert vs["batch_size"] == 2 and vs["drop_last"] is False
    assert "validation and early stopping of the reference are out of scope" not in T.__doc__ and "do_validation" in T.__doc__


def test_reference_validation_dataset_section_maps_to_centre_crop_only():
    """valid_dataloader.dataset as the reference ships it (config/train_ours.yml:159-192), typed in: centre crop 128, random
    crop and flips off, noise off."""
    from ebfi_amd import clipdata
    section = {
        "scale": 2, "ori_scale": "down2", "time_bins": 16, "NumFramePerPeriod": 16, "NumFramePerBlurry": 16, "NumPeriodPerSeq": 4,
        "SlidingWindowSeq": 4, "NumPeriodPerLoad": 1, "SlidingWindowLoad": 1, "ExposureMethod": "Custom",
        "ExposureTime": [9, 10, 11, 12, 13, 14, 15], "NeedNeighborGT": False,
        "data_augment": {
            "enabled": True,
            "augment": ["RandomCrop", "CenterCrop", "HorizontalFlip", "VertivcalFlip", "Noise", "HotPixel"],
            "random_crop": {"enabled": False, "size": [128, 128]},
            "center_crop": {"enabled": True, "size": [128, 128]},
            "flip": {"enabled": False, "horizontal_prob": 0.5, "vertical_prob": 0.5},
            "noise": {"enabled": False, "noise_std": 1.0, "noise_fraction": 0.05},
            "hot_pixel": {"enabled": False, "hot_pixel_std": 2.0, "hot_pixel_fraction": 0.001}}}
    got = clipdata.dataset_args_from_config(section)
    assert got["crop"] == [128, 128] and got["crop_mode"] == "center" and got["center_crop"] is None
    assert got["flips"] is False and got["noise"] is None
    # the section of this repo's own config says the same
    cfg = yaml.safe_load(open(os.path.join(PKG, "config", "train_ours.yml")))
    own = clipdata.dataset_args_from_config(cfg["valid_dataloader"]["dataset"])
    assert own == got


# ------------------------------------------------------------------ sharding of the validation order
@pytest.mark.parametrize("world", [1, 2, 3, 4])
def test_shards_are_equal_and_cover_everything(world):
    from ebfi_amd.clipdata import shard_indices
    for n in range(10):
        shards = [shard_indices(n, r, world) for r in range(world)]
        assert len({len(s) for s in shards}) == 1 and len(shards[0]) == -(-n // world)
        assert set().union(*shards) == set(range(n))
        # DistributedSampler(shuffle=False): the padded order dealt round-robin
        order = list(range(n))
        padded = (order * (world + 1))[:len(shards[0]) * world] if n else []
        assert shards == [padded[r::world] for r in range(world)]
    with pytest.raises(ValueError):
        shard_indices(4, world, world)


def test_validation_seeds_never_meet_a_training_seed():
    T = _trainer()
    seeds = T.validation_seeds(123, 5)
    assert len(set(seeds)) == 5 and max(seeds) < 123          # every training batch is drawn from seed + 1000 k + rank >= seed
    assert T.validation_seeds(123, 5) == seeds
    from ebfi_amd.engine import synthetic_validation_batch
    a = synthetic_validation_batch(2, 8, 8, TB=4, num_frames=3, device="cpu", seed=seeds[0])
    b = synthetic_validation_batch(2, 8, 8, TB=4, num_frames=3, device="cpu", seed=seeds[0])
    c = synthetic_validation_batch(2, 8, 8, TB=4, num_frames=3, device="cpu", seed=seeds[1])
    assert all(torch.equal(u, v) for u, v in zip(a, b)) and not torch.equal(a[0], c[0])
    assert a[2].shape == (2, 3) and a[4].shape == (2, 3, 3, 8, 8) and a[2][0].tolist() == pytest.approx([0.0, 1 / 3, 2 / 3], abs=1e-7)


# ------------------------------------------------------------------ monitor_best through checkpoint and resume
def test_monitor_best_is_written_restored_and_dropped_by_reset(tmp_path):
    from ebfi_amd.engine import Engine
    T = _trainer()
    cfg = _config()
    eng = Engine(cfg["model"]["args"], device="cpu", lr=1e-3, seed=1)
    sched = T.build_lr_scheduler(cfg, eng.optimizer.inner)
    path = str(tmp_path / "checkpoint-iteration6.pth")
    written = T.save_checkpoint(path, eng, sched, cfg, 6, monitor_best=41.5, save_best=True)
    assert T.best_checkpoint_name(6) == "model_best_until_iteration6.pth"
    assert written == [path, str(tmp_path / "model_best_until_iteration6.pth")] and all(os.path.exists(p) for p in written)
    a, b = (torch.load(p, map_location="cpu", weights_only=False) for p in written)
    assert a["trainer"] == b["trainer"] == {"training_mode": "iteration_based_train", "iteration": 6, "monitor_best": 41.5}
    assert set(a) == set(T.CHECKPOINT_KEYS)
    for u, v in zip(a["model"]["states"].values(), b["model"]["states"].values()):
        assert torch.equal(u, v)
    # the earlier call shapes still work and write None, and no best file
    plain = str(tmp_path / "plain" / "checkpoint-iteration2.pth")
    T.save_checkpoint(plain, eng, sched, cfg, 2)
    assert torch.load(plain, map_location="cpu", weights_only=False)["trainer"]["monitor_best"] is None
    assert os.listdir(str(tmp_path / "plain")) == ["checkpoint-iteration2.pth"]
    assert T.checkpoint_state(eng, sched, cfg, 2)["trainer"]["monitor_best"] is None

    def resume(ckpt, reset=False, monitor="min valid_loss"):
        e = Engine(cfg["model"]["args"], device="cpu", lr=1e-3, seed=2)
        m = T.Monitor(monitor, 3)
        m.not_improved_count = 2
        start = T.resume_checkpoint(ckpt, e, T.build_lr_scheduler(cfg, e.optimizer.inner), cfg, reset=reset, monitor=m)
        return start, m

    start, m = resume(path)
    assert start == 7 and m.best == 41.5
    start, m = resume(path, reset=True)
    assert start == 0 and m.best == math.inf                 # --reset: the model only
    start, m = resume(plain)
    assert start == 3 and m.best == math.inf                 # a checkpoint written without validation leaves the monitor alone
    start, m = resume(path, monitor="off")
    assert start == 7 and m.best is None
    other = torch.load(path, map_location="cpu", weights_only=False)
    other["trainer"]["training_mode"] = "epoch_based_train"
    torch.save(other, str(tmp_path / "other.pth"))
    start, m = resume(str(tmp_path / "other.pth"))
    assert start == 0 and m.best == math.inf                 # another training mode: like --reset


# ------------------------------------------------------------------ ranks take the same decision (gloo, world 2)
def _decision_worker(rank, world, port, outdir):
    import torch.distributed as dist
    os.environ.update(MASTER_ADDR="127.0.0.1", MASTER_PORT=str(port), RANK=str(rank), WORLD_SIZE=str(world))
    dist.init_process_group("gloo", rank=rank, world_size=world)
    from ebfi_amd.clipdata import shard_indices
    from ebfi_amd.metrics import MetricTracker
    T = _trainer()

    class FakeEngine:
        """Engine.validate replaced by a table: the 'batch' is an item index, its score depends on the stamp."""
        VALID_KEYS = ("valid_loss", "valid_psnr", "valid_ssim")
        calls = 0

        def validate(self, batch, load=0, refresh=True):
            self.calls += 1
            v = float(self.scores[batch])
            return {"valid_loss": torch.tensor(v, dtype=torch.float64), "valid_psnr": torch.tensor(-v, dtype=torch.float64),
                    "valid_ssim": torch.tensor(0.5, dtype=torch.float64)}

    eng, tracker, monitor = FakeEngine(), MetricTracker(FakeEngine.VALID_KEYS), T.Monitor("min valid_loss", 1, warn=lambda m: None)
    mine = shard_indices(5, rank, world)                 # 5 items over 2 ranks: 3 each, item 0 wraps round to rank 1
    record = []
    for stamp, scores in enumerate(([5, 1, 2, 3, 4], [4, 1, 2, 3, 4], [9, 9, 9, 9, 9], [8, 8, 8, 8, 8]), 1):
        eng.scores = scores
        log = T.run_validation(eng, lambda: iter(mine), tracker, stamp, log_step=10 ** 6, rank=1)
        record.append((log["valid_loss"],) + monitor.evaluate(log))
    torch.save((record, eng.calls), os.path.join(outdir, "r%d.pt" % rank))
    dist.barrier()
    dist.destroy_process_group()


def test_two_ranks_make_the_same_calls_and_take_the_same_decision(tmp_path):
    import torch.multiprocessing as mp
    ctx = mp.get_context("spawn")
    port = 29500 + (os.getpid() % 500)
    procs = [ctx.Process(target=_decision_worker, args=(r, 2, port, str(tmp_path))) for r in range(2)]
    for p in procs:
        p.start()
    for p in procs:
        p.join(timeout=180)
        assert p.exitcode == 0
    (ra, ca), (rb, cb) = (torch.load(os.path.join(str(tmp_path), "r%d.pt" % r)) for r in range(2))
    assert ra == rb and ca == cb == 12                   # 3 (batch, load) collectives per stamp on both ranks
    # rank 0 scores items 0, 2, 4 and rank 1 items 1, 3, 0: the stamp's value is the mean over ranks and batches
    assert ra[0][0] == pytest.approx(((5 + 2 + 4) + (1 + 3 + 5)) / 6)
    assert [r[1:] for r in ra] == [(False, True), (False, True), (False, False), (True, False)]
