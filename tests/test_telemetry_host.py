"""The training monitor without a GPU: the float64 restatement of the segment statistics the GPU tests compare the kernel with,
the bucket table, the parameter groups, the config keys and their default-off behaviour, the entry points' host side, and
train_loop with a fake engine: which tags at which steps reach the event file, and that only rank 0 writes."""
import ctypes
import importlib.util
import os
import sys

import numpy as np
import pytest
import torch
import yaml

import telemetry_ref as TR
import tfevents_ref as R
from ebfi_amd import _native as N
from ebfi_amd import monitor as M
from ebfi_amd import telemetry

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
PKG = os.path.join(ROOT, "ebfi-be_amd")


def _trainer(name="train_ours"):
    spec = importlib.util.spec_from_file_location("ebfi_%s_telemetry" % name, os.path.join(PKG, name + ".py"))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod


# ------------------------------------------------------------------ the restatement and the bucket table
def test_default_limits_are_tensorflows():
    lim = telemetry.default_bucket_limits()
    assert lim.dtype == np.float64 and lim.size == 1550 and np.all(np.diff(lim) > 0)
    assert lim[-1] == sys.float_info.max and lim[774] == 0.0 and lim[775] == 1e-12 and lim[773] == -1e-12
    assert lim[776] == 1e-12 * 1.1 and lim[-2] < 1e20 <= lim[-2] * 1.1
    assert np.array_equal(lim, TR.tf_default_limits())
    assert np.array_equal(lim[:774], -lim[775:-1][::-1])


def test_restatement_against_a_plain_loop():
    lim = np.array([-2.0, -1e-12, 0.0, 1e-12, 0.5, 3.0])
    x = np.array([0.0, -0.0, 0.5, 0.5000001, np.nan, -2.0, -2.5, np.inf, 1e-13, 7.0, -np.inf, 3.0, 1e-45], dtype=np.float32)
    offsets = [0, 0, 5, 13]
    moments, hist = TR.segment_stats_ref(x, offsets, lim)
    for s in range(3):
        seg = [float(v) for v in x[offsets[s]:offsets[s + 1]]]
        fin = [v for v in seg if np.isfinite(v)]
        want = np.zeros(lim.size, np.int64)
        for v in fin:
            i = 0
            while i < lim.size - 1 and not v <= lim[i]:
                i += 1
            want[i] += 1
        assert np.array_equal(hist[s], want)
        assert moments[s, 0] == len(fin) and moments[s, 1] == len(seg) - len(fin)
        assert moments[s, 2] == (min(fin) if fin else np.inf) and moments[s, 3] == (max(fin) if fin else -np.inf)
        assert moments[s, 4] == pytest.approx(sum(fin), rel=1e-15) and moments[s, 5] == pytest.approx(sum(v * v for v in fin), rel=1e-15)
    assert list(moments[0]) == [0, 0, np.inf, -np.inf, 0, 0] and hist[0].sum() == 0
    # +-0 and a value exactly on a limit fall into the bucket that limit closes; 7.0 lies past the table: the last bucket
    assert list(hist[1]) == [0, 0, 2, 0, 1, 1] and list(hist[2]) == [2, 0, 0, 2, 0, 2]


def test_histogram_span_keeps_first_to_last_non_empty_bucket():
    lim = np.arange(6, dtype=np.float64)
    assert telemetry.histogram_span(lim, [0, 2, 0, 0, 1, 0]) == ([1.0, 2.0, 3.0, 4.0], [2.0, 0.0, 0.0, 1.0])
    assert telemetry.histogram_span(lim, [0, 0, 0, 0, 0, 3]) == ([5.0], [3.0])
    assert telemetry.histogram_span(lim, [0] * 6) == ([], [])


def test_parameter_groups_follow_the_flat_order():
    from ebfi_amd.model import EVFIAutoEx
    from ebfi_amd.engine import DEFAULT_MODEL_ARGS
    net = EVFIAutoEx(**dict(DEFAULT_MODEL_ARGS, FrameBasech=8, EventBasech=8, InterCH=8, TB=4, step=2, channels=[4, 4, 8, 8]))
    named = [(n, p) for n, p in net.named_parameters() if p.requires_grad]
    for depth in (1, 2, 3):
        names, offsets = telemetry.parameter_groups(named, depth)
        assert len(set(names)) == len(names) == len(offsets) - 1 and offsets[0] == 0
        assert offsets[-1] == sum(p.numel() for _, p in named) and all(b > a for a, b in zip(offsets, offsets[1:]))
        off = 0
        for n, p in named:                              # every parameter lies inside the segment that carries its prefix
            s = names.index(".".join(n.split(".")[:depth]))
            assert offsets[s] <= off and off + p.numel() <= offsets[s + 1]
            off += p.numel()
    assert len(telemetry.parameter_groups(named, 1)[0]) < len(telemetry.parameter_groups(named, 2)[0])
    a, b = torch.nn.Parameter(torch.zeros(3)), torch.nn.Parameter(torch.zeros(2))
    with pytest.raises(ValueError):
        telemetry.parameter_groups([("x.w", a), ("y.w", b), ("x.b", b)], 1)
    assert telemetry.parameter_groups([], 2) == ([], [0])


# ------------------------------------------------------------------ the entry points' host side
def test_new_symbols_are_declared_bound_and_exported():
    new = {"ebfi_segment_stats_workspace", "ebfi_segment_stats"}
    assert new <= set(N.declared_symbols()) and new <= set(N.SIGNATURES)
    if not os.path.exists(N.LIB_PATH):
        N.build()
    h = ctypes.CDLL(N.LIB_PATH)
    for name in new:
        assert hasattr(h, name), name
    assert N.lib().ebfi_abi_version() == 14              # a pure addition: the ABI generation does not move


def test_workspace_arithmetic_and_argument_errors_touch_no_gpu():
    lib = N.lib()
    assert lib.ebfi_segment_stats_workspace(0, 0) == 0
    assert lib.ebfi_segment_stats_workspace(4096, 1) == (1 + 1) * 6 * 8
    assert lib.ebfi_segment_stats_workspace(4097, 7) == (2 + 7) * 6 * 8          # one record per possible chunk: ceil(n / 4096) + S
    assert lib.ebfi_segment_stats_workspace(-1, 3) == 0
    p = ctypes.c_void_p(16)
    args = lambda **kw: [kw.get("x", p), kw.get("n", 8), p, kw.get("S", 2), p, kw.get("nb", 10), p, p, kw.get("ws", p),
                         kw.get("bytes", 1 << 20), None]
    assert lib.ebfi_segment_stats(*args(n=-1)) == -1
    assert lib.ebfi_segment_stats(*args(nb=0)) == -1 and lib.ebfi_segment_stats(*args(nb=2049)) == -1
    assert b"bucket" in lib.ebfi_last_error()
    assert lib.ebfi_segment_stats(*args(x=None)) == -1 and b"null" in lib.ebfi_last_error()
    assert lib.ebfi_segment_stats(*args(ws=None)) == -4
    assert lib.ebfi_segment_stats(*args(ws=ctypes.c_void_p(8))) == -1
    assert lib.ebfi_segment_stats(*args(bytes=8)) == -4
    assert lib.ebfi_segment_stats(*args(S=0, x=None)) == 0                        # no segments: a no-op
    with pytest.raises(NotImplementedError):
        telemetry.SegmentStats([0, 4], 4, "cpu")


# ------------------------------------------------------------------ config keys, default off
def test_config_keys_and_default_off():
    for name in ("train_ours.yml", "train_ours_exposuredecision.yml"):
        cfg = yaml.safe_load(open(os.path.join(PKG, "config", name)))
        s = M.monitor_settings(cfg)
        assert not s["tensorboard"] and not s["vis_enabled"] and s["stats_step"] == 0, name
    cfg = {"experiment": "E", "trainer": {"output_path": "/o", "tensorboard": True,
                                          "vis": {"enabled": True, "train_img_writer_num": 7, "valid_img_writer_num": "3"},
                                          "telemetry": {"stats_step": 100.0, "group_depth": 3}}}
    assert M.monitor_settings(cfg) == {"tensorboard": True, "vis_enabled": True, "train_img_writer_num": 7, "valid_img_writer_num": 3,
                                       "stats_step": 100, "group_depth": 3}
    off = M.monitor_settings(cfg, cli_tensorboard=False)                         # --no-tensorboard switches every part off
    assert not off["tensorboard"] and not off["vis_enabled"] and off["stats_step"] == 0
    on = M.monitor_settings({"trainer": {}}, cli_tensorboard=True)               # --tensorboard alone: scalars only
    assert on["tensorboard"] and not on["vis_enabled"] and on["stats_step"] == 0 and on["group_depth"] == 2
    assert M.log_directory(cfg, "r7") == os.path.join("/o", "log", "E", "r7")


@pytest.mark.parametrize("script", ["train_ours", "train_ours_exposuredecision"])
def test_flags_override_the_config(script, tmp_path):
    T = _trainer(script)
    parse = (lambda argv: T.get_args(argv)) if script == "train_ours" else (lambda argv: T.build_parser().parse_args(argv))
    assert parse([]).tensorboard is None and parse(["--tensorboard"]).tensorboard is True
    assert parse(["--no-tensorboard"]).tensorboard is False
    cfg = {"experiment": "E", "trainer": {"output_path": str(tmp_path), "tensorboard": True}}
    assert T.build_monitor({"trainer": {}}, parse([]), "r", 0, object()) is None
    assert T.build_monitor(cfg, parse(["--no-tensorboard"]), "r", 0, object()) is None
    assert not (tmp_path / "log").exists()
    mon = T.build_monitor({"experiment": "E", "trainer": {"output_path": str(tmp_path)}}, parse(["--tensorboard"]), "r", 0, object())
    assert os.path.dirname(mon.writer.path) == str(tmp_path / "log" / "E" / "r")
    mon.close()


# ------------------------------------------------------------------ train_loop with a fake engine
class FakeBook:
    def __init__(self):
        self.guard = torch.tensor([0, 3], dtype=torch.int32)


class FakeEngine:
    """train_step returns a table's loss; the flat buffers are two small host tensors over a two-layer 'model'."""
    VALID_KEYS = ("valid_loss", "valid_psnr", "valid_ssim")
    settled = True

    def __init__(self):
        self.model = torch.nn.Sequential()
        self.model.add_module("A", torch.nn.Linear(2, 2))
        self.model.add_module("B", torch.nn.Linear(2, 1))
        params = list(self.model.parameters())
        self.optimizer = type("Opt", (), {})()
        self.optimizer.params = params
        self.optimizer.param_groups = [{"lr": 1e-4}]
        self.optimizer.flat = torch.nn.Parameter(torch.cat([p.detach().reshape(-1) for p in params]))
        self.bucket = type("Bucket", (), {})()
        self.bucket.flat = torch.arange(9, dtype=torch.float32) - 4
        self.book = FakeBook()
        self.keep_panels, self.panel_sharp, self.last_valid_panels = False, None, None
        self.losses = []

    def train_step(self, frame, event, t, gtex, target):
        self.losses.append(torch.tensor(0.5 ** len(self.losses) + 0.1, dtype=torch.float32))
        if self.keep_panels:
            self.panel_sharp = frame[:1] * 0.5
        return self.losses[-1]

    def validate(self, batch, load=0, refresh=True):
        if self.keep_panels:
            self.last_valid_panels = (batch[0], batch[1], batch[0] * 0.25, batch[4][:, -1])
        return {k: torch.tensor(float(i + 1), dtype=torch.float64) for i, k in enumerate(self.VALID_KEYS)}

    def state(self):
        return {}


def _host_panels(event, frame, sharp, target, out=None):
    f = lambda x: (x[0].clamp(0, 1).numpy() * 255).transpose(1, 2, 0).astype("uint8")
    ev = np.zeros_like(f(frame))
    ev[..., 1] = 255 * (event.sum(1)[0, 0] > 0).numpy()
    return torch.from_numpy(np.stack([ev, f(frame), f(sharp), f(target)]))


class HostStats:
    """stats_factory of the host test: the numpy restatement behind SegmentStats' interface."""
    def __init__(self, offsets, numel, device):
        self.offsets, self.limits_host = list(offsets), TR.tf_default_limits()

    def run(self, flat):
        m, h = TR.segment_stats_ref(flat.detach().numpy(), self.offsets, self.limits_host)
        return torch.from_numpy(m), torch.from_numpy(h.astype(np.int32))


def _run_loop(tmp_path, rank, monkeypatch):
    T = _trainer()
    monkeypatch.setattr(T, "save_checkpoint", lambda *a, **k: [])
    monkeypatch.setattr(torch.cuda, "synchronize", lambda *a, **k: None)
    cfg = {"experiment": "E", "trainer": {"output_path": str(tmp_path), "tensorboard": True,
                                          "vis": {"enabled": True, "train_img_writer_num": 2, "valid_img_writer_num": 2},
                                          "telemetry": {"stats_step": 3, "group_depth": 1}}}
    eng = FakeEngine()
    mon = M.TrainMonitor(M.monitor_settings(cfg), M.log_directory(cfg, "r"), rank=rank, ring=2, panels=_host_panels,
                         stats_factory=HostStats).attach(eng)
    g = torch.Generator().manual_seed(3)
    batch = (torch.rand(2, 3, 3, 5, generator=g), torch.poisson(torch.full((2, 4, 2, 3, 5), 0.4), generator=g), torch.rand(2, 1),
             torch.rand(2, 1), torch.rand(2, 3, 3, 5, generator=g))
    vbatch = (batch[0], batch[1], torch.rand(2, 2), batch[3], torch.rand(2, 2, 3, 3, 5, generator=g))
    st = {"iterations": 5, "save_period": 0, "lr_change_rate": 1, "lr_min": 0.0, "accu_step": 1, "log_step": 10}
    vs = {"do_validation": True, "valid_step": 3, "valid_log_step": 50}
    from ebfi_amd.metrics import MetricTracker
    it = T.train_loop(eng, lambda it, micro: batch, 2, "frames", st, vs, None, T.Monitor("off"), lambda: iter([vbatch, vbatch, vbatch]),
                      MetricTracker(eng.VALID_KEYS), str(tmp_path / "models"), cfg, rank, 1, 0, telemetry=mon)
    mon.close()
    assert it == 5
    return eng, mon, batch, vbatch


def test_train_loop_writes_the_listed_tags_and_steps(tmp_path, monkeypatch, capsys):
    eng, mon, batch, vbatch = _run_loop(tmp_path, 0, monkeypatch)
    files = os.listdir(str(tmp_path / "log" / "E" / "r"))
    assert len(files) == 1 and files[0].startswith("events.out.tfevents.")
    events = R.read_events(os.path.join(str(tmp_path / "log" / "E" / "r"), files[0]))
    assert events[0]["file_version"] == "brain.Event:2"
    tags = R.by_tag(events)
    steps = {t: [s for s, _ in v] for t, v in tags.items()}
    groups = ["A", "B"]
    want = {"train_loss/train": [0, 1, 2, 3, 4], "learning rate": [0, 1, 2, 3, 4],
            # flushes: the log line of iteration 0, the two-slot ring full at 2, the stamp at 3, the last iteration's log line
            "steps_per_sec/train": [0, 2, 3, 4],
            "valid_loss/valid": [0, 1, 2], "valid_HR_events": [0, 2], "valid_blurry_frame": [0, 2], "valid_sharp_frame": [0, 2],
            "valid_gt_frame": [0, 2],
            "stamp_valid_loss": [1], "stamp_valid_psnr": [1], "stamp_valid_ssim": [1], "stamp_train_loss": [1],
            "train_HR_events": [0, 2, 4], "train_blurry_frame": [0, 2, 4], "train_sharp_frame": [0, 2, 4], "train_gt_frame": [0, 2, 4],
            "grad_norm/all": [0, 3], "f16/skipped_steps": [0, 3]}
    for g in groups:
        for t in ("weight_norm/%s", "grad_norm/%s", "grad_nonfinite/%s", "weights/%s", "grads/%s"):
            want[t % g] = [0, 3]
    assert steps == want
    # values: the losses train_step returned, bit for bit; the learning rate; the stamp's train loss is iteration 3's
    assert [v["simple_value_bits"] for _, v in tags["train_loss/train"]] == [int(l.numpy().view(np.uint32)) for l in eng.losses]
    assert all(v["simple_value"] == np.float32(1e-4) for _, v in tags["learning rate"])
    assert tags["stamp_train_loss"][0][1]["simple_value_bits"] == int(eng.losses[3].numpy().view(np.uint32))
    assert [tags["stamp_%s" % k][0][1]["simple_value"] for k in eng.VALID_KEYS] == [1.0, 2.0, 3.0]
    assert all(v["simple_value"] > 0 for _, v in tags["steps_per_sec/train"])
    assert tags["f16/skipped_steps"][0][1]["simple_value"] == 3.0
    # statistics: the gradient 'buffer' is -4 .. 4 over A (6 elements) and B (3)
    gflat = eng.bucket.flat.double().numpy()
    assert tags["grad_norm/all"][0][1]["simple_value"] == np.float32(np.sqrt((gflat ** 2).sum()))
    assert tags["grad_norm/A"][0][1]["simple_value"] == np.float32(np.sqrt((gflat[:6] ** 2).sum()))
    assert tags["grad_norm/B"][1][1]["simple_value"] == np.float32(np.sqrt((gflat[6:] ** 2).sum()))
    assert tags["grad_nonfinite/A"][0][1]["simple_value"] == 0.0
    h = tags["grads/A"][0][1]["histo"]
    assert (h["min"], h["max"], h["num"], h["sum"], h["sum_squares"]) == (-4.0, 1.0, 6.0, -9.0, 31.0)
    assert sum(h["bucket"]) == 6 and h["bucket"][0] > 0 and h["bucket"][-1] > 0 and len(h["bucket"]) == len(h["bucket_limit"]) < 1550
    w = eng.optimizer.flat.detach().double().numpy()
    assert tags["weight_norm/B"][0][1]["simple_value"] == np.float32(np.sqrt((w[6:] ** 2).sum()))
    # images: sample 0 through the composer handed in
    from PIL import Image
    import io
    want_pics = _host_panels(batch[1], batch[0], batch[0][:1] * 0.5, batch[4]).numpy()
    for tag, pic in zip(M.TRAIN_IMAGE_TAGS, want_pics):
        for _, v in tags[tag]:
            assert (v["image"]["height"], v["image"]["width"]) == (3, 5)
            assert np.array_equal(np.asarray(Image.open(io.BytesIO(v["image"]["encoded_image_string"]))), pic)
    want_pics = _host_panels(vbatch[1], vbatch[0], vbatch[0] * 0.25, vbatch[4][:, -1]).numpy()
    for tag, pic in zip(M.VALID_IMAGE_TAGS, want_pics):
        assert np.array_equal(np.asarray(Image.open(io.BytesIO(tags[tag][1][1]["image"]["encoded_image_string"]))), pic)
    # the log line takes its loss from the monitor's flush: the same value as without one
    out = capsys.readouterr().out
    assert "Iteration: 0/5 train_loss: %.4e" % eng.losses[0].item() in out and "Iteration: 4/5 train_loss: %.4e" % eng.losses[4].item() in out


def test_rank_one_writes_nothing(tmp_path, monkeypatch):
    eng, mon, _, _ = _run_loop(tmp_path, 1, monkeypatch)
    assert mon.writer is None and not (tmp_path / "log").exists()
    assert eng.keep_panels is False                      # (no panel copy in the step of a rank that writes no images)
    assert mon.last_train_loss == eng.losses[4].item() and mon.valid_iter == 3     # it still took part in every flush


def test_loop_without_a_monitor_is_unchanged(tmp_path, monkeypatch, capsys):
    """telemetry=None (every run without the new keys): the log line's loss comes from reduce_tensor as before, nothing of
    ebfi_amd.monitor is called and no log directory appears."""
    T = _trainer()
    monkeypatch.setattr(T, "save_checkpoint", lambda *a, **k: [])
    monkeypatch.setattr(torch.cuda, "synchronize", lambda *a, **k: None)
    monkeypatch.setattr(M.TrainMonitor, "after_step", lambda *a, **k: (_ for _ in ()).throw(AssertionError("monitor called")))
    eng = FakeEngine()
    st = {"iterations": 3, "save_period": 0, "lr_change_rate": 1, "lr_min": 0.0, "accu_step": 1, "log_step": 1}
    batch = (torch.rand(1, 3, 2, 2),) * 5
    T.train_loop(eng, lambda it, micro: batch, 1, "frames", st, {"do_validation": False}, None, None, None, None, str(tmp_path), {}, 0, 1, 0)
    out = capsys.readouterr().out
    assert all("Iteration: %d/3 train_loss: %.4e" % (i, eng.losses[i].item()) in out for i in range(3))
    assert os.listdir(str(tmp_path)) == [] and eng.keep_panels is False
