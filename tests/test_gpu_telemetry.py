"""The training monitor on the device: ebfi_segment_stats against its numpy float64 restatement (tests/telemetry_ref.py), its
reproducibility and graph capture, the four pictures of a batch against the reference's compositions, and one instrumented
train_ours.py run against the same run without the monitor."""
import io
import os
import subprocess
import sys

import numpy as np
import pytest
import torch
import yaml

import eventvis_ref
import telemetry_ref as TR
import tfevents_ref as R
from ebfi_amd import telemetry

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
PKG = os.path.join(ROOT, "ebfi-be_amd")

# segment lengths: empty, one element, around the 64-lane wave, 4097 = one 4096-element chunk plus one element (two workgroups,
# starting at the odd offset 193), 63 starting at the odd offset 1 (not a multiple of 4), and 9001 (three chunks, a ragged last one)
SIZES = [0, 1, 63, 64, 65, 4097, 9001, 0]
OFFSETS = [0] + list(np.cumsum(SIZES))

# a table fp32 values can sit on exactly (all but its two ends): -2, -0.5, +-0, the smallest denormal, 0.25 and 1 are in the data
EXACT_LIMITS = np.array([-1e21, -2.0, -0.5, 0.0, 2.0 ** -149, 0.25, 1.0, 1e30])


def _specials(limits):
    """fp32 values around the table: on a limit where fp32 can hit it, else the two fp32 neighbours of the limit (decided rightly
    only by a float64 comparison), +-0, denormals, values below the smallest and above the largest 1.1^k limit, non-finite ones."""
    near = []
    for k in (0, 1, len(limits) // 2 - 3, len(limits) // 2 + 3, len(limits) - 2):
        f = np.float32(limits[k])
        if np.isfinite(f):
            near += [f, np.nextafter(f, np.float32(np.inf)), np.nextafter(f, np.float32(-np.inf))]
    fixed = [0.0, -0.0, 1e-45, -1e-40, 1.1754942e-38, 1e-13, -1e-13, 1e21, -1e21, 0.25, -0.5, -2.0, 1.0, np.nan, np.inf, -np.inf]
    return np.array(near + fixed, dtype=np.float32)


def _data(limits, seed, specials=True):
    rng = np.random.default_rng(seed)
    n = OFFSETS[-1]
    x = (rng.standard_normal(n) * np.exp(rng.uniform(-30, 3, n))).astype(np.float32)
    sp = _specials(limits) if specials else np.zeros(0, np.float32)
    for s, size in enumerate(SIZES):
        if size >= 63:                                   # every special value in every segment that has room, at random places
            at = OFFSETS[s] + rng.choice(size, size=min(size, sp.size), replace=False)
            x[at] = sp[:at.size]
    x[OFFSETS[1]] = np.float32(np.nan)                   # the one-element segment holds nothing finite
    return x


# "plain": magnitudes 1e-13 .. 20 only -- without the 1e21 / 1e30 values that set the ulp of the other cases' sums, the bar on the
# sums is 4 ulp of a sum of order 10
@pytest.fixture(scope="module", params=["tensorflow", "exact", "plain"])
def case(request):
    limits = EXACT_LIMITS if request.param == "exact" else TR.tf_default_limits()
    x = _data(limits, {"tensorflow": 11, "exact": 12, "plain": 13}[request.param], specials=request.param != "plain")
    ref = TR.segment_stats_ref(x, OFFSETS, limits)
    return limits, x, ref, TR.sum_bounds(x, OFFSETS)


def _check(moments, hist, ref, bounds):
    want_m, want_h = ref
    moments, hist = moments.cpu().numpy(), hist.cpu().numpy()
    assert np.array_equal(hist, want_h)                                            # histograms: exactly
    assert np.array_equal(moments[:, :4], want_m[:, :4])                           # counts, min, max: exactly
    for s, (b_sum, b_sq) in enumerate(bounds):
        print("segment %d: sum error %.3e (bar %.3e), sum of squares error %.3e (bar %.3e)"
              % (s, abs(moments[s, 4] - want_m[s, 4]), b_sum, abs(moments[s, 5] - want_m[s, 5]), b_sq))
        assert abs(moments[s, 4] - want_m[s, 4]) <= b_sum and abs(moments[s, 5] - want_m[s, 5]) <= b_sq


def test_segment_stats_against_the_restatement(case):
    limits, x, ref, bounds = case
    moments, hist = telemetry.segment_stats(torch.from_numpy(x).cuda(), OFFSETS, limits)
    torch.cuda.synchronize()
    _check(moments, hist, ref, bounds)
    m = moments.cpu().numpy()
    assert list(m[0]) == [0, 0, np.inf, -np.inf, 0, 0] and list(m[1]) == [0, 1, np.inf, -np.inf, 0, 0]   # empty / nothing finite
    assert m[:, 1].sum() == np.count_nonzero(~np.isfinite(x)) and hist.sum().item() == np.count_nonzero(np.isfinite(x))


def test_two_calls_give_the_same_bits(case):
    limits, x, _, _ = case
    st = telemetry.SegmentStats(OFFSETS, x.size, "cuda", limits)
    flat = torch.from_numpy(x).cuda()
    first = [t.clone() for t in st.run(flat)]
    st.workspace.fill_(float("nan"))                     # (nothing of an earlier call may be read)
    second = st.run(flat)
    torch.cuda.synchronize()
    assert torch.equal(first[0].view(torch.int64), second[0].view(torch.int64)) and torch.equal(first[1], second[1])


def test_a_view_that_starts_mid_buffer(case):
    """FlatGradBucket.flat is a view of the wire buffer; a base pointer that is only 4-byte aligned must read the same."""
    limits, x, ref, bounds = case
    wide = torch.zeros(x.size + 5, device="cuda")
    wide[3:3 + x.size] = torch.from_numpy(x).cuda()
    moments, hist = telemetry.segment_stats(wide[3:3 + x.size], OFFSETS, limits)
    _check(moments, hist, ref, bounds)


def test_offsets_outside_the_buffer_are_clamped():
    """The table lives on the device and is never read by the host: the kernels clamp it."""
    x = torch.arange(100, dtype=torch.float32, device="cuda")
    st = telemetry.SegmentStats([0, 40, 100], 100, "cuda", [10.0, 1e9])
    st.offsets.copy_(torch.tensor([-5, 40, 10 ** 12], device="cuda"))
    m, h = st.run(x)
    assert m[:, 0].tolist() == [40, 60] and m[:, 3].tolist() == [39, 99] and h.tolist() == [[11, 29], [0, 60]]


def test_captured_call_replays_on_changed_data(case):
    limits, x, ref, bounds = case
    st = telemetry.SegmentStats(OFFSETS, x.size, "cuda", limits)
    static = torch.zeros(x.size, device="cuda")
    st.run(static)                                       # (library and workspace are ready before the capture)
    torch.cuda.synchronize()
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        st.run(static)
    graph.replay()
    torch.cuda.synchronize()
    assert st.moments[2].tolist() == [63, 0, 0, 0, 0, 0] and st.hist.sum().item() == x.size
    static.copy_(torch.from_numpy(x))
    graph.replay()
    torch.cuda.synchronize()
    _check(st.moments, st.hist, ref, bounds)


# ------------------------------------------------------------------ the four pictures
def test_panels_equal_the_reference_compositions():
    from ebfi_amd.monitor import device_panels
    g = torch.Generator().manual_seed(5)
    B, TB, H, W = 2, 3, 32, 48
    frame, target = torch.rand(B, 3, H, W, generator=g), torch.rand(B, 3, H, W, generator=g)
    sharp = torch.randn(B, 3, H, W, generator=g) * 0.7 + 0.5                       # an unclamped prediction: values on both sides
    event = torch.poisson(torch.full((B, TB, 2, H, W), 0.6), generator=g)
    assert (sharp < 0).any() and (sharp > 1).any()
    got = device_panels(event.cuda(), frame.cuda(), sharp.cuda(), target.cuda()).cpu().numpy()
    assert got.shape == (4, H, W, 3) and got.dtype == np.uint8
    cast = lambda x: (x[0].numpy() * 255).transpose(1, 2, 0).astype("uint8")       # train_ours.py:301-307 of the reference
    want = [eventvis_ref.plot_event_cnt_numpy(event.sum(1)[0].numpy().transpose(1, 2, 0), "green_red", is_black_background=True),
            cast(frame), cast(sharp.clamp(0, 1)), cast(target)]
    for name, a, b in zip(("events", "blurry", "sharp", "gt"), got, want):
        assert np.array_equal(a, b), name


# ------------------------------------------------------------------ an instrumented run against the plain one
# train_ours.py with Engine.train_step wrapped: argv = [script, where to save (losses, gradient norms), the script's own arguments]
PLAIN_RUN = """
import importlib.util, sys, torch
script, out = sys.argv[1], sys.argv[2]
spec = importlib.util.spec_from_file_location("plain_train_ours", script)
T = importlib.util.module_from_spec(spec)
spec.loader.exec_module(T)
from ebfi_amd.engine import Engine
losses, norms, step = [], [], Engine.train_step
def recording(self, *inputs):
    loss = step(self, *inputs)
    losses.append(loss.detach().clone())
    norms.append(self.bucket.flat.double().norm())
    return loss
Engine.train_step = recording
T.main(sys.argv[3:])
torch.save((torch.stack(losses).cpu(), torch.stack(norms).cpu()), out)
"""


def test_instrumented_run_equals_the_plain_run(tmp_path):
    cfg = yaml.safe_load(open(os.path.join(PKG, "config", "train_ours.yml")))
    cfg["model"]["args"].update(FrameBasech=16, EventBasech=16, InterCH=16, TB=4, step=2, channels=[4, 4, 8, 8])
    cfg["trainer"].update(batch_size=2, height=64, width=64, output_path=str(tmp_path / "plain"), do_validation=True, valid_batches=2)
    cfg["trainer"]["iteration_based_train"].update(valid_step=3)                   # one stamp, at iteration 3, over two batches
    cfg["valid_dataloader"]["dataset"]["NumFramePerPeriod"] = 2
    plain = tmp_path / "plain.yml"
    plain.write_text(yaml.safe_dump(cfg))
    cfg["trainer"].update(output_path=str(tmp_path / "tb"), tensorboard=True,
                          vis={"enabled": True, "train_img_writer_num": 2, "valid_img_writer_num": 2},
                          telemetry={"stats_step": 2, "group_depth": 2})
    instrumented = tmp_path / "tb.yml"
    instrumented.write_text(yaml.safe_dump(cfg))
    argv = ["-id", "t", "--graph", "--iterations", "6"]
    r = subprocess.run([sys.executable, os.path.join(PKG, "train_ours.py"), "-c", str(instrumented)] + argv, capture_output=True,
                       text=True, env=dict(os.environ, PYTHONPATH=PKG), timeout=600)
    assert r.returncode == 0, r.stderr[-2000:]

    # the same run without the monitor, in a process of its own: the losses train_step returns and the norm of the packed gradient
    r = subprocess.run([sys.executable, "-c", PLAIN_RUN, os.path.join(PKG, "train_ours.py"), str(tmp_path / "plain.pt"), "-c", str(plain)]
                       + argv, capture_output=True, text=True, env=dict(os.environ, PYTHONPATH=PKG), timeout=600)
    assert r.returncode == 0, r.stderr[-2000:]
    losses, norms = (v.numpy() for v in torch.load(str(tmp_path / "plain.pt")))
    assert len(losses) == 6 and not (tmp_path / "plain" / "log").exists()

    log_dir = tmp_path / "tb" / "log" / "Ours" / "t"
    (name,) = os.listdir(str(log_dir))
    events = R.read_events(str(log_dir / name))          # (decodes: every CRC, every field)
    assert events[0]["file_version"] == "brain.Event:2"
    tags = R.by_tag(events)
    got = tags["train_loss/train"]
    assert [s for s, _ in got] == list(range(6)) and [s for s, _ in tags["learning rate"]] == list(range(6))
    print("train_loss/train:", [v["simple_value"] for _, v in got], "plain run:", losses.tolist())
    assert [v["simple_value_bits"] for _, v in got] == [int(v) for v in losses.view(np.uint32)]
    assert [s for s, _ in tags["grad_norm/all"]] == [0, 2, 4]
    for s, v in tags["grad_norm/all"]:
        print("grad_norm/all at %d: %.9e, float64 norm of bucket.flat %.9e" % (s, v["simple_value"], norms[s]))
        assert abs(v["simple_value"] - norms[s]) <= 1e-6 * norms[s]
    assert [s for s, _ in tags["f16/skipped_steps"]] == [0, 2, 4] and all(v["simple_value"] == 0 for _, v in tags["f16/skipped_steps"])
    groups = sorted(t.split("/", 1)[1] for t in tags if t.startswith("weights/"))
    assert len(groups) > 3 and "Modification.KernelConv" in groups
    for g in groups:
        for t in ("weight_norm/", "grad_norm/", "grad_nonfinite/", "weights/", "grads/"):
            assert [s for s, _ in tags[t + g]] == [0, 2, 4], t + g
        h = tags["weights/" + g][-1][1]["histo"]
        assert h["num"] == sum(h["bucket"]) > 0 and h["bucket"][0] > 0 and h["bucket"][-1] > 0
        assert h["min"] <= h["bucket_limit"][0] and h["bucket_limit"][-1] >= h["max"]
    from PIL import Image
    for t in ("train_HR_events", "train_blurry_frame", "train_sharp_frame", "train_gt_frame"):
        assert [s for s, _ in tags[t]] == [0, 2, 4]
        pic = np.asarray(Image.open(io.BytesIO(tags[t][-1][1]["image"]["encoded_image_string"])))
        assert pic.shape == (64, 64, 3) and pic.dtype == np.uint8 and (t == "train_sharp_frame" or pic.any())

    # the validation side: one (batch, load) per batch, pictures of every second one, one stamp
    assert [s for s, _ in tags["valid_loss/valid"]] == [0, 1]
    for t in ("valid_HR_events", "valid_blurry_frame", "valid_sharp_frame", "valid_gt_frame"):
        assert [s for s, _ in tags[t]] == [0]
        pic = np.asarray(Image.open(io.BytesIO(tags[t][0][1]["image"]["encoded_image_string"])))
        assert pic.shape == (64, 64, 3) and pic.any()
    for key in ("valid_loss", "valid_psnr", "valid_ssim", "train_loss"):
        assert [s for s, _ in tags["stamp_" + key]] == [1]
    assert tags["stamp_train_loss"][0][1]["simple_value_bits"] == got[3][1]["simple_value_bits"]
    stamp_loss = tags["stamp_valid_loss"][0][1]["simple_value"]
    assert stamp_loss == pytest.approx(np.mean([v["simple_value"] for _, v in tags["valid_loss/valid"]]), rel=1e-6)

    # the monitor changes nothing the run computes: the checkpoints hold the same bits
    a = torch.load(str(tmp_path / "tb" / "models" / "Ours" / "t" / "checkpoint-iteration5.pth"), map_location="cpu", weights_only=False)
    b = torch.load(str(tmp_path / "plain" / "models" / "Ours" / "t" / "checkpoint-iteration5.pth"), map_location="cpu", weights_only=False)
    assert a["model"]["states"].keys() == b["model"]["states"].keys()
    assert all(torch.equal(a["model"]["states"][k], b["model"]["states"][k]) for k in a["model"]["states"])
    sa, sb = a["optimizer"]["states"]["state"], b["optimizer"]["states"]["state"]
    assert sa.keys() == sb.keys() and all(torch.equal(sa[i][k], sb[i][k]) for i in sa for k in ("exp_avg", "exp_avg_sq"))
