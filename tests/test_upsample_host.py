"""Host side of the frame-upsampling step (no GPU): the float64 restatement (tests/upsample_ref.py) against what the reference's
own code gave (tests/golden/upsample_small.npz), the byte law in numpy float32 against the reference's bytes, and the host logic
of ebfi_amd.upsample and generate_dataset/upsampling/upsample.py: crop, sequence discovery, the refusals, timestamps.txt, flags."""
import importlib.util
import os

import numpy as np
import pytest
import torch

import upsample_ref as R
from ebfi_amd import upsample as U

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SCRIPT = os.path.join(ROOT, "ebfi-be_amd", "generate_dataset", "upsampling", "upsample.py")

_cache = {}


def fixture():
    if "fx" not in _cache:
        _cache["fx"] = dict(np.load(os.path.join(ROOT, "tests", "golden", "upsample_small.npz")))
    return _cache["fx"]


def restated_pair():
    """The float64 restatement of the fixture's pair, made once per session and never modified."""
    if "pair" not in _cache:
        fx = fixture()
        I0, I1 = (torch.from_numpy(R.normalise(f)) for f in fx["pair_u8"])
        with torch.no_grad():
            _cache["pair"] = R.upsample_pair(R.flow_state_dict(), R.interp_state_dict(), I0, I1, float(fx["times"][0]), float(fx["times"][1]))
    return _cache["pair"]


def load_script():
    spec = importlib.util.spec_from_file_location("upsample_script", SCRIPT)
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod


def rel(got, want):
    got, want = np.asarray(got, dtype=np.float64), np.asarray(want, dtype=np.float64)
    return np.abs(got - want).max() / np.abs(want).max()


def test_seeded_weights_are_the_fixtures():
    fx = fixture()
    assert float(fx["fc_last_scale"]) == R.FC_LAST_SCALE
    np.testing.assert_allclose(R.checksums(R.flow_state_dict()), fx["checksums_fc"], rtol=1e-12, atol=0)
    np.testing.assert_allclose(R.checksums(R.interp_state_dict()), fx["checksums_at"], rtol=1e-12, atol=0)


def test_fixture_margins():
    fx = fixture()
    assert 3 <= int(fx["N"]) <= 8
    assert 0.2 <= float(fx["flow_max64"]) % 1.0 <= 0.8
    assert fx["frames"].shape == (int(fx["N"]), 3, 64, 96) and fx["frames"].dtype == np.float32


def test_restatement_reproduces_reference():
    """float64 restatement against the reference's float32 outputs, within the float32 noise the generator measured on the
    reference itself (float32 run against float64 run); twice that, since the restatement is a third computation."""
    fx, res = fixture(), restated_pair()
    assert res["N"] == int(fx["N"])
    assert res["timestamps"] == list(fx["timestamps"])
    for name, got, want, noise in (("flow", res["flow_out"], fx["flow_out"], fx["noise_flow"]),
                                   ("frames", res["frames"], fx["frames"], fx["noise_frames"]),
                                   ("intrp", res["intrp"][1], fx["intrp_k1"], fx["noise_intrp"])):
        err = rel(got.numpy(), want)
        print("%s: rel err %.3e (float32 noise of the reference %.3e)" % (name, err, float(noise)))
        assert err <= 2 * float(noise), (name, err, float(noise))


def test_byte_law_matches_reference_levels():
    fx = fixture()
    want = fx["levels"].transpose(0, 3, 1, 2)
    assert np.array_equal(R.frames_to_levels(fx["frames"]), want)
    # I0: the stored bytes -> / 255 - mean -> + mean, * 255, truncate: the reference's own round trip (not always the identity)
    assert np.array_equal(R.levels_f32(R.normalise(fx["pair_u8"][0])), want[0])
    table = U.normalise_table()
    assert np.array_equal(np.stack([table[c][fx["pair_u8"][0][..., c]] for c in range(3)]), R.normalise(fx["pair_u8"][0]))


def test_gray_law():
    lv = np.zeros((3, 1, 4), np.uint8)
    lv[:, 0, 1] = 255
    lv[:, 0, 2] = (255, 0, 0)       # channel 0 (R of the RGB frame) takes the blue coefficient
    lv[:, 0, 3] = (0, 0, 255)
    assert R.gray15(lv).tolist() == [[0, 255, (3735 * 255 + 16384) >> 15, (9798 * 255 + 16384) >> 15]]
    assert sum(R.GRAY15) == 1 << 15


@pytest.mark.parametrize("w,h,box", [(100, 70, (2, 3, 98, 67)), (1280, 720, (0, 8, 1280, 712)), (96, 64, (0, 0, 96, 64)),
                                       (63, 33, (15, 0, 47, 32))])
def test_crop_offsets(w, h, box):
    assert U.crop_box(w, h) == box == R.crop_box(w, h)


def make_png(path, w=40, h=36, seed=0):
    from PIL import Image
    g = np.random.RandomState(seed)
    Image.fromarray(g.randint(0, 256, size=(h, w, 3)).astype(np.uint8)).save(path)


def test_sequence_discovery(tmp_path):
    a = tmp_path / "a" / "deep"
    (a / "imgs").mkdir(parents=True)
    (a / "fps.txt").write_text("240\n")
    for name in ("0002.png", "0000.png", "0001.PNG", "notes.txt"):
        if name.endswith("txt"):
            (a / "imgs" / name).write_text("x")
        else:
            make_png(str(a / "imgs" / name))
    (tmp_path / "b" / "imgs").mkdir(parents=True)          # imgs/ without fps.txt: not a sequence
    found = U.find_sequences(str(tmp_path))
    assert [d for d, _ in found] == [str(a)]
    seq = found[0][1]
    assert seq.file_names == ["0000.png", "0001.PNG", "0002.png"] and len(seq) == 2 and seq.fps == 240.0
    assert seq.times(1) == (1 / 240.0, 2 / 240.0)
    img = seq.load_rgb_u8(seq.path(0))
    assert img.shape == (32, 32, 3) and img.dtype == np.uint8


def test_video_only_directory_fails_loudly(tmp_path):
    d = tmp_path / "clips" / "v1"
    d.mkdir(parents=True)
    (d / "GOPR0001.MP4").write_bytes(b"")
    with pytest.raises(NotImplementedError) as e:
        U.find_sequences(str(tmp_path))
    assert str(d) in str(e.value) and "GOPR0001.MP4" in str(e.value)
    (d / "fps.txt").write_text("30\n")                       # fps.txt + a video, no imgs/: still a video sequence
    with pytest.raises(NotImplementedError) as e:
        U.sequence_or_none(str(d))
    assert str(d) in str(e.value)


def test_existing_output_dir_is_refused(tmp_path):
    src, dst = tmp_path / "in", tmp_path / "out"
    src.mkdir()
    dst.mkdir()
    with pytest.raises(FileExistsError) as e:
        U.Upsampler(str(src), str(dst), "cuda:0", checkpoint=str(tmp_path / "none.ckpt"))
    assert str(dst) in str(e.value)
    with pytest.raises(FileExistsError):
        load_script().main(["--input_dir", str(src), "--output_dir", str(dst)])


def test_missing_checkpoint_names_the_path_and_creates_nothing(tmp_path, monkeypatch):
    import urllib.request

    def no_network(*a, **k):
        raise AssertionError("a URL was opened")
    monkeypatch.setattr(urllib.request, "urlopen", no_network)
    src, dst, ckpt = tmp_path / "in", tmp_path / "out", tmp_path / "ckpt" / "SuperSloMo.ckpt"
    src.mkdir()
    with pytest.raises(FileNotFoundError) as e:
        U.Upsampler(str(src), str(dst), "cuda:0", checkpoint=str(ckpt))
    assert str(ckpt) in str(e.value)
    assert not dst.exists() and not ckpt.parent.exists()
    src_text = open(U.__file__).read() + open(SCRIPT).read()
    assert "urlopen" not in src_text and "http" not in src_text


def test_timestamps_text_and_pair_times():
    t0, t1 = 3 / 240.0, 4 / 240.0
    stamps = U.pair_timestamps(t0, t1, 4)
    assert stamps == [t0, t0 + 0.25 * (t1 - t0), t0 + 0.5 * (t1 - t0), t0 + 0.75 * (t1 - t0)] == list(fixture()["timestamps"])
    assert U.pair_timestamps(0.5, 1.0, 0) == [0.5] == U.pair_timestamps(0.5, 1.0, 1)
    assert U.timestamps_text([0.0, 1 / 240.0, 0.0125]) == "0.0\n0.004166666666666667\n0.0125\n"
    assert U.frame_count(3.5255) == 4 and U.frame_count(4.0) == 4 and U.frame_count(0.0) == 0
    with pytest.raises(ValueError):
        U.frame_count(float("nan"))


def test_flag_defaults():
    mod = load_script()
    flags = mod.get_flags(["--input_dir", "a", "--output_dir", "b"])
    assert (flags.input_dir, flags.output_dir, flags.device) == ("a", "b", "cuda:0")
    assert flags.checkpoint == "./upsampling/checkpoint/SuperSloMo.ckpt" == U.DEFAULT_CHECKPOINT
    assert flags.imgs_dirname == "imgs" == U.IMGS_DIRNAME
    assert mod.get_flags(["--input_dir", "a", "--output_dir", "b", "--imgs_dirname", "mono"]).imgs_dirname == "mono"
    with pytest.raises(SystemExit):
        mod.get_flags(["--input_dir", "a"])


def test_layer_table_matches_restatement():
    for cin, cout in ((6, 4), (20, 5)):
        assert U.unet_layers(cin, cout) == R.unet_layers(cin, cout)
    sd = R.flow_state_dict()
    assert sorted(sd) == sorted(p + s for p, _, _, _ in U.unet_layers(6, 4) for s in (".weight", ".bias"))
    assert sum(v.numel() for v in sd.values()) + sum(v.numel() for v in R.interp_state_dict().values()) > 39e6
