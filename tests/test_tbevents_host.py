"""ebfi_amd.tbevents without a GPU: the CRC32C vector and mask, the record framing, the hand-encoded protobuf and the PNG encoder,
read back by tests/tfevents_ref.py (a decoder written separately from the format text) and by PIL."""
import io
import os
import re
import struct

import numpy as np
import pytest

import tfevents_ref as R
from ebfi_amd import tbevents as T


def test_crc32c_vector_and_mask():
    assert T.crc32c(b"123456789") == 0xE3069283
    assert R.crc32c_bitwise(b"123456789") == 0xE3069283
    assert T.crc32c(b"") == 0
    c = 0xE3069283
    assert T.masked_crc32c(b"123456789") == (((c >> 15) | (c << 17)) + 0xA282EAD8) & 0xFFFFFFFF == R.mask(c)
    assert T.masked_crc32c(b"123456789") < 1 << 32


@pytest.mark.parametrize("n", [1, 3, 4, 5, 255, 256, 257, 320, 4095, 4096, 4097, 70001])
def test_crc32c_lane_form_equals_the_bit_loop(n):
    """Below 256 bytes the writer runs a byte loop, above it the 64-byte-lane form with a pairwise fold: lengths on both sides,
    lane counts that are and are not powers of two, and a message that starts mid-lane."""
    data = np.random.default_rng(n).integers(0, 256, n, dtype=np.uint8).tobytes()
    assert T.crc32c(data) == R.crc32c_bitwise(data)
    zeros = bytes(n)                                     # (leading zeros must not vanish into the front padding)
    assert T.crc32c(zeros) == R.crc32c_bitwise(zeros)


def _png_pixels(blob):
    from PIL import Image
    img = Image.open(io.BytesIO(blob))
    assert img.format == "PNG" and img.mode == "RGB"
    return np.asarray(img)


@pytest.mark.parametrize("hw", [(1, 1), (3, 5), (32, 48), (5, 3)])
def test_png_decodes_to_the_same_pixels(hw):
    img = np.random.default_rng(hw[0] * 100 + hw[1]).integers(0, 256, hw + (3,), dtype=np.uint8)
    blob = T.encode_png(img)
    assert blob[:8] == b"\x89PNG\r\n\x1a\n"
    assert struct.unpack(">II", blob[16:24]) == (hw[1], hw[0]) and blob[24:29] == bytes([8, 2, 0, 0, 0])
    assert np.array_equal(_png_pixels(blob), img)


def test_png_refuses_what_it_does_not_encode():
    for bad in (np.zeros((2, 2), np.uint8), np.zeros((2, 2, 4), np.uint8), np.zeros((2, 2, 3), np.float32),
                np.zeros((0, 2, 3), np.uint8)):
        with pytest.raises(ValueError):
            T.encode_png(bad)


def test_file_round_trip(tmp_path):
    rng = np.random.default_rng(7)
    w = T.EventWriter(str(tmp_path / "log"))
    name = os.path.basename(w.path)
    assert re.fullmatch(r"events\.out\.tfevents\.\d+\..+\.%d" % os.getpid(), name)
    scalars = [np.float32(0.1), np.float32(-3.5e-7), np.float32(np.inf), np.float32(1e-42)]
    for step, v in enumerate(scalars):
        w.add_scalar("train_loss/train", v, step * 7)
    imgs = {hw: rng.integers(0, 256, hw + (3,), dtype=np.uint8) for hw in ((1, 1), (3, 5))}
    for k, (hw, img) in enumerate(imgs.items()):
        w.add_image("train_gt_frame", img, 300 + k)
    limits = [-1.0, 0.0, 1e-12, 2.5]
    histo = {"min": -0.5, "max": 2.25, "num": 9.0, "sum": 3.75, "sum_squares": 11.0, "bucket_limit": limits, "bucket": [1, 0, 3, 5]}
    w.add_histogram("weights/A.b", histo, 1 << 33)       # (a step that needs more than four varint bytes)
    w.flush()
    events = R.read_events(w.path)                       # (every CRC is checked in there)
    w.close()
    assert events[0].get("file_version") == "brain.Event:2" and events[0]["values"] == []
    assert all("file_version" not in e and e["wall_time"] > 1e9 for e in events[1:])
    tags = R.by_tag(events)
    assert sorted(tags) == ["train_gt_frame", "train_loss/train", "weights/A.b"]
    got = tags["train_loss/train"]
    assert [s for s, _ in got] == [0, 7, 14, 21]
    assert [v["simple_value_bits"] for _, v in got] == [int(np.float32(x).view(np.uint32)) for x in scalars]
    for (step, v), (hw, img) in zip(tags["train_gt_frame"], imgs.items()):
        im = v["image"]
        assert (im["height"], im["width"], im["colorspace"]) == (hw[0], hw[1], 3)
        assert np.array_equal(_png_pixels(im["encoded_image_string"]), img)
    assert [s for s, _ in tags["train_gt_frame"]] == [300, 301]
    (step, v), = tags["weights/A.b"]
    h = v["histo"]
    assert step == 1 << 33
    assert (h["min"], h["max"], h["num"], h["sum"], h["sum_squares"]) == (-0.5, 2.25, 9.0, 3.75, 11.0)
    assert h["bucket_limit"] == limits and h["bucket"] == [1.0, 0.0, 3.0, 5.0]


def test_histogram_refuses_ragged_buckets(tmp_path):
    w = T.EventWriter(str(tmp_path))
    with pytest.raises(ValueError):
        w.add_histogram("h", {"min": 0, "max": 0, "num": 0, "sum": 0, "sum_squares": 0, "bucket_limit": [1.0, 2.0], "bucket": [1]}, 0)
    w.close()
    w.close()                                            # (closing twice is harmless)


def test_writer_needs_nothing_beyond_numpy():
    """The module must import where neither TensorBoard, TensorFlow, protobuf, PIL nor torch is installed."""
    src = open(T.__file__).read()
    imported = set(re.findall(r"^(?:import\s+(\w+)|from\s+(\w+)[\w.]*\s+import\s)", src, flags=re.M))
    imported = {a or b for a, b in imported}
    assert imported <= {"os", "socket", "struct", "time", "zlib", "numpy"}, imported
