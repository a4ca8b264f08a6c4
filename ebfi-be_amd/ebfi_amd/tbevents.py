"""TensorBoard event files without TensorBoard: the reference logs through torch.utils.tensorboard (train_ours.py:283-319), which
cannot be imported without the `tensorboard` package; this writer needs the standard library and numpy only.

File: ``events.out.tfevents.<int time>.<host>.<pid>``, a sequence of records
    uint64 length (LE) | uint32 masked CRC32C of those 8 bytes | payload | uint32 masked CRC32C of the payload
with CRC32C the Castagnoli polynomial (``crc32c(b"123456789") == 0xE3069283``) and the mask
``((c >> 15 | c << 17) + 0xA282EAD8) & 0xFFFFFFFF``.  A payload is a protobuf ``Event``, encoded by hand:
    Event           wall_time = 1 (double), step = 2 (varint), file_version = 3 (string), summary = 5
    Summary         value = 1 (repeated)
    Summary.Value   tag = 1, simple_value = 2 (float), image = 4, histo = 5
    Image           height = 1, width = 2, colorspace = 3, encoded_image_string = 4
    HistogramProto  min = 1, max = 2, num = 3, sum = 4, sum_squares = 5 (doubles), bucket_limit = 6, bucket = 7 (packed doubles)
The first record is ``file_version = "brain.Event:2"``.  Images are PNG-encoded here on zlib (8-bit RGB, filter 0).
No machine of this project has TensorBoard: that the viewer opens these files is unverified; tests/tfevents_ref.py decodes them
from the same format text.
"""
import os
import socket
import struct
import time
import zlib

import numpy as np

FILE_VERSION = "brain.Event:2"


def _crc_table():
    table = []
    for n in range(256):
        c = n
        for _ in range(8):
            c = (c >> 1) ^ 0x82F63B78 if c & 1 else c >> 1      # (the Castagnoli polynomial, reflected)
        table.append(c)
    return table


_TABLE = _crc_table()
_NP_TABLE = np.array(_TABLE, dtype=np.uint32)
_LANE = 64                               # bytes per lane of the vectorised form
_SHORT = 4 * _LANE                       # below this the byte loop is faster


def _crc32c_bytewise(data):
    c = 0xFFFFFFFF
    for b in bytes(data):
        c = _TABLE[(c ^ b) & 0xFF] ^ (c >> 8)
    return c ^ 0xFFFFFFFF


def _advance(tables, s):
    """`tables` [4, 256]: the register after some fixed number of zero bytes, for every value of each register byte (the update is
    linear over GF(2), so the four bytes' images add up)."""
    return tables[0][s & 0xFF] ^ tables[1][(s >> 8) & 0xFF] ^ tables[2][(s >> 16) & 0xFF] ^ tables[3][s >> 24]


def _lane_tables():
    t = (np.arange(256, dtype=np.uint32)[None, :] << (8 * np.arange(4, dtype=np.uint32))[:, None]).astype(np.uint32)
    for _ in range(_LANE):
        t = _NP_TABLE[t & 0xFF] ^ (t >> 8)
    return t


_LANE_TABLES = _lane_tables()


def crc32c(data):
    """CRC32C (Castagnoli) of a bytes-like object.  A PNG of a training panel is a few hundred kilobytes: long inputs are cut into
    lanes of 64 bytes whose registers advance together (one table step per byte position, vectorised over the lanes) and are then
    folded pairwise, the left register of a pair advanced over the right one's length -- the same value as the byte loop."""
    data = bytes(data)
    n = len(data)
    if n < _SHORT:
        return _crc32c_bytewise(data)
    lanes = 1
    while lanes * _LANE < n:
        lanes *= 2
    # (the initial register 0xFFFFFFFF is the same as inverting the first four bytes; zero bytes in FRONT of those leave a zero
    #  register at zero, so the message is padded there to a power-of-two lane count)
    buf = np.zeros(lanes * _LANE, dtype=np.uint8)
    buf[lanes * _LANE - n:] = np.frombuffer(data, dtype=np.uint8)
    buf[lanes * _LANE - n:lanes * _LANE - n + 4] ^= 0xFF
    cols = buf.reshape(lanes, _LANE).astype(np.uint32)
    c = np.zeros(lanes, dtype=np.uint32)
    for j in range(_LANE):
        c = _NP_TABLE[(c ^ cols[:, j]) & 0xFF] ^ (c >> 8)
    tables = _LANE_TABLES
    while c.size > 1:
        c = _advance(tables, c[0::2]) ^ c[1::2]
        tables = _advance(tables, tables)
    return int(c[0]) ^ 0xFFFFFFFF


def masked_crc32c(data):
    c = crc32c(data)
    return (((c >> 15) | (c << 17)) + 0xA282EAD8) & 0xFFFFFFFF


# ---------------------------------------------------------------------------------------------------- protobuf wire format
def _varint(v):
    v = int(v)
    if v < 0:
        v += 1 << 64                     # (int64 two's complement: ten bytes)
    out = bytearray()
    while True:
        b = v & 0x7F
        v >>= 7
        if v:
            out.append(b | 0x80)
        else:
            out.append(b)
            return bytes(out)


def _key(field, wire):
    return _varint((field << 3) | wire)


def _f_varint(field, v):
    return _key(field, 0) + _varint(v)


def _f_double(field, v):
    return _key(field, 1) + struct.pack("<d", float(v))


def _f_float(field, v):
    return _key(field, 5) + struct.pack("<f", float(v))


def _f_bytes(field, data):
    data = data.encode("utf-8") if isinstance(data, str) else bytes(data)
    return _key(field, 2) + _varint(len(data)) + data


def _f_packed_doubles(field, values):
    return _f_bytes(field, np.asarray(values, dtype="<f8").tobytes())


def encode_png(hwc_uint8):
    """uint8 [H, W, 3] -> PNG bytes: 8-bit RGB, every row with filter 0, one zlib stream (level 1: the encoder runs beside a
    training loop, and unfiltered camera rows gain little from a longer search)."""
    img = np.ascontiguousarray(hwc_uint8)
    if img.dtype != np.uint8 or img.ndim != 3 or img.shape[2] != 3 or img.shape[0] < 1 or img.shape[1] < 1:
        raise ValueError("encode_png: expected uint8 [H, W, 3], got %s %r" % (img.dtype, img.shape))
    h, w = img.shape[:2]
    rows = np.zeros((h, 1 + 3 * w), dtype=np.uint8)      # (column 0: the filter byte)
    rows[:, 1:] = img.reshape(h, 3 * w)

    def chunk(kind, data):
        return struct.pack(">I", len(data)) + kind + data + struct.pack(">I", zlib.crc32(kind + data) & 0xFFFFFFFF)

    return (b"\x89PNG\r\n\x1a\n" + chunk(b"IHDR", struct.pack(">IIBBBBB", w, h, 8, 2, 0, 0, 0))
            + chunk(b"IDAT", zlib.compress(rows.tobytes(), 1)) + chunk(b"IEND", b""))


def _event(payload_field, wall_time, step=None):
    ev = _f_double(1, wall_time)
    if step is not None:
        ev += _f_varint(2, step)
    return ev + payload_field


def _summary(tag, value_field):
    return _f_bytes(5, _f_bytes(1, _f_bytes(1, tag) + value_field))


class EventWriter:
    """add_scalar / add_image / add_histogram append one record each; records are buffered by the file object and reach the disk
    on flush() / close()."""

    def __init__(self, log_dir):
        os.makedirs(log_dir, exist_ok=True)
        self.log_dir = log_dir
        self.path = os.path.join(log_dir, "events.out.tfevents.%d.%s.%d" % (int(time.time()), socket.gethostname(), os.getpid()))
        self._fh = open(self.path, "ab")
        self._record(_event(_f_bytes(3, FILE_VERSION), time.time()))
        self.flush()

    def _record(self, payload):
        header = struct.pack("<Q", len(payload))
        self._fh.write(header + struct.pack("<I", masked_crc32c(header)) + payload + struct.pack("<I", masked_crc32c(payload)))

    def add_scalar(self, tag, value, step, wall_time=None):
        self._record(_event(_summary(tag, _f_float(2, value)), time.time() if wall_time is None else wall_time, step))

    def add_image(self, tag, hwc_uint8, step, wall_time=None):
        img = np.asarray(hwc_uint8)
        image = _f_varint(1, img.shape[0]) + _f_varint(2, img.shape[1]) + _f_varint(3, 3) + _f_bytes(4, encode_png(img))
        self._record(_event(_summary(tag, _f_bytes(4, image)), time.time() if wall_time is None else wall_time, step))

    def add_histogram(self, tag, stats, step, wall_time=None):
        """stats: {"min", "max", "num", "sum", "sum_squares", "bucket_limit": [k], "bucket": [k]} (a HistogramProto, field for
        field; bucket i counts the values in (bucket_limit[i - 1], bucket_limit[i]])."""
        limits, counts = np.asarray(stats["bucket_limit"], dtype=np.float64), np.asarray(stats["bucket"], dtype=np.float64)
        if limits.shape != counts.shape or limits.ndim != 1:
            raise ValueError("add_histogram: bucket_limit %r and bucket %r must be equally long vectors" % (limits.shape, counts.shape))
        histo = (_f_double(1, stats["min"]) + _f_double(2, stats["max"]) + _f_double(3, stats["num"]) + _f_double(4, stats["sum"])
                 + _f_double(5, stats["sum_squares"]) + _f_packed_doubles(6, limits) + _f_packed_doubles(7, counts))
        self._record(_event(_summary(tag, _f_bytes(5, histo)), time.time() if wall_time is None else wall_time, step))

    def flush(self):
        if self._fh is not None:
            self._fh.flush()

    def close(self):
        if self._fh is not None:
            self._fh.flush()
            self._fh.close()
            self._fh = None
