"""A reader of TensorBoard event files, written for the tests from the format text alone (it shares no code with
ebfi_amd.tbevents, not even the CRC table: the CRC here shifts bit by bit):

    record   uint64 length (LE) | uint32 masked CRC32C of those 8 bytes | payload | uint32 masked CRC32C of the payload
    CRC32C   Castagnoli polynomial 0x1EDC6F41 (reflected 0x82F63B78), init and final xor 0xFFFFFFFF;
             mask(c) = ((c >> 15 | c << 17) + 0xA282EAD8) mod 2^32
    Event           wall_time = 1 double, step = 2 varint, file_version = 3 string, summary = 5 message
    Summary         value = 1 repeated message
    Summary.Value   tag = 1 string, simple_value = 2 float, image = 4 message, histo = 5 message
    Image           height = 1, width = 2, colorspace = 3 varints, encoded_image_string = 4 bytes
    HistogramProto  min = 1, max = 2, num = 3, sum = 4, sum_squares = 5 doubles, bucket_limit = 6, bucket = 7 packed doubles
"""
import struct


def crc32c_bitwise(data):
    c = 0xFFFFFFFF
    for byte in data:
        c ^= byte
        for _ in range(8):
            c = (c >> 1) ^ (0x82F63B78 if c & 1 else 0)
    return c ^ 0xFFFFFFFF


def mask(c):
    return ((((c >> 15) | (c << 17)) & 0xFFFFFFFF) + 0xA282EAD8) & 0xFFFFFFFF


def read_records(path):
    """-> [payload bytes]; every length CRC and payload CRC is checked, a truncated tail is an error."""
    blob = open(path, "rb").read()
    out, pos = [], 0
    while pos < len(blob):
        assert pos + 12 <= len(blob), "truncated record header at %d" % pos
        header = blob[pos:pos + 8]
        (length,) = struct.unpack("<Q", header)
        (hcrc,) = struct.unpack("<I", blob[pos + 8:pos + 12])
        assert hcrc == mask(crc32c_bitwise(header)), "length CRC mismatch at %d" % pos
        pos += 12
        assert pos + length + 4 <= len(blob), "truncated payload at %d" % pos
        payload = blob[pos:pos + length]
        (pcrc,) = struct.unpack("<I", blob[pos + length:pos + length + 4])
        assert pcrc == mask(crc32c_bitwise(payload)), "payload CRC mismatch at %d" % pos
        out.append(payload)
        pos += length + 4
    return out


def _varint(buf, pos):
    v, shift = 0, 0
    while True:
        b = buf[pos]
        pos += 1
        v |= (b & 0x7F) << shift
        if not b & 0x80:
            return v, pos
        shift += 7


def fields(buf):
    """protobuf message -> [(field number, wire type, value)]: varint -> int, 64-bit / 32-bit -> raw bytes, length-delimited -> bytes"""
    out, pos = [], 0
    while pos < len(buf):
        key, pos = _varint(buf, pos)
        field, wire = key >> 3, key & 7
        if wire == 0:
            v, pos = _varint(buf, pos)
        elif wire == 1:
            v, pos = buf[pos:pos + 8], pos + 8
        elif wire == 5:
            v, pos = buf[pos:pos + 4], pos + 4
        elif wire == 2:
            n, pos = _varint(buf, pos)
            v, pos = buf[pos:pos + n], pos + n
            assert len(v) == n, "length-delimited field runs past the message"
        else:
            raise AssertionError("wire type %d" % wire)
        out.append((field, wire, v))
    assert pos == len(buf)
    return out


def _doubles(raw):
    assert len(raw) % 8 == 0
    return list(struct.unpack("<%dd" % (len(raw) // 8), raw))


def decode_event(payload):
    """-> {"wall_time", "step", "file_version"?, "values": [{"tag", "simple_value_bits"?, "simple_value"?, "image"?, "histo"?}]}"""
    ev = {"step": 0, "values": []}
    for field, wire, v in fields(payload):
        if field == 1 and wire == 1:
            ev["wall_time"] = struct.unpack("<d", v)[0]
        elif field == 2 and wire == 0:
            ev["step"] = v
        elif field == 3 and wire == 2:
            ev["file_version"] = v.decode("utf-8")
        elif field == 5 and wire == 2:
            for f2, w2, value in fields(v):
                assert (f2, w2) == (1, 2), "Summary holds only `value` messages"
                item = {}
                for f3, w3, x in fields(value):
                    if f3 == 1 and w3 == 2:
                        item["tag"] = x.decode("utf-8")
                    elif f3 == 2 and w3 == 5:
                        item["simple_value_bits"] = struct.unpack("<I", x)[0]
                        item["simple_value"] = struct.unpack("<f", x)[0]
                    elif f3 == 4 and w3 == 2:
                        img = {}
                        for f4, w4, y in fields(x):
                            img[{1: "height", 2: "width", 3: "colorspace", 4: "encoded_image_string"}[f4]] = y
                        item["image"] = img
                    elif f3 == 5 and w3 == 2:
                        h = {}
                        for f4, w4, y in fields(x):
                            name = {1: "min", 2: "max", 3: "num", 4: "sum", 5: "sum_squares", 6: "bucket_limit", 7: "bucket"}[f4]
                            h[name] = _doubles(y) if f4 >= 6 else struct.unpack("<d", y)[0]
                        item["histo"] = h
                    else:
                        raise AssertionError("unexpected Summary.Value field %d (wire %d)" % (f3, w3))
                ev["values"].append(item)
        else:
            raise AssertionError("unexpected Event field %d (wire %d)" % (field, wire))
    return ev


def read_events(path):
    return [decode_event(p) for p in read_records(path)]


def by_tag(events):
    """{tag: [(step, value dict)]} in file order (the file_version record has no values)."""
    out = {}
    for ev in events:
        for v in ev["values"]:
            out.setdefault(v["tag"], []).append((ev["step"], v))
    return out
