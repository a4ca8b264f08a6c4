"""The law of an fp16 scale slot, restated in numpy float32 from its description (DESIGN.md section 4 "slot law"; the device
statement is csrc/scale_law.hpp, the host one ebfi_amd.f16scale.next_scale -- both are pinned against this file bit for bit, this
file calls neither).

A slot is 64 floats: [0] scale in use (a power of two), [1] floor, [32] running |max| of the values staged through it since the
last finish launch; the other 61 words are unused and must stay what they are.

  record   a writer kernel leaves |max|' = M when M, the largest |value| it staged, is above both the |max| already there and the
           floor -- compared on the float BITS, so every NaN pattern orders above +inf; otherwise the slot is left alone.
  finish   once per step, per slot:
             |max| == 0 (idle, or nothing above the floor)   scale kept, floor halved
             |max| NaN                                        scale kept, floor halved, flag
             |max| in (0, 3.0e38]                             scale = next_scale(|max|), floor = 7/8 |max|;
                                                              flag if |max| * scale-in-use > 60000
             |max| above 3.0e38 (+inf included)               scale kept, floor = 0, flag
           |max| is cleared in every case; the flag is or'ed into guard[0]; guard[1] is not touched.
  next_scale(|max|) = 2^min(2 - e, 120) with |max| = m * 2^e, m in [0.5, 1): |max| * scale in [2, 4) for |max| >= 2^-118.
"""
import os
import subprocess

import numpy as np

SLOT_STRIDE, SLOT_AMAX, SLOT_FLOOR = 64, 32, 1
TARGET_EXP, SCALE_EXP_MAX = 2, 120
AMAX_LIMIT = np.float32(3.0e38)
RANGE_LIMIT = np.float32(60000.0)
FLOOR_FACTOR = np.float32(0.875)

_HERE = os.path.dirname(os.path.abspath(__file__))
_PROGRAM = os.path.join(_HERE, "_ref", "scale_law_host")


def bits(x):
    """uint32 bit patterns of float32 values."""
    return np.ascontiguousarray(x, dtype=np.float32).view(np.uint32)


def from_bits(u):
    return np.ascontiguousarray(u, dtype=np.uint32).view(np.float32)


def _exponent(a):
    """e of a = m * 2^e, m in [0.5, 1), for positive finite float32 `a`, read off the bit pattern (no libm): a normal number
    carries e + 126 in its exponent field, a subnormal is mantissa * 2^-149 and its e the mantissa's bit length - 149."""
    u = bits(a).astype(np.int64)
    field, mant = (u >> 23) & 0xff, u & 0x7fffff
    length = np.floor(np.log2(np.maximum(mant, 1).astype(np.float64))).astype(np.int64) + 1     # exact: mant < 2^23
    return np.where(field > 0, field - 126, length - 149)


def _pow2(k):
    """2^k as float32 for -126 <= k <= 127, written as its bits."""
    k = np.asarray(k, dtype=np.int64)
    return from_bits(((k + 127) << 23).astype(np.uint32)).reshape(k.shape)


def next_scale(amax):
    """float32 array -> float32 array; 1 where amax is 0 or not finite (the host's first-use fallback)."""
    a = np.asarray(amax, dtype=np.float32)
    ok = (a > 0) & np.isfinite(a)
    k = np.minimum(TARGET_EXP - _exponent(np.where(ok, a, np.float32(1))), SCALE_EXP_MAX)
    return np.where(ok, _pow2(k), np.float32(1)).astype(np.float32)


def finish(slots, guard):
    """One finish launch over `slots` (float32, n * 64 words) and `guard` (two int32).  Returns new arrays (slots in the shape
    given, all 64 words of every slot) and leaves its arguments unchanged."""
    out = np.array(slots, dtype=np.float32, copy=True)
    v = out.reshape(-1, SLOT_STRIDE)
    g = np.array(guard, dtype=np.int32, copy=True)
    if v.shape[0] == 0:
        return out, g
    a, s, f = v[:, SLOT_AMAX].copy(), v[:, 0].copy(), v[:, SLOT_FLOOR].copy()
    with np.errstate(all="ignore"):
        idle = ~(a > 0)                         # 0 and NaN
        measured = (a > 0) & (a <= AMAX_LIMIT)
        beyond = (a > 0) & ~(a <= AMAX_LIMIT)
        flag = np.isnan(a) | beyond | ((a > 0) & ((a * s).astype(np.float32) > RANGE_LIMIT))
        v[:, 0] = np.where(measured, next_scale(np.where(measured, a, np.float32(1))), s)
        v[:, SLOT_FLOOR] = np.where(idle, (f * np.float32(0.5)).astype(np.float32),
                                    np.where(measured, (FLOOR_FACTOR * a).astype(np.float32), np.float32(0)))
    v[:, SLOT_AMAX] = 0
    if flag.any():
        g[0] |= 1
    return out, g


def record(slot, m_bits):
    """One writer kernel whose largest staged |value| has the bit pattern `m_bits` (non-negative float or NaN, sign bit clear),
    on one slot (64 float32 words).  Returns the new slot."""
    out = np.array(slot, dtype=np.float32, copy=True)
    m = np.uint32(m_bits)
    assert out.shape == (SLOT_STRIDE,) and m < 0x80000000
    nan_from = np.uint32(0x7f800001)
    cur, floor = bits(out[SLOT_AMAX:SLOT_AMAX + 1])[0], bits(out[SLOT_FLOOR:SLOT_FLOOR + 1])[0]
    if m >= nan_from:                           # a NaN always reaches the slot; the larger pattern stays
        new = max(cur, m)
    elif cur >= nan_from:                       # a NaN already there stays
        new = cur
    else:
        new = m if m > max(cur, floor) else cur
    out[SLOT_AMAX:SLOT_AMAX + 1] = from_bits(np.array([new], dtype=np.uint32))
    return out


def steps_until_remeasured(amax_before, amax_after):
    """A slot measured at `amax_before` whose tensor then stays at `amax_after`: the number of idle finish launches (floor
    halvings) after which a writer's report goes through again -- 0 if the first one already does.  By iteration of the law."""
    slots = np.zeros(SLOT_STRIDE, dtype=np.float32)
    slots[SLOT_AMAX] = amax_before
    slots, _ = finish(slots, np.zeros(2, np.int32))
    m = bits(np.array([amax_after], dtype=np.float32))[0]
    for idle_steps in range(400):
        if record(slots, m)[SLOT_AMAX] != 0:
            return idle_steps
        slots, _ = finish(slots, np.zeros(2, np.int32))
    raise AssertionError("the floor never fell below %r" % amax_after)


# ---------------------------------------------------------------------------------------------------------------------------
# csrc/scale_law.hpp compiled for the host (oracle/scale_law_host.cpp): the functions the kernels call
def host_program(force=False):
    if force or not os.path.exists(_PROGRAM):
        subprocess.check_call(["make", "-C", _HERE, "_ref/scale_law_host"] + (["-B"] if force else []), stdout=subprocess.DEVNULL)
    return _PROGRAM


def host_finish(a, s, floor, program=None):
    """finish_slot of csrc/scale_law.hpp on float32 arrays -> (scale', floor', flag) arrays."""
    a, s, floor = (bits(x).reshape(-1) for x in (a, s, floor))
    text = "".join("F %08x %08x %08x\n" % t for t in zip(a.tolist(), s.tolist(), floor.tolist()))
    res = subprocess.run([program or host_program()], input=text, capture_output=True, text=True, check=True)
    rows = [ln.split() for ln in res.stdout.splitlines()]
    assert len(rows) == len(a)
    return (from_bits(np.array([int(r[0], 16) for r in rows], dtype=np.uint32)),
            from_bits(np.array([int(r[1], 16) for r in rows], dtype=np.uint32)), np.array([int(r[2]) for r in rows], dtype=np.int32))


def host_should_report(m, amax_now, floor, program=None):
    m, amax_now, floor = (bits(x).reshape(-1) for x in (m, amax_now, floor))
    text = "".join("R %08x %08x %08x\n" % t for t in zip(m.tolist(), amax_now.tolist(), floor.tolist()))
    res = subprocess.run([program or host_program()], input=text, capture_output=True, text=True, check=True)
    return np.array([int(ln) for ln in res.stdout.split()], dtype=bool)


# ---------------------------------------------------------------------------------------------------------------------------
# The finish table both test files use
def _prev(x):
    return np.nextafter(np.float32(x), np.float32(0), dtype=np.float32)


def _next(x):
    return np.nextafter(np.float32(x), np.float32(np.inf), dtype=np.float32)


def clean_amax_values():
    """0, the smallest subnormal, 2^-126; 2^k and both neighbours for k = -126 .. 127; the clamp boundary; 3.0e38."""
    vals = [np.float32(0), from_bits(np.array([1], np.uint32))[0], np.float32(2.0 ** -126)]
    for k in range(-126, 128):
        p = np.float32(2.0 ** k)
        vals += [_prev(p), p, _next(p)]
    vals += [np.float32(2.0 ** -119), np.float32(2.0 ** -118), np.float32(2.0 ** -117), AMAX_LIMIT]
    return [v for v in vals if v <= AMAX_LIMIT]      # (the upper neighbour of 2^127 and beyond raise the flag: separate rows)


FINISH_ROWS = 600            # rows of one table launch: three workgroups of 256 threads, the last one partial
_TAIL = 8                    # rows at the end of every table that are placed by hand


def finish_tables(pattern_seed=11):
    """Clean finish launches as a list of (slots [600, 64] float32, guard [2] int32).  The |max| values of clean_amax_values()
    number 769, more than one launch of 600 rows holds, so they are dealt over TWO launches of 600 rows.  Every row has a scale
    in use between 2^-126 and 2^120 with |max| * scale <= 60000 (from the largest such power of two downwards), floors 0 /
    normal / subnormal in turn, and the 61 unused words filled with a bit pattern.  The last 8 rows of each launch: four idle
    slots (floor 0, normal, the smallest subnormal, 3 * 2^-149), three with |max| * scale == 60000 exactly, one at 3.0e38."""
    amax = clean_amax_values()
    body = FINISH_ROWS - _TAIL
    assert 2 * body >= len(amax)
    rng = np.random.RandomState(pattern_seed)
    sub = from_bits(np.array([1, 3, 0x7fffff], np.uint32))
    tables = []
    for part in range(2):
        slots = from_bits(rng.randint(0, 2 ** 32, size=(FINISH_ROWS, SLOT_STRIDE), dtype=np.uint64).astype(np.uint32)).copy()
        for i in range(body):
            a = amax[(part * body + i) % len(amax)]
            if a > 0:
                # a = m * 2^e: the largest power of two with a * s <= 60000 is 2^(16 - e) for m <= 60000 / 65536, else 2^(15 - e)
                e = int(_exponent(np.array([a], np.float32))[0])
                top = 16 - e if float(a) * 2.0 ** (16 - e) <= 60000.0 else 15 - e
                s = _pow2(max(-126, min(SCALE_EXP_MAX, top - (i % 20))))
            else:
                s = _pow2(-126 + (i * 41) % 247)
            slots[i, 0], slots[i, SLOT_AMAX] = s, a
            slots[i, SLOT_FLOOR] = (np.float32(0), np.float32(0.3) * _pow2(-100 + (i * 7) % 200), sub[i % 3])[i % 3]
        t = body
        for k, floor in enumerate((np.float32(0), np.float32(0.7), sub[0], sub[1])):        # idle: the floor halves, 2^-149 -> 0
            slots[t + k, 0], slots[t + k, SLOT_AMAX], slots[t + k, SLOT_FLOOR] = _pow2(-126 + 82 * k), np.float32(0), floor
        for k, j in enumerate((0, -100, 100)):       # 60000 = 1875 * 2^5: |max| = 1875 * 2^j under the scale 2^(5 - j)
            slots[t + 4 + k, 0], slots[t + 4 + k, SLOT_AMAX] = _pow2(5 - j), np.float32(1875.0) * _pow2(j)
        slots[t + 7, 0], slots[t + 7, SLOT_AMAX] = _pow2(-126), AMAX_LIMIT
        prod = slots[:, SLOT_AMAX].astype(np.float64) * slots[:, 0].astype(np.float64)
        assert (prod <= 60000.0).all() and (prod[t + 4:t + 7] == 60000.0).all()
        tables.append((slots, np.array([0, 7], dtype=np.int32)))
    return tables


def flagged_rows():
    """(name, |max|, scale in use) of the rows that must raise the flag."""
    return [("nan_quiet", from_bits(np.array([0x7fc00000], np.uint32))[0], np.float32(1)),
            ("nan_payload", from_bits(np.array([0x7f80beef], np.uint32))[0], np.float32(4)),
            ("inf", np.float32(np.inf), np.float32(1)),
            ("above_limit", _next(AMAX_LIMIT), np.float32(2.0 ** -126)),
            ("flt_max", np.finfo(np.float32).max, np.float32(2.0 ** -126)),
            ("above_60000", _next(np.float32(60000.0)), np.float32(1))]
