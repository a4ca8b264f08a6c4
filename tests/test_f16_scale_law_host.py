"""The law of an fp16 scale slot (csrc/scale_law.hpp, ebfi_amd.f16scale.next_scale) against its numpy restatement
(oracle/scale_ref.py), bit for bit, without a GPU: the host calibration, the C++ the kernels call (compiled for the CPU by
oracle/Makefile), properties of the restatement itself, and the layout constants of the two sides."""
import math
import os
import re

import numpy as np
import torch

from oracle import scale_ref as R

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _binade_sweep():
    """2^k and its two float32 neighbours for k = -126 .. 126 (759 values)."""
    vals = []
    for k in range(-126, 127):
        p = np.float32(2.0 ** k)
        vals += [np.nextafter(p, np.float32(0), dtype=np.float32), p, np.nextafter(p, np.float32(np.inf), dtype=np.float32)]
    return np.array(vals, dtype=np.float32)


def test_next_scale_is_the_frexp_law_at_every_binade_and_on_random_values():
    from ebfi_amd import f16scale
    rng = np.random.RandomState(5)
    rand = R.from_bits(rng.randint(1, 0x7f800000, size=100000).astype(np.uint32))          # every positive finite float32
    special = np.array([0.0, np.inf, np.nan, 2.0 ** -149, 2.0 ** -127, 0.24999999, np.finfo(np.float32).max, 3.0e38], dtype=np.float32)
    for amax in (_binade_sweep(), rand, special):
        got = f16scale.next_scale(torch.from_numpy(amax.copy())).numpy()
        ref = R.next_scale(amax)
        bad = np.nonzero(R.bits(got) != R.bits(ref))[0]
        assert bad.size == 0, (bad.size, amax[bad[:5]], got[bad[:5]], ref[bad[:5]])
        fin = np.isfinite(amax) & (amax > 0)
        big = fin & (amax >= np.float32(2.0 ** -118))
        prod = amax[big].astype(np.float64) * got[big].astype(np.float64)
        assert ((prod >= 2.0) & (prod < 4.0)).all(), amax[big][(prod < 2.0) | (prod >= 4.0)][:5]
        assert (got[fin & ~big] == np.float32(2.0 ** 120)).all()
        assert (got[~fin] == 1.0).all()
    # shapes and 0-d tensors (calibrate hands over a 0-d maximum)
    assert f16scale.next_scale(torch.tensor(0.24999999)).item() == 16.0
    assert f16scale.next_scale(torch.full((2, 3), 3.0)).shape == (2, 3)


def _law_table():
    """(|max|, scale, floor) of every row of the GPU finish table, clean and flag-raising."""
    a, s, f = [], [], []
    for slots, _ in R.finish_tables():
        a.append(slots[:, R.SLOT_AMAX]); s.append(slots[:, 0]); f.append(slots[:, R.SLOT_FLOOR])
    for _, amax, scale in R.flagged_rows():
        a.append(np.array([amax], np.float32)); s.append(np.array([scale], np.float32)); f.append(np.array([0.5], np.float32))
    return np.concatenate(a), np.concatenate(s), np.concatenate(f)


def test_cpp_law_matches_the_restatement_on_the_finish_table():
    a, s, f = _law_table()
    hs, hf, hflag = R.host_finish(a, s, f)
    slots = np.zeros((len(a), R.SLOT_STRIDE), np.float32)
    slots[:, R.SLOT_AMAX], slots[:, 0], slots[:, R.SLOT_FLOOR] = a, s, f
    # (row by row for the flags: the array form or's them into one guard word per launch)
    flags = np.array([R.finish(slots[i], [0, 0])[1][0] for i in range(len(a))])
    out, _ = R.finish(slots, [0, 0])
    assert np.array_equal(R.bits(hs), R.bits(out[:, 0]))
    assert np.array_equal(R.bits(hf), R.bits(out[:, R.SLOT_FLOOR]))
    assert np.array_equal(hflag, flags) and flags.sum() == len(R.flagged_rows())
    # the clean rows cover what the table promises
    clean = a[:2 * R.FINISH_ROWS]
    assert set(R.bits(np.array(R.clean_amax_values(), np.float32)).tolist()) <= set(R.bits(clean).tolist())
    assert ((clean.astype(np.float64) * s[:2 * R.FINISH_ROWS]) == 60000.0).sum() >= 6
    assert s.min() == np.float32(2.0 ** -126) and s[:2 * R.FINISH_ROWS].max() == np.float32(2.0 ** 120)


def test_sanitized_cpp_law_runs_clean_over_the_table_and_every_exponent():
    """The same stand-alone program built with -fsanitize=undefined,address (oracle/Makefile scale_law_asan; any report aborts
    it): the whole finish table, then both functions over every float32 exponent field with four mantissas -- frexpf / ldexpf
    at the extremes are where undefined behaviour would sit.  Same bits as the plain build."""
    import subprocess
    subprocess.check_call(["make", "-C", os.path.join(ROOT, "oracle"), "scale_law_asan"], stdout=subprocess.DEVNULL)
    prog = os.path.join(ROOT, "oracle", "_ref", "scale_law_host_asan")
    a, s, f = _law_table()
    x = R.from_bits(np.array([(e << 23) | m for e in range(256) for m in (0, 1, 0x400000, 0x7fffff)], np.uint32))
    for aa, ss, ff in ((a, s, f), (x, np.ones_like(x), x[::-1].copy()), (x, x[::-1].copy(), np.zeros_like(x))):
        san, plain = R.host_finish(aa, ss, ff, program=prog), R.host_finish(aa, ss, ff)
        assert all(np.array_equal(R.bits(p) if p.dtype == np.float32 else p, R.bits(q) if q.dtype == np.float32 else q)
                   for p, q in zip(san, plain))
    assert np.array_equal(R.host_should_report(x, x[::-1].copy(), np.roll(x, 7), program=prog),
                          R.host_should_report(x, x[::-1].copy(), np.roll(x, 7)))


def test_cpp_report_predicate_matches_record():
    rng = np.random.RandomState(9)
    vals = np.concatenate([R.from_bits(rng.randint(0, 0x7f800000, size=300).astype(np.uint32)),
                           R.from_bits(np.array([0, 1, 0x7f800000, 0x7fc00000, 0x7f80beef, 0x3f800000], np.uint32)),
                           np.array([0.5, 1.0, 2.0, 3.0, np.nextafter(np.float32(3), np.float32(0))], np.float32)])
    m, cur, fl = (x.reshape(-1) for x in np.meshgrid(vals[-11:], vals[-11:], vals[-11:][~np.isnan(vals[-11:])], indexing="ij"))
    m = np.concatenate([m, vals[:300]]); cur = np.concatenate([cur, vals[100:300], vals[:100]]); fl = np.concatenate([fl, vals[200:300], vals[:200]])
    sends = R.host_should_report(m, cur, fl)
    for mi, ci, fi, sent in zip(m, cur, fl, sends):
        slot = np.zeros(R.SLOT_STRIDE, np.float32)
        slot[R.SLOT_AMAX], slot[R.SLOT_FLOOR] = ci, fi
        mb, cb = int(R.bits([mi])[0]), int(R.bits([ci])[0])
        after = int(R.bits(R.record(slot, mb)[R.SLOT_AMAX:R.SLOT_AMAX + 1])[0])
        # the wave sends an atomic max on the bits when the predicate holds; else the slot is left alone
        assert after == (max(cb, mb) if sent else cb), (mi, ci, fi, sent)


def test_finish_is_idempotent_on_an_idle_slot_apart_from_the_floor():
    slots, guard = R.finish_tables()[0]
    once, g1 = R.finish(slots, guard)
    twice, g2 = R.finish(once, g1)
    keep = np.ones(R.SLOT_STRIDE, bool)
    keep[R.SLOT_FLOOR] = False
    assert np.array_equal(R.bits(once[:, keep]), R.bits(twice[:, keep])) and np.array_equal(g1, g2)
    assert np.array_equal(R.bits(twice[:, R.SLOT_FLOOR]), R.bits((once[:, R.SLOT_FLOOR] * np.float32(0.5)).astype(np.float32)))
    assert np.array_equal(R.bits(slots), R.bits(R.finish_tables()[0][0]))          # the argument is left alone


def test_a_dropped_maximum_is_measured_again_after_the_predicted_number_of_idle_steps():
    """After a drop by r < 7/8 the floor 7/8 * 2^-t first falls BELOW r after ceil(log2(0.875 / r)) halvings (r values for
    which 0.875 / r is an exact power of two are left out: there the floor EQUALS the maximum once and one more step passes)."""
    rng = np.random.RandomState(3)
    ratios = [0.8, 0.5, 0.25, 0.3, 2.0 ** -12, 2.0 ** -30, 1e-9, 0.874] + list(rng.uniform(1e-6, 0.87, size=40))
    for before in (1.0, 3.0e-5, 7.7e20):
        for r in ratios:
            after = np.float32(np.float32(before) * np.float32(r))
            true_r = float(after) / float(np.float32(before))
            assert R.steps_until_remeasured(before, after) == math.ceil(math.log2(0.875 / true_r)), (before, r)
    assert R.steps_until_remeasured(1.0, 0.9) == 0          # within 1/8: reported at once
    assert R.steps_until_remeasured(1.0, 0.4375) == 2       # the floor equals the maximum after one halving: not above it


def test_python_and_cpp_agree_on_the_slot_layout():
    from ebfi_amd import f16scale
    csrc = os.path.join(ROOT, "ebfi-be_amd", "csrc")
    c16 = open(os.path.join(csrc, "c16.hpp")).read()
    assert '#include "scale_law.hpp"' in c16                 # (the target exponent lives in the header c16.hpp includes)
    text = c16 + open(os.path.join(csrc, "scale_law.hpp")).read()
    const = {k: int(v) for k, v in re.findall(r"\b(SLOT_STRIDE|SLOT_AMAX|SLOT_FLOOR|F16_TARGET_EXP|F16_SCALE_EXP_MAX)\s*=\s*(-?\d+)", text)}
    assert const == {"SLOT_STRIDE": f16scale.SLOT_STRIDE, "SLOT_AMAX": f16scale.SLOT_AMAX, "SLOT_FLOOR": f16scale.SLOT_FLOOR,
                     "F16_TARGET_EXP": f16scale.TARGET_EXP, "F16_SCALE_EXP_MAX": f16scale.SCALE_EXP_MAX}
    assert (R.SLOT_STRIDE, R.SLOT_AMAX, R.SLOT_FLOOR, R.TARGET_EXP, R.SCALE_EXP_MAX) == \
        (f16scale.SLOT_STRIDE, f16scale.SLOT_AMAX, f16scale.SLOT_FLOOR, f16scale.TARGET_EXP, f16scale.SCALE_EXP_MAX)
