"""numpy float64 restatement of ebfi_segment_stats (include/ebfi_hip.h), written for the tests: per segment the moments
{finite count, non-finite count, min, max, sum, sum of squares} over the finite values and the histogram
    hist[i] = #{finite v : limit[i - 1] < v <= limit[i]},  bucket 0 from -inf, values above the last limit in the last bucket.
Every value is widened to float64 before anything is compared or added; the sums are numpy's pairwise ones (another order than the
kernel's, the same precision)."""
import numpy as np


def tf_default_limits():
    """TensorFlow's default histogram limits, restated: 1e-12 * 1.1^k below 1e20, mirrored, 0.0 between, DBL_MAX last."""
    pos = []
    v = 1e-12
    while v < 1e20:
        pos.append(v)
        v *= 1.1
    return np.array([-p for p in pos[::-1]] + [0.0] + pos + [np.finfo(np.float64).max], dtype=np.float64)


def segment_stats_ref(x, offsets, limits):
    """x float32 [n]; offsets S + 1 ints; limits float64 [nb] ascending -> (moments float64 [S, 6], hist int64 [S, nb])."""
    x = np.asarray(x, dtype=np.float32)
    limits = np.asarray(limits, dtype=np.float64)
    S = len(offsets) - 1
    moments = np.zeros((S, 6), dtype=np.float64)
    hist = np.zeros((S, limits.size), dtype=np.int64)
    for s in range(S):
        seg = x[int(offsets[s]):int(offsets[s + 1])].astype(np.float64)
        finite = np.isfinite(seg)
        v = seg[finite]
        moments[s, 0], moments[s, 1] = v.size, seg.size - v.size
        moments[s, 2] = v.min() if v.size else np.inf
        moments[s, 3] = v.max() if v.size else -np.inf
        moments[s, 4], moments[s, 5] = v.sum(), (v * v).sum()
        # first limit that is not below v: searchsorted 'left' returns the first index i with limit[i] >= v
        idx = np.minimum(np.searchsorted(limits, v, side="left"), limits.size - 1)
        hist[s] = np.bincount(idx, minlength=limits.size)
    return moments, hist


def sum_bounds(x, offsets):
    """Per segment the absolute error allowed to a float64 sum and a float64 sum of squares computed in another order: 4 ulp of
    float64 per 2^20 addends (rounded up to whole blocks), the ulp taken at the sum of the magnitudes -- what bounds every partial
    sum of either order."""
    x = np.asarray(x, dtype=np.float32)
    out = []
    for s in range(len(offsets) - 1):
        seg = x[int(offsets[s]):int(offsets[s + 1])].astype(np.float64)
        v = seg[np.isfinite(seg)]
        blocks = max(1, -(-v.size // (1 << 20)))
        out.append((4 * blocks * np.spacing(np.abs(v).sum()), 4 * blocks * np.spacing((v * v).sum())))
    return out
