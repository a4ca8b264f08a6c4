"""numpy restatement of what ebfi_grad_norm and the moving average of ebfi_optim_step_ex compute (csrc/gradnorm.hip,
csrc/optim.hip; include/ebfi_hip.h states the laws), written for the tests:

  total_norm     the float64 norm of a float32 gradient: sqrt(sum g^2) or max |g|; a NaN anywhere gives NaN
  clip_coef      torch.nn.utils.clip_grad_norm_'s coefficient in float32: c = max_norm / (norm + 1e-6), then min(c, 1) with a
                 NaN kept
  ema_decay_at   the decay of the t-th applied average: decay, or min(decay, (1 + t) / (10 + t)) with warm-up (float64)
  ema_update     e + w (p - e) in float32, one rounding per operation, w = float32(1 - d)
  EmaRef         the buffer, its count and the skipped-step rule: a skipped step changes neither
"""
import numpy as np

L2, INF = 2, float("inf")


def total_norm(g, norm_type=L2):
    """float64.  `g`: float32 array.  Squares and sums in float64 (numpy's pairwise sum: 6e6 terms err by far less than 2^-53
    times their count, which the tests' one-ulp-of-float32 allowance dwarfs)."""
    g = np.asarray(g, dtype=np.float32).astype(np.float64).reshape(-1)
    if g.size == 0:
        return np.float64(0.0)
    if norm_type == L2:
        with np.errstate(over="ignore", invalid="ignore"):
            return np.sqrt(np.sum(g * g))
    if norm_type == INF:
        a = np.abs(g)
        return np.float64(np.nan) if np.isnan(a).any() else a.max()
    raise ValueError("norm_type must be 2 or inf")


def norm_candidates(norm64):
    """float32(norm64) and its two float32 neighbours: what a correctly accumulated float64 sum may round to."""
    with np.errstate(over="ignore"):
        x = np.float32(norm64)
    if not np.isfinite(x):
        return [x]
    return [np.nextafter(x, np.float32(-np.inf)), x, np.nextafter(x, np.float32(np.inf))]


def clip_coef(norm32, max_norm):
    """float32, from the float32 norm: every operation rounds to float32 once."""
    norm32, max_norm = np.float32(norm32), np.float32(max_norm)
    with np.errstate(over="ignore", invalid="ignore", divide="ignore"):
        c = np.float32(max_norm / np.float32(norm32 + np.float32(1e-6)))
    return np.float32(1.0) if c > np.float32(1.0) else c


def ema_decay_at(decay, warmup, t):
    decay, t = float(decay), float(t)
    return min(decay, (1.0 + t) / (10.0 + t)) if warmup else decay


def ema_update(e, p, decay, warmup, t):
    """The t-th applied average (t counts from 1) of float32 arrays e, p -> new e (float32)."""
    w = np.float32(1.0 - ema_decay_at(decay, warmup, t))
    e, p = np.asarray(e, dtype=np.float32), np.asarray(p, dtype=np.float32)
    with np.errstate(over="ignore", invalid="ignore"):
        d = (p - e).astype(np.float32)
        return (e + (w * d).astype(np.float32)).astype(np.float32)


class EmaRef:
    def __init__(self, p0, decay, warmup):
        self.e = np.array(p0, dtype=np.float32, copy=True)
        self.decay, self.warmup, self.step = float(decay), bool(warmup), 0

    def update(self, p_new, skipped=False):
        """`p_new`: the parameters after the step.  A skipped step leaves buffer and count alone."""
        if not skipped:
            self.step += 1
            self.e = ema_update(self.e, p_new, self.decay, self.warmup, self.step)
        return self.e
