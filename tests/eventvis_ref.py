"""numpy restatement of the reference's event_visualisation.plot_event_cnt (myutils/vis_events/matplotlib_plot_events.py:127-251)
for the 'blue_red' and 'green_red' schemes, written for the event-image tests (and timed by tools/opbench.py as the host path
the native op replaces).  It is held bit for bit against the reference's own outputs in tests/golden/eventvis_small.npz
(test_eventvis_host.py) and is then the oracle of the seed-generated GPU cases.

Unlike the reference it does not write into its input, computes the percentiles from ebfi_amd.eventvis.percentile_rank (the
rank law the library implements, itself held against np.percentile) and states the colour map per pixel class instead of as a
sequence of masked assignments."""
import numpy as np

from ebfi_amd.eventvis import percentile_rank

SCHEMES = ("blue_red", "green_red")
MODES = [(s, b, n) for s in SCHEMES for b in (True, False) for n in (True, False)]


def mode_key(name, scheme, black, norm):
    return "%s__%s__%s__%s" % (name, scheme, "black" if black else "white", "norm" if norm else "raw")


def lerp32(a, b, t):
    """numpy's _lerp on float32 scalars: every operation rounds to float32 once."""
    a, b, t = np.float32(a), np.float32(b), np.float32(t)
    d = np.float32(b - a)
    if t >= np.float32(0.5):
        return np.float32(b - np.float32(d * np.float32(np.float32(1) - t)))
    return np.float32(a + np.float32(d * t))


def percentile32(plane, q):
    """(lower neighbour, upper neighbour, value) of np.percentile(plane, q) for a float32 array, from a full sort."""
    s = np.sort(np.asarray(plane, dtype=np.float32).ravel())
    lo, hi, g = percentile_rank(s.size, q)
    with np.errstate(all="ignore"):
        return s[lo], s[hi], lerp32(s[lo], s[hi], g)


def plot_event_cnt_numpy(event_cnt, color_scheme="green_red", use_opencv=False, is_black_background=True, is_norm=True,
                         np_percentile=False):
    """np_percentile: take the four percentiles from np.percentile (a partition; what a host path would run, and what
    tools/opbench.py times) instead of the sort + rank law + lerp32 restatement."""
    assert color_scheme in SCHEMES
    ev = np.asarray(event_cnt, dtype=np.float32)
    pos, neg = ev[:, :, 0].copy(), ev[:, :, 1].copy()
    one, zero = np.float32(1), np.float32(0)
    with np.errstate(all="ignore"):
        if is_norm:
            pct = (lambda v, q: np.percentile(v, q)) if np_percentile else (lambda v, q: percentile32(v, q)[2])
            pos_min, pos_max = pct(pos, 1), pct(pos, 99)
            neg_min, neg_max = pct(neg, 1), pct(neg, 99)
            mx = pos_max if pos_max > neg_max else neg_max
            if pos_min != mx:
                pos = (pos - pos_min) / np.float32(mx - pos_min)
            if neg_min != mx:
                neg = (neg - neg_min) / np.float32(mx - neg_min)
        else:
            as_pos = (pos >= neg) & (pos != 0)
            as_neg = (pos < neg) & (neg != 0)
            pos = np.where(as_pos, one, np.where(as_neg, zero, pos))
            neg = np.where(as_pos, zero, np.where(as_neg, one, neg))
        assert pos.dtype == np.float32 and neg.dtype == np.float32
        pos, neg = np.clip(pos, 0, 1), np.clip(neg, 0, 1)
        mp, mn = pos > 0, neg > 0
        pc = 1 if color_scheme == "green_red" else 0      # canvas channel of the positive polarity; the negative one is 2
        H, W = pos.shape
        if is_black_background:
            canvas = np.zeros((H, W, 3), np.float64)
            canvas[:, :, pc] = np.where(mp, pos, zero)
            canvas[:, :, 2] = np.where(mn, neg, zero)
        else:
            canvas = np.ones((H, W, 3), np.float64)
            as_pos = (mp & (neg == 0)) | (mp & mn & (pos >= neg))
            as_neg = (mn & (pos == 0)) | (mp & mn & (pos < neg))
            inv_p, inv_n = (one - pos).astype(np.float32), (one - neg).astype(np.float32)     # `1 - x` in float32, then widened
            for ch in range(3):
                if ch != pc:
                    canvas[:, :, ch][as_pos] = inv_p[as_pos]
                if ch != 2:
                    canvas[:, :, ch][as_neg] = inv_n[as_neg]
        img = (canvas * 255).astype(np.uint8)
    return img if use_opencv else np.ascontiguousarray(img[:, :, ::-1])
