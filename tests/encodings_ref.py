"""Numpy restatement of the laws of dataloader/encodings.py that ebfi_amd.encodings implements (csrc/encodings.hip).

Serial and fp32 throughout: a pixel receives its addends in event-list order (``np.add.at`` is unbuffered and walks the index
list front to back; ``serial_sum`` below is the same thing as a plain loop and the host tests hold the two against each other),
every product and sum is a float32 operation, nothing is fused.  Independent of torch's scatter.  The reference edits its
inputs in place; these functions never do -- they state what the edits do to the OUTPUT, function by function:

  rule 1  voxel grids with temporal weights: the weights are a fresh tensor per bin, the coordinates are the caller's, so an
          out-of-range event adds nothing in bin 0 and its full weight at pixel (0,0) in every later bin;
  rule 2  naive voxel / stack without polarity: ps[beg:end] is a view, the first bin zeroes it for good: such an event adds 0;
  rule 3  channels: the positive pass drops the event and moves it, the negative pass counts it at (0,0);
  rule 4  mask: accumulate=False, the last event of a pixel wins; an out-of-range last writer stores 0 at (0,0).

tests/test_encodings_host.py checks every function here against what the reference itself returned
(tests/golden/encodings_small.npz), bit for bit.
"""
import numpy as np

F = np.float32


def in_range(xs, ys, H, W):
    return (xs >= 0) & (xs < W) & (ys >= 0) & (ys < H)


def pixel(xs, ys, H, W):
    """(in-range mask, row, column) with out-of-range events at (0,0); .long() truncates."""
    ok = in_range(xs, ys, H, W)
    ix = np.where(ok, xs, 0).astype(np.int64)
    iy = np.where(ok, ys, 0).astype(np.int64)
    return ok, iy, ix


def scatter(shape, iy, ix, w):
    img = np.zeros(shape, F)
    np.add.at(img, (iy, ix), np.asarray(w, F))
    return img


def serial_sum(shape, iy, ix, w, reverse=False):
    """The same sum as a plain loop; reverse=True feeds every pixel its addends in the opposite order."""
    img = np.zeros(shape, F)
    order = range(len(w) - 1, -1, -1) if reverse else range(len(w))
    for k in order:
        img[iy[k], ix[k]] = F(img[iy[k], ix[k]] + F(w[k]))
    return img


def events_to_image(xs, ys, ps, sensor_size):
    H, W = sensor_size
    ok, iy, ix = pixel(xs, ys, H, W)
    return scatter((H, W), iy, ix, np.where(ok, ps, F(0)))


def bsearch(t, l, r, x, side="left"):
    while l <= r:
        if t[l] == x:
            return l
        if t[r] == x:
            return r
        mid = l + (r - l) // 2
        if t[mid] == x:
            return mid
        elif t[mid] < x:
            l = mid + 1
        else:
            r = mid - 1
    return l if side == "left" else r


def skip(ts):
    return len(ts) <= 3 or ts.sum() == 0


def time_span(ts):
    return F(F(ts[-1] - ts[0]) + F(1e-6))


def naive_bounds(ts, B):
    dt = time_span(ts)
    delta_t = F(dt / F(B))
    out = []
    for bi in range(B):
        tstart = F(ts[0] + F(delta_t * F(bi)))
        tend = F(tstart + delta_t)
        out.append((bsearch(ts, 0, len(ts) - 1, tstart), bsearch(ts, 0, len(ts) - 1, tend, "right") + 1))
    return out


def temporal_weights(tn, bi):
    return np.maximum(F(0), F(1) - np.abs(tn - F(bi))).astype(F)


def _temporal_voxel(xs, ys, tn, ps, B, H, W):
    ok, iy, ix = pixel(xs, ys, H, W)
    bins = []
    for bi in range(B):
        w = (ps * temporal_weights(tn, bi)).astype(F)
        if bi == 0:
            w = np.where(ok, w, F(0))                                     # rule 1
        bins.append(scatter((H, W), iy, ix, w))
    return np.stack(bins)


def voxel_addends(xs, ys, ts, ps, B, sensor_size):
    """(iy, ix, [weights per bin]) of the temporal-bilinear voxel grid: what the discriminating-case check permutes."""
    H, W = sensor_size
    ok, iy, ix = pixel(xs, ys, H, W)
    tn = ((ts - ts[0]) / time_span(ts) * F(B - 1)).astype(F)
    ws = [(ps * temporal_weights(tn, bi)).astype(F) for bi in range(B)]
    ws[0] = np.where(ok, ws[0], F(0))
    return iy, ix, ws


def events_to_voxel_torch(xs, ys, ts, ps, B, sensor_size, temporal_bilinear=True):
    H, W = sensor_size
    if skip(ts):
        return np.zeros((B, H, W), F)
    if temporal_bilinear:
        tn = ((ts - ts[0]) / time_span(ts) * F(B - 1)).astype(F)
        return _temporal_voxel(xs, ys, tn, ps, B, H, W)
    return events_to_stack_no_polarity(xs, ys, ts, ps, B, sensor_size)


def events_to_voxel(xs, ys, ts, ps, num_bins, sensor_size):
    H, W = sensor_size
    return _temporal_voxel(xs, ys, (ts * F(num_bins - 1)).astype(F), ps, num_bins, H, W)


def events_to_stack_no_polarity(xs, ys, ts, ps, B, sensor_size):
    H, W = sensor_size
    if skip(ts):
        return np.zeros((B, H, W), F)
    ok, iy, ix = pixel(xs, ys, H, W)
    w = np.where(ok, ps, F(0))                                            # rule 2
    return np.stack([scatter((H, W), iy[b:e], ix[b:e], w[b:e]) for b, e in naive_bounds(ts, B)])


def events_to_channels(xs, ys, ps, sensor_size):
    H, W = sensor_size
    ok, iy, ix = pixel(xs, ys, H, W)
    pos = (ps * np.where(ps < 0, F(0), ps)).astype(F)
    neg = (ps * np.where(ps > 0, F(0), ps)).astype(F)
    return np.stack([scatter((H, W), iy, ix, np.where(ok, pos, F(0))), scatter((H, W), iy, ix, neg)])      # rule 3


def events_to_mask(xs, ys, ps, sensor_size):
    H, W = sensor_size
    ok, iy, ix = pixel(xs, ys, H, W)
    w = np.abs(np.where(ok, ps, F(0))).astype(F)
    img = np.zeros((H, W), F)
    for k in range(len(w)):                                               # rule 4
        img[iy[k], ix[k]] = w[k]
    return img


def interpolate_to_image(pxs, pys, dxs, dys, weights, img):
    """Returns the new image (the reference works in place).  Four passes in turn; an event whose footprint leaves the image is
    skipped (the reference raises there)."""
    img = np.array(img, F)
    H, W = img.shape
    keep = (pxs >= 0) & (pxs <= W - 2) & (pys >= 0) & (pys <= H - 2)
    px, py, dx, dy, w = (np.asarray(a)[keep] for a in (pxs, pys, dxs, dys, weights))
    one = F(1)
    np.add.at(img, (py, px), (w * (one - dx) * (one - dy)).astype(F))
    np.add.at(img, (py, px + 1), (w * dx * (one - dy)).astype(F))
    np.add.at(img, (py + 1, px), (w * (one - dx) * dy).astype(F))
    np.add.at(img, (py + 1, px + 1), (w * dx * dy).astype(F))
    return img


def bilinear_operands(xs, ys, ps, sensor_size, clip_out_of_range=True, padding=True):
    H, W = sensor_size
    ok = in_range(xs, ys, H, W)
    x, y, p = (np.where(ok, a, F(0)).astype(F) for a in (xs, ys, ps))
    oH, oW = (H + 1, W + 1) if padding else (H, W)
    mask = np.ones(len(x), F)
    if clip_out_of_range:
        mask = (np.where(x >= oW - 1, F(0), F(1)) * np.where(y >= oH - 1, F(0), F(1))).astype(F)
    fx, fy = np.floor(x), np.floor(y)
    return (fx * mask).astype(np.int64), (fy * mask).astype(np.int64), (x - fx).astype(F), (y - fy).astype(F), \
        (p * mask).astype(F), (oH, oW)


def events_to_image_torch(xs, ys, ps, sensor_size, clip_out_of_range=True, interpolation=None, padding=True):
    H, W = sensor_size
    integer = np.issubdtype(np.asarray(xs).dtype, np.integer)
    if interpolation == "bilinear" and not integer:
        if not padding and not clip_out_of_range:
            raise ValueError("padding=False needs clip_out_of_range=True")
        px, py, dx, dy, w, shape = bilinear_operands(xs, ys, ps, sensor_size, clip_out_of_range, padding)
        return interpolate_to_image(px, py, dx, dy, w, np.zeros(shape, F))
    img = events_to_image(xs, ys, ps, sensor_size)
    if interpolation == "bilinear" and padding:
        out = np.zeros((H + 1, W + 1), F)
        out[:H, :W] = img
        return out
    return img


def events_polarity_mask(ps):
    return np.stack([np.where(ps < 0, F(0), ps), np.where(ps > 0, F(0), ps) * F(-1)], 1).astype(F)


def get_hot_event_mask(event_rate, idx, max_px=100, min_obvs=5, max_rate=0.8):
    """Returns (mask, edited event_rate)."""
    rate = np.array(event_rate, F)
    mask = np.ones(rate.shape, F)
    if idx > min_obvs:
        flat = rate.reshape(-1)
        for _ in range(max_px):
            nan = np.flatnonzero(np.isnan(flat))
            k = int(nan[0]) if nan.size else int(np.argmax(flat))         # the first index of the maximum; a NaN is the maximum
            if flat[k] > F(max_rate):
                flat[k] = 0
                mask.reshape(-1)[k] = 0
            else:
                break
    return mask, rate


def stack2cnt(stack):
    r = np.rint(np.asarray(stack, F))
    pos = np.where(r < 0, F(0), r).astype(F)
    neg = (np.where(r > 0, F(0), r) * F(-1)).astype(F)
    B, TB = r.shape[:2]
    out = np.zeros((B, 2) + r.shape[2:], F)
    for t in range(TB):                                                   # bin order
        out[:, 0] = out[:, 0] + pos[:, t]
        out[:, 1] = out[:, 1] + neg[:, t]
    return out
