"""numpy restatement of the device noise law of the clip loaders (include/ebfi_hip.h, ebfi_event_augment / ebfi_event_hot_pixels):
Philox4x32-10, the erfc table, the noise field and the hot pixels.  Everything after the table is integer arithmetic, so the
device kernels (test_gpu_eventaug.py) must agree with it to the bit; the generator is pinned to its published known answer and
the law's distribution to the closed form and to the reference's own draw in test_eventaug_host.py.  Written from the law's text,
independently of csrc/eventaug.hip: whole arrays at once, words picked by indexing, hot pixels accumulated one by one.
"""
import math

import numpy as np

M0, M1 = np.uint64(0xD2511F53), np.uint64(0xCD9E8D57)
W0, W1 = 0x9E3779B9, 0xBB67AE85
MASK32 = np.uint64(0xFFFFFFFF)
S32 = np.uint64(32)
TABLE_MAX = 32


def philox4x32_10(counter, key):
    """counter: four arrays (or scalars) of 32-bit words, key: two 32-bit integers -> uint64 array [..., 4] of 32-bit words."""
    c = [np.asarray(v, dtype=np.uint64) & MASK32 for v in counter]
    c = list(np.broadcast_arrays(*c))
    k0, k1 = int(key[0]) & 0xFFFFFFFF, int(key[1]) & 0xFFFFFFFF
    for _ in range(10):
        p0, p1 = M0 * c[0], M1 * c[2]                      # 32 x 32 -> 64 bits: no overflow in uint64
        c = [(p1 >> S32) ^ c[1] ^ np.uint64(k0), p1 & MASK32, (p0 >> S32) ^ c[3] ^ np.uint64(k1), p0 & MASK32]
        k0, k1 = (k0 + W0) & 0xFFFFFFFF, (k1 + W1) & 0xFFFFFFFF
    return np.stack(c, axis=-1)


def words(groups, stream, seed):
    """The four words of each Philox group of `stream` under the 64-bit `seed` -> uint64 [len(groups), 4]."""
    g = np.asarray(groups, dtype=np.uint64)
    seed = int(seed) & ((1 << 64) - 1)
    return philox4x32_10((g & MASK32, g >> S32, np.uint64(stream), np.uint64(0)), (seed & 0xFFFFFFFF, seed >> 32))


def table(std, fraction=1.0):
    """T_m = floor(2^32 f erfc(m / (std sqrt 2))), m = 1, 2, ... up to the first zero entry (not included)."""
    f = min(max(float(fraction), 0.0), 1.0)
    out, m = [], 1
    while True:
        t = math.floor(2.0 ** 32 * f * math.erfc(m / (float(std) * math.sqrt(2.0))))
        if t <= 0:
            return out
        out.append(int(t))
        m += 1


def counts(u, tab):
    """k = #{m : u < T_m} of every word of `u` -> int64 array of u's shape."""
    u = np.asarray(u, dtype=np.uint64)
    k = np.zeros(u.shape, dtype=np.int64)
    for t in tab:
        k += u < np.uint64(t)
    return k


def noise_field(shape, seed, tab, first_cell=0):
    """The noise counts of a contiguous stack of `shape` whose first cell is cell `first_cell` of the item: cell c takes word
    c & 3 of group c >> 2 of stream 0 -> int64 array of `shape`."""
    n = int(np.prod(shape))
    cells = np.arange(first_cell, first_cell + n, dtype=np.uint64)
    g0 = int(first_cell) >> 2
    w = words(np.arange(g0, ((first_cell + n + 3) >> 2) + 1, dtype=np.uint64), 0, seed)
    u = w[(cells >> np.uint64(2)).astype(np.int64) - g0, (cells & np.uint64(3)).astype(np.int64)]
    return counts(u, tab).reshape(shape)


def hot_pixel_count(fraction, h, w):
    return max(int(fraction * h * w), 0)


def hot_pixels(h, w, seed, std, fraction):
    """The [h, w] int64 image every plane of the stack gains: pixel n takes words 0, 1, 2 of group n of stream 1."""
    img = np.zeros((h, w), dtype=np.int64)
    n = hot_pixel_count(fraction, h, w)
    if n == 0:
        return img
    u = words(np.arange(n, dtype=np.uint64), 1, seed)
    amp = counts(u[:, 2], table(std, 1.0))
    for k in range(n):
        x, y = (int(u[k, 0]) * w) >> 32, (int(u[k, 1]) * h) >> 32
        img[y, x] += int(amp[k])
    return img


def augment(src, window, flip_h, flip_v, seed, tab, first_cell=0):
    """src: float32 array [TB, 2, H, W] (any view) -> the contiguous float32 [TB, 2, h, w] stack of ebfi_event_augment."""
    i, j, h, w = (0, 0) + src.shape[2:] if window is None else window
    v = src[:, :, i:i + h, j:j + w]
    v = v[..., ::-1] if flip_h else v
    v = v[..., ::-1, :] if flip_v else v
    out = np.ascontiguousarray(v, dtype=np.float32)
    if len(tab):
        out = out + noise_field(out.shape, seed, tab, first_cell).astype(np.float32)
    return out


def class_probabilities(std, fraction):
    """P(k = 0), P(k = 1), P(k = 2), P(k = 3), P(k >= 4) of int(|N(0, std)|) on a `fraction` of the cells, closed form."""
    f = min(max(float(fraction), 0.0), 1.0)
    tail = [f * math.erfc(m / (std * math.sqrt(2.0))) for m in range(1, 5)]
    return [1.0 - tail[0], tail[0] - tail[1], tail[1] - tail[2], tail[2] - tail[3], tail[3]]
