"""The device noise law of the clip loaders (csrc/eventaug.hip): crop, flips, event noise and hot pixels of AugmentData
(dataloader/h5dataset.py:368-463) on an event stack, drawn where the stack lives.

The loaders' default law (``clipdata.draw_noise``) repeats the reference's host draw bit for bit and costs its single-threaded
time.  This one has the same distribution and is a pure integer function of (seed, cell):

  generator  Philox4x32-10; key = the 64-bit seed as (low word, high word), counter = (g low, g high, stream, 0).  The noise
             field is stream 0 -- cell ``c`` of the contiguous output takes word ``c & 3`` of group ``c >> 2`` -- and the hot
             pixels are stream 1 -- pixel ``n`` takes words 0, 1, 2 of group ``n``.
  count      a draw's word ``u`` gives ``k = #{m >= 1 : u < T_m}`` with ``T_m = floor(2^32 f erfc(m / (std sqrt 2)))``
             (``noise_table``, float64 on the host): ``int(|N(0, std)|)`` on a fraction ``f`` of the draws, folded into one word.
  hot pixel  ``x = (u0 * w) >> 32``, ``y = (u1 * h) >> 32``, amplitude from ``u2`` through the table of ``f = 1``, added to every
             bin and polarity at (y, x); repeated positions accumulate.

No transcendental runs on the device, so tests/eventaug_ref.py restates both kernels in numpy to the bit.

Inputs must be GPU tensors; there is no CPU path.
"""
import ctypes
import math

import torch

from . import _native as N

TABLE_MAX = N.CONSTANTS["EBFI_NOISE_TABLE_MAX"]          # the table travels by value in the kernel arguments
_MASK64 = (1 << 64) - 1


def noise_table(std, fraction=1.0):
    """(T_1, T_2, ...) up to, not including, the first zero entry: ``T_m = floor(2^32 f erfc(m / (std sqrt 2)))`` with
    ``f = min(max(fraction, 0), 1)``.  Strictly decreasing; empty for fraction 0.  A ``std`` that is not a positive finite
    number, or one whose table needs more than TABLE_MAX entries (std above about 5), raises ValueError."""
    std, f = float(std), float(fraction)
    if not (math.isfinite(std) and std > 0.0):
        raise ValueError("noise_table: std must be a positive finite number, got %r" % (std,))
    if math.isnan(f):
        raise ValueError("noise_table: fraction is NaN")
    f = min(max(f, 0.0), 1.0)
    table, m = [], 1
    while True:
        t = int(math.floor(4294967296.0 * f * math.erfc(m / (std * math.sqrt(2.0)))))
        if t <= 0:
            return tuple(table)
        if len(table) == TABLE_MAX:
            raise ValueError("noise_table: std %r needs more than the cap of %d table entries (std up to about 5)" % (std, TABLE_MAX))
        table.append(min(t, 4294967295))
        m += 1


def _table_arg(table):
    table = tuple(int(t) for t in table)
    if len(table) > TABLE_MAX:
        raise ValueError("noise table of %d entries: the cap is %d" % (len(table), TABLE_MAX))
    if any(not 0 < t <= 4294967295 for t in table) or any(a <= b for a, b in zip(table, table[1:])):
        raise ValueError("noise table entries must be strictly decreasing 32-bit words above zero (noise_table makes them)")
    return ((ctypes.c_uint32 * len(table))(*table) if table else None), len(table)


@torch.no_grad()
def augment_events(stack, window, flip_h, flip_v, seed, table, out=None, cell_offset=0):
    """stack: float32 [TB, 2, H, W] on the GPU, any non-negative strides with adjacent columns -- the transposed view the
    binning returns is read in place.  window: (i, j, h, w) of the frame, or None for the whole frame.  Returns the contiguous
    float32 [TB, 2, h, w] stack ``stack[:, :, window].flip(...) + k`` with the noise counts ``k`` of ``table`` (``noise_table``;
    empty: no noise) under ``seed`` -- one launch.  out: a contiguous destination to fill (a load's slice of an item);
    cell_offset: the index of out's first cell in the item the noise field is drawn over (0 for a whole item)."""
    N.require_gpu(stack, out)
    if stack.dtype != torch.float32 or stack.dim() != 4 or stack.shape[1] != 2:
        raise ValueError("augment_events: expected float32 [TB, 2, H, W], got %s %r" % (stack.dtype, tuple(stack.shape)))
    if stack.stride(3) != 1:
        stack = stack.contiguous()
    TB, _, H0, W0 = (int(v) for v in stack.shape)
    i, j, h, w = (0, 0, H0, W0) if window is None else (int(v) for v in window)
    shape = (TB, 2, max(h, 0), max(w, 0))
    if out is None:
        out = torch.empty(shape, dtype=torch.float32, device=stack.device)
    elif out.dtype != torch.float32 or tuple(out.shape) != shape or not out.is_contiguous() or out.device != stack.device:
        raise ValueError("augment_events: out must be a contiguous float32 tensor of shape %r on %s" % (shape, stack.device))
    tab, n = _table_arg(table)
    s = stack.stride()
    with torch.cuda.device_of(stack):
        rc = N.lib().ebfi_event_augment(N.ptr(stack), (ctypes.c_int64 * 3)(s[0], s[1], s[2]), TB, H0, W0, i, j, h, w,
                                        int(bool(flip_h)), int(bool(flip_v)), int(seed) & _MASK64, tab, n, int(cell_offset),
                                        N.ptr(out), N.stream_ptr(stack.device))
    N.check(rc, "ebfi_event_augment")
    return out


def hot_pixel_count(fraction, h, w):
    """``int(fraction * h * w)`` of add_hot_pixels, on the augmented size."""
    return max(int(float(fraction) * int(h) * int(w)), 0)


@torch.no_grad()
def add_hot_pixels(stack, seed, std, fraction):
    """In place on a contiguous float32 [..., h, w] stack on the GPU: ``hot_pixel_count(fraction, h, w)`` hot pixels under
    ``seed``, each with an amplitude of ``int(|N(0, std)|)`` added to every leading plane at its (y, x).  Returns stack."""
    N.require_gpu(stack)
    if stack.dtype != torch.float32 or stack.dim() < 2 or not stack.is_contiguous():
        raise ValueError("add_hot_pixels: expected a contiguous float32 [..., h, w] stack, got %s %r" % (stack.dtype, tuple(stack.shape)))
    h, w = int(stack.shape[-2]), int(stack.shape[-1])
    tab, n = _table_arg(noise_table(std, 1.0))
    planes = stack.numel() // max(h * w, 1)
    with torch.cuda.device_of(stack):
        rc = N.lib().ebfi_event_hot_pixels(N.ptr(stack), planes, h, w, int(seed) & _MASK64, tab, n, hot_pixel_count(fraction, h, w),
                                           N.stream_ptr(stack.device))
    N.check(rc, "ebfi_event_hot_pixels")
    return stack
