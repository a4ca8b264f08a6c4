"""The reference's event-count images on the device (csrc/eventvis.hip).

``event_count_images``: float32 [n, 2, H, W] (polarity 0 positive, 1 negative; one image per time bin of ``SeqHREv[0]``) ->
interleaved uint8 [n, H, W, 3], bit-identical to ``event_visualisation().plot_event_cnt(ev[i].transpose(1, 2, 0), ...)`` of
myutils/vis_events/matplotlib_plot_events.py:127-251 for every finite input: the 1st / 99th percentile normalisation
(an exact radix select on the device, numpy's interpolation), the clip, the masks and the colour map, with the final
BGR -> RGB reversal folded into the store.  The stack is read where it lies (any image / polarity / row strides, unit column
stride); the picture leaves the device finished, three bytes per pixel.

Inputs must be GPU tensors; there is no CPU path.
"""
import ctypes

import numpy as np
import torch

from . import _native as N

COLOR_SCHEMES = {"blue_red": 0, "green_red": 1, "gray": 2}   # include/ebfi_hip.h EBFI_EVENT_*

_workspaces = {}


def percentile_rank(n, q):
    """(lower index, upper index, weight) of ``np.percentile(a, q)`` for a float32 array of n values (method 'linear'): numpy
    forms q / 100, the virtual index (n - 1) * q and its fractional part in the ARRAY's dtype, and reads the last element twice
    when the index reaches it.  The library computes the same in C (csrc/eventvis.hip percentile_rank); this restatement is
    what the host tests hold against np.percentile itself."""
    last = np.float32(n - 1)
    vi = last * (np.float32(q) / np.float32(100))
    if vi >= last:
        return n - 1, n - 1, np.float32(0)
    lo = int(np.floor(vi))
    return lo, lo + 1, np.float32(vi - np.float32(lo))


def _workspace(device, stream, shape):
    key = (device, stream, shape)
    ws = _workspaces.get(key)
    if ws is None:
        nbytes = N.lib().ebfi_event_cnt_image_workspace(*shape)
        ws = torch.empty(max(nbytes // 8, 1), dtype=torch.float64, device=device)   # (float64: 16-byte aligned storage)
        _workspaces[key] = ws
    return ws


@torch.no_grad()
def event_count_images(ev, color_scheme="blue_red", black_background=False, is_norm=True, use_opencv=False, out=None):
    """ev: float32 [n, 2, H, W] on the GPU, any strides with adjacent columns (a [TB, 2, H, W] slice of the event stack is read
    in place).  out: a contiguous uint8 [n, H, W, 3] tensor to fill; allocated otherwise.  Runs on the current stream."""
    N.require_gpu(ev, out)
    if color_scheme not in COLOR_SCHEMES:
        raise ValueError("event_count_images: Not support %s" % (color_scheme,))
    if ev.dtype != torch.float32 or ev.dim() != 4 or ev.shape[1] != 2:
        raise ValueError("event_count_images: expected float32 [n, 2, H, W], got %s %r" % (ev.dtype, tuple(ev.shape)))
    if ev.stride(3) != 1 and ev.shape[3] != 1:
        ev = ev.contiguous()
    n, _, H, W = (int(v) for v in ev.shape)
    if out is None:
        out = torch.empty((n, H, W, 3), dtype=torch.uint8, device=ev.device)
    elif out.dtype != torch.uint8 or tuple(out.shape) != (n, H, W, 3) or not out.is_contiguous() or out.device != ev.device:
        raise ValueError("event_count_images: out must be a contiguous uint8 tensor of shape %r on %s" % ((n, H, W, 3), ev.device))
    norm = int(bool(is_norm))
    if n == 0:
        return out
    with torch.cuda.device_of(ev):
        stream = N.stream_ptr(ev.device)
        ws = _workspace(ev.device, stream.value, (n, H, W, norm))
        strides = (ctypes.c_int64 * 3)(*[int(v) for v in ev.stride()[:3]])
        rc = N.lib().ebfi_event_cnt_image(N.ptr(ev), strides, n, H, W, COLOR_SCHEMES[color_scheme], int(bool(black_background)),
                                          norm, int(bool(use_opencv)), N.ptr(out), N.ptr(ws), ws.numel() * 8, stream)
    N.check(rc, "ebfi_event_cnt_image")
    return out
