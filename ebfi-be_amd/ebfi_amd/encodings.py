"""dataloader/encodings.py on the device: every public function of the reference module, with its signature.

``events_to_stack(xs, ys, ts, ps, B, sensor_size)`` (reference :307-350) keeps the reference's signature and returns the
same ``[2, B, H, W]`` float32 stack (index 0 positive, 1 negative; callers transpose to
``[B, 2, H, W]`` as h5dataset.py:349 does), bit-exact including the reference's shared-bin-edge
and out-of-range-event behaviour (csrc/events.hip).  Differences: inputs must be GPU tensors and
the result stays on the GPU; the caller's xs/ys are NOT zeroed in place (the reference mutates
them as a side effect of events_to_image).

The other functions (csrc/encodings.hip) add fractional float32 weights, where the order of addition is part of the result.
Their law is the reference run with one thread: every pixel receives its addends in event-list order, fp32, unfused.  The
library builds a stable sort of the events by pixel once per call and lets one thread per (pixel, plane) add in that order;
the result is bit-identical from run to run and to the serial reference.  What the reference's in-place zeroing of
out-of-range events does to its own later passes is reproduced in the output (include/ebfi_hip.h lists the four rules); the
caller's tensors are never modified -- except ``event_rate`` in ``get_hot_event_mask``, whose purpose that is.

float32 only, as the reference is in effect (with float64 stamps its index_put_ raises "source and destination dtypes
match"): ``xs``, ``ys`` float32 or an integer type where the reference takes ``long``; ``ts``, ``ps`` float32.  Inputs are
GPU tensors, results stay on the GPU (``stack2cnt`` included: the reference's ``.cpu()`` is the one documented difference),
and a ``device=`` other than the tensors' own is refused.  No call synchronises or reads a value back; all are capturable.
"""
import torch

from . import _native as N

__all__ = ["interpolate_to_image", "events_to_image_torch", "binary_search_torch_tensor", "events_to_voxel_torch",
           "events_to_stack_polarity", "events_to_stack_no_polarity", "events_to_image", "events_to_voxel",
           "events_to_channels", "events_to_stack", "events_to_mask", "events_polarity_mask", "get_hot_event_mask",
           "stack2cnt"]

_INTEGER = (torch.int64, torch.int32, torch.int16, torch.int8, torch.uint8)


@torch.no_grad()
def events_to_stack(xs, ys, ts, ps, B, sensor_size=(180, 240)):
    N.require_gpu(xs, ys, ts, ps)
    assert len(xs) == len(ys) and len(ys) == len(ts) and len(ts) == len(ps)
    H, W = int(sensor_size[0]), int(sensor_size[1])
    dev = ts.device
    xs, ys, ts = (t.to(torch.float64).contiguous() for t in (xs, ys, ts))
    ps = ps.to(torch.float32).contiguous()
    out = torch.empty((2, int(B), H, W), dtype=torch.float32, device=dev)
    lib = N.lib()
    need = int(lib.ebfi_events_workspace(int(B)))
    ws = torch.empty(max(need, 8), dtype=torch.uint8, device=dev)
    with torch.cuda.device_of(ts):
        rc = lib.ebfi_events_to_stack(N.ptr(xs), N.ptr(ys), N.ptr(ts), N.ptr(ps), int(len(ts)), int(B), H, W,
                                      N.ptr(out), N.ptr(ws), need, N.stream_ptr(dev))
    N.check(rc, "ebfi_events_to_stack")
    return out


# ------------------------------------------------------------------ argument plumbing
def _mode(name):
    return N.CONSTANTS["EBFI_GRID_" + name]


def _f32(what, **tensors):
    """Contiguous float32 views of the float arguments; anything else is refused, as the reference in effect refuses it."""
    out = []
    for name, t in tensors.items():
        if t.dtype != torch.float32:
            raise TypeError("%s: %s is %s; the encodings take float32 event tensors (the reference's index_put_ refuses a "
                            "float64 source for its float32 image), convert with .float()" % (what, name, t.dtype))
        if t.dim() != 1:
            raise ValueError("%s: %s must be one-dimensional, got %r" % (what, name, tuple(t.shape)))
        out.append(t.contiguous())
    return out


def _coords(what, xs, ys):
    """float32 coordinates for the kernels: float32 as given, an integer type converted (exact below 2^24; beyond that the
    event is out of range for any sensor the library accepts either way)."""
    out = []
    for name, t in (("xs", xs), ("ys", ys)):
        if t.dtype in _INTEGER:
            t = t.to(torch.float32)
        out.append(t)
    return _f32(what, xs=out[0], ys=out[1])


def _device(what, device, t):
    if device is not None and torch.device(device) != t.device and not (
            torch.device(device).type == t.device.type and torch.device(device).index is None):
        raise ValueError("%s: device=%s, but the events are on %s; the result is built where the events are" % (what, device, t.device))
    return t.device


def _same_device(what, *tensors):
    """One device for every tensor of a call: the kernels dereference all of them on the device of the launch."""
    devices = {t.device for t in tensors if t is not None}
    if len(devices) > 1:
        raise ValueError("%s: tensors on different devices %s" % (what, sorted(str(d) for d in devices)))


def _same_length(what, *tensors):
    if len({len(t) for t in tensors}) != 1:
        raise AssertionError("%s: event tensors of different lengths %r" % (what, [len(t) for t in tensors]))


def _grid(what, mode, xs, ys, ts, ps, planes, sensor_size, out_shape):
    H, W = int(sensor_size[0]), int(sensor_size[1])
    N.require_gpu(xs, ys, ts, ps)              # (after the dtype checks: a float64 list is refused as such on any device)
    _same_device(what, xs, ys, ts, ps)
    n = int(len(ps))
    dev = ps.device
    lib = N.lib()
    need = int(lib.ebfi_events_grid_workspace(n, int(planes), H, W))
    ws = torch.empty(max(need, 16), dtype=torch.uint8, device=dev)
    out = torch.empty(out_shape, dtype=torch.float32, device=dev)
    with torch.cuda.device_of(ps):
        rc = lib.ebfi_events_to_grid(N.ptr(xs), N.ptr(ys), N.ptr(ts), N.ptr(ps), n, _mode(mode), int(planes), H, W, N.ptr(out),
                                     N.ptr(ws), need, N.stream_ptr(dev))
    N.check(rc, "ebfi_events_to_grid (%s)" % what)
    return out


# ------------------------------------------------------------------ images
@torch.no_grad()
def events_to_image(xs, ys, ps, sensor_size=(180, 240)):
    """Accumulate events into an image, nearest pixel: img[y, x] += p in event order (reference :243-268)."""
    _same_length("events_to_image", xs, ys, ps)
    xs, ys = _coords("events_to_image", xs, ys)
    ps, = _f32("events_to_image", ps=ps)
    H, W = int(sensor_size[0]), int(sensor_size[1])
    return _grid("events_to_image", "IMAGE", xs, ys, None, ps, 1, sensor_size, (H, W))


@torch.no_grad()
def interpolate_to_image(pxs, pys, dxs, dys, weights, img):
    """Accumulate onto ``img`` in place with bilinear weights (reference :8-15): four passes in turn, each in event order.
    An event whose 2 x 2 footprint leaves the image is skipped (the reference raises IndexError)."""
    what = "interpolate_to_image"
    _same_length(what, pxs, pys, dxs, dys, weights)
    for name, t in (("pxs", pxs), ("pys", pys)):
        if t.dtype not in _INTEGER:
            raise TypeError("%s: %s is %s; base pixels are integer tensors" % (what, name, t.dtype))
    dxs, dys, weights = _f32(what, dxs=dxs, dys=dys, weights=weights)
    if img.dtype != torch.float32 or img.dim() != 2:
        raise TypeError("%s: img must be a two-dimensional float32 tensor, got %s %r" % (what, img.dtype, tuple(img.shape)))
    N.require_gpu(pxs, pys, dxs, dys, weights, img)
    _same_device(what, pxs, pys, dxs, dys, weights, img)
    pxs, pys = pxs.to(torch.int64).contiguous(), pys.to(torch.int64).contiguous()
    work = img if img.is_contiguous() else img.contiguous()
    H, W = int(img.shape[0]), int(img.shape[1])
    n = int(len(weights))
    lib = N.lib()
    need = int(lib.ebfi_events_grid_workspace(n, 1, H, W))
    ws = torch.empty(max(need, 16), dtype=torch.uint8, device=img.device)
    with torch.cuda.device_of(img):
        rc = lib.ebfi_interpolate_to_image(N.ptr(pxs), N.ptr(pys), N.ptr(dxs), N.ptr(dys), N.ptr(weights), n, H, W, N.ptr(work),
                                           N.ptr(ws), need, N.stream_ptr(img.device))
    N.check(rc, "ebfi_interpolate_to_image")
    if work is not img:
        img.copy_(work)


@torch.no_grad()
def events_to_image_torch(xs, ys, ps, device=None, sensor_size=(180, 240), clip_out_of_range=True, interpolation=None,
                          padding=True):
    """Event tensor to image, nearest or bilinear (reference :18-74).  Integer coordinates take the nearest branch whatever
    ``interpolation`` says, as in the reference; ``interpolation='bilinear'`` with ``padding`` returns ``[H+1, W+1]``."""
    what = "events_to_image_torch"
    _device(what, device, xs)
    _same_length(what, xs, ys, ps)
    if interpolation not in (None, "bilinear"):
        raise ValueError("%s: interpolation must be None or 'bilinear', got %r" % (what, interpolation))
    H, W = int(sensor_size[0]), int(sensor_size[1])
    integer = xs.dtype in _INTEGER
    bilinear = interpolation == "bilinear" and not integer
    if bilinear and not padding and not clip_out_of_range:
        raise ValueError("%s: interpolation='bilinear' with padding=False and clip_out_of_range=False writes past the image "
                         "for any event in the last row or column (the reference raises IndexError there); pass "
                         "padding=True or clip_out_of_range=True" % what)
    if ps.dim() > 1:
        ps = ps.squeeze()
    xs, ys = _coords(what, xs, ys)
    ps, = _f32(what, ps=ps)
    if bilinear:
        if padding:
            return _grid(what, "BILINEAR_PADDED", xs, ys, None, ps, 1, sensor_size, (H + 1, W + 1))
        return _grid(what, "BILINEAR_CLIPPED", xs, ys, None, ps, 1, sensor_size, (H, W))
    img = _grid(what, "IMAGE", xs, ys, None, ps, 1, sensor_size, (H, W))
    if interpolation == "bilinear" and padding:          # integer coordinates: the nearest image inside the padded frame
        out = torch.zeros((H + 1, W + 1), dtype=torch.float32, device=img.device)
        out[:H, :W] = img
        return out
    return img


def binary_search_torch_tensor(t, l, r, x, side='left'):
    """Binary search sorted pytorch tensor (plain Python, as it is in the reference :77-99)."""
    if r is None:
        r = len(t) - 1
    while l <= r:
        if t[l] == x:
            return l
        if t[r] == x:
            return r
        mid = l + (r - l) // 2
        midval = t[mid]
        if midval == x:
            return mid
        elif midval < x:
            l = mid + 1
        else:
            r = mid - 1
    if side == 'left':
        return l
    return r


# ------------------------------------------------------------------ time-binned grids
def _timed(what, mode, xs, ys, ts, ps, B, device, sensor_size):
    _device(what, device, xs)
    _same_length(what, xs, ys, ts, ps)
    if int(B) < 1:
        raise ValueError("%s: B must be at least 1, got %r" % (what, B))
    xs, ys = _coords(what, xs, ys)
    ts, ps = _f32(what, ts=ts, ps=ps)
    H, W = int(sensor_size[0]), int(sensor_size[1])
    return _grid(what, mode, xs, ys, ts, ps, int(B), sensor_size, (int(B), H, W))


@torch.no_grad()
def events_to_voxel_torch(xs, ys, ts, ps, B, device=None, sensor_size=(180, 240), temporal_bilinear=True):
    """Voxel grid ``[B, H, W]`` of the events between ts[0] and ts[-1] (reference :102-150): temporal bilinear weights, or
    naive accumulation per time slice.  ``len(ts) <= 3`` or all stamps zero (sorted, non-negative stamps) gives zeros."""
    return _timed("events_to_voxel_torch", "VOXEL_BILINEAR" if temporal_bilinear else "VOXEL_NAIVE", xs, ys, ts, ps, B, device,
                  sensor_size)


@torch.no_grad()
def events_to_stack_no_polarity(xs, ys, ts, ps, B, device=None, sensor_size=(180, 240)):
    """``[B, H, W]`` stack of signed sums per time slice (reference :204-240)."""
    return _timed("events_to_stack_no_polarity", "STACK_NO_POLARITY", xs, ys, ts, ps, B, device, sensor_size)


@torch.no_grad()
def events_to_voxel(xs, ys, ts, ps, num_bins, sensor_size=(180, 240)):
    """Voxel grid from stamps already normalised to [0, 1] (reference :271-286)."""
    return _timed("events_to_voxel", "VOXEL_NORMALISED", xs, ys, ts, ps, num_bins, None, sensor_size)


@torch.no_grad()
def events_to_stack_polarity(xs, ys, ts, ps, B, device=None, sensor_size=(180, 240)):
    """``[2, B, H, W]`` polarity stack (reference :153-201): the result of ``events_to_stack``, which it calls."""
    N.require_gpu(xs, ys, ts, ps)
    _device("events_to_stack_polarity", device, xs)
    return events_to_stack(xs, ys, ts, ps, B, sensor_size=sensor_size)


# ------------------------------------------------------------------ counters and masks
@torch.no_grad()
def events_to_channels(xs, ys, ps, sensor_size=(180, 240)):
    """Two-channel event image ``[2, H, W]``: sums of p * p over the positive and over the negative events (reference :289-304)."""
    _same_length("events_to_channels", xs, ys, ps)
    xs, ys = _coords("events_to_channels", xs, ys)
    ps, = _f32("events_to_channels", ps=ps)
    H, W = int(sensor_size[0]), int(sensor_size[1])
    return _grid("events_to_channels", "CHANNELS", xs, ys, None, ps, 2, sensor_size, (2, H, W))


@torch.no_grad()
def events_to_mask(xs, ys, ps, sensor_size=(180, 240)):
    """``[H, W]`` mask holding |p| of the LAST event of each pixel (reference :353-377; index_put_ without accumulation)."""
    _same_length("events_to_mask", xs, ys, ps)
    xs, ys = _coords("events_to_mask", xs, ys)
    ps, = _f32("events_to_mask", ps=ps)
    H, W = int(sensor_size[0]), int(sensor_size[1])
    return _grid("events_to_mask", "MASK", xs, ys, None, ps, 1, sensor_size, (H, W))


@torch.no_grad()
def events_polarity_mask(ps):
    """``[N, 2]`` (a transposed ``[2, N]``, as in the reference :380-391): column 0 the positive part, column 1 minus the negative."""
    ps, = _f32("events_polarity_mask", ps=ps)
    N.require_gpu(ps)
    n = int(len(ps))
    out = torch.empty((2, n), dtype=torch.float32, device=ps.device)
    with torch.cuda.device_of(ps):
        rc = N.lib().ebfi_polarity_mask(N.ptr(ps), n, N.ptr(out), N.stream_ptr(ps.device))
    N.check(rc, "ebfi_polarity_mask")
    return out.transpose(0, 1)


@torch.no_grad()
def get_hot_event_mask(event_rate, idx, max_px=100, min_obvs=5, max_rate=0.8):
    """Binary mask that removes hot pixels (reference :394-409).  EDITS ``event_rate`` in place, as the reference does: up to
    ``max_px`` times the first maximum above ``max_rate`` is cleared in ``event_rate`` and in the mask.  One launch."""
    if event_rate.dtype != torch.float32 or event_rate.dim() != 2:
        raise TypeError("get_hot_event_mask: event_rate must be a two-dimensional float32 tensor, got %s %r"
                        % (event_rate.dtype, tuple(event_rate.shape)))
    N.require_gpu(event_rate)
    H, W = int(event_rate.shape[0]), int(event_rate.shape[1])
    rounds = int(max_px) if idx > min_obvs else 0        # (idx > min_obvs is a host branch in the reference too)
    work = event_rate if event_rate.is_contiguous() else event_rate.contiguous()
    mask = torch.empty((H, W), dtype=torch.float32, device=event_rate.device)
    with torch.cuda.device_of(event_rate):
        rc = N.lib().ebfi_hot_event_mask(N.ptr(work), H, W, max(rounds, 0), float(max_rate), N.ptr(mask),
                                         N.stream_ptr(event_rate.device))
    N.check(rc, "ebfi_hot_event_mask")
    if work is not event_rate:
        event_rate.copy_(work)
    return mask


@torch.no_grad()
def stack2cnt(stack):
    """``[B, TB, H, W]`` stack -> ``[B, 2, H, W]`` counts (0 positive, 1 negative; reference :412-430): round half to even, then
    sum the positive and the negated negative parts over the bin axis.  Returns a DEVICE tensor (the reference returns a CPU one)."""
    if stack.dtype != torch.float32 or stack.dim() < 2:
        raise TypeError("stack2cnt: stack must be a float32 tensor [B, TB, ...], got %s %r" % (stack.dtype, tuple(stack.shape)))
    N.require_gpu(stack)
    stack = stack.detach().contiguous()
    B, TB = int(stack.shape[0]), int(stack.shape[1])
    rest = tuple(int(s) for s in stack.shape[2:])
    plane = 1
    for s in rest:
        plane *= s
    cnt = torch.empty((B, 2) + rest, dtype=torch.float32, device=stack.device)
    with torch.cuda.device_of(stack):
        rc = N.lib().ebfi_stack_to_cnt(N.ptr(stack), B, TB, plane, N.ptr(cnt), N.stream_ptr(stack.device))
    N.check(rc, "ebfi_stack_to_cnt")
    return cnt
