"""Per-layer statistics of the flat parameter and gradient buffers on the device (csrc/telemetry.hip).

``segment_stats``: float32 [n] + int64 [S + 1] segment offsets on the device -> (moments float64 [S, 6] = finite count, non-finite
count, min, max, sum, sum of squares; histogram int32 [S, nb] over ascending float64 bucket limits, bucket i holding the finite
values in (limit[i - 1], limit[i]]).  ``default_bucket_limits`` is TensorFlow's default histogram table, built once on the host.
``parameter_groups`` cuts a model's parameters into the segments the monitor reports: named_parameters order grouped by the first
`group_depth` components of the names -- contiguous runs of FlatAdam.flat and FlatGradBucket.flat.

Inputs must be GPU tensors; there is no CPU path (tests/telemetry_ref.py restates the arithmetic in numpy for the tests).
"""
import sys

import numpy as np
import torch

from . import _native as N

MOMENTS = ("count", "nonfinite", "min", "max", "sum", "sum_squares")

_limits_host = None


def default_bucket_limits():
    """TensorFlow's default histogram limits: 1e-12 * 1.1^k below 1e20 on both sides of 0.0, closed by DBL_MAX (float64 [1550])."""
    global _limits_host
    if _limits_host is None:
        pos = []
        v = 1e-12
        while v < 1e20:
            pos.append(v)
            v *= 1.1
        _limits_host = np.array([-p for p in reversed(pos)] + [0.0] + pos + [sys.float_info.max], dtype=np.float64)
        _limits_host.setflags(write=False)
    return _limits_host


def parameter_groups(named_params, group_depth=2):
    """[(name, parameter)] in flat-buffer order -> (group names, offsets [S + 1]): consecutive parameters whose names share the
    first `group_depth` dot-separated components form one segment.  A prefix that comes back after another one (not the case for
    module trees, whose named_parameters walk is depth-first) would start a second segment: refused, the tags would collide."""
    depth = max(1, int(group_depth))
    names, offsets, off = [], [0], 0
    for name, p in named_params:
        group = ".".join(name.split(".")[:depth])
        if not names or names[-1] != group:
            if group in names:
                raise ValueError("parameter_groups: group %r is not contiguous in the parameter order" % group)
            if names:
                offsets.append(off)
            names.append(group)
        off += int(p.numel())
    offsets.append(off)
    if not names:
        return [], [0]
    return names, offsets


class SegmentStats:
    """The statistics of one segment table, with every device buffer allocated once: `run(flat)` puts the three
    launches on the current stream and returns (moments, hist) -- the SAME tensors at every call, overwritten by the next one.
    Nothing is allocated and nothing is read back in `run`: it can be captured into a graph."""

    def __init__(self, offsets, numel, device, limits=None):
        self.device = torch.device(device)
        if self.device.type != "cuda":
            raise NotImplementedError("ebfi_amd.telemetry runs on an MI355X through libebfi_hip.so only; got device %s" % self.device)
        if self.device.index is None:
            self.device = torch.device("cuda", torch.cuda.current_device())
        offsets = [int(v) for v in offsets]
        if len(offsets) < 1 or any(b < a for a, b in zip(offsets, offsets[1:])) or offsets[0] < 0 or offsets[-1] > int(numel):
            raise ValueError("SegmentStats: offsets must ascend inside [0, %d]" % int(numel))
        self.numel, self.segments = int(numel), len(offsets) - 1
        limits = default_bucket_limits() if limits is None else np.asarray(limits, dtype=np.float64)
        if limits.ndim != 1 or limits.size < 1 or np.any(np.diff(limits) < 0):
            raise ValueError("SegmentStats: bucket limits must be an ascending vector")
        self.limits_host = limits
        self.offsets = torch.tensor(offsets, dtype=torch.int64, device=self.device)
        self.limits = torch.from_numpy(np.array(limits)).to(self.device)
        self.moments = torch.empty((self.segments, len(MOMENTS)), dtype=torch.float64, device=self.device)
        self.hist = torch.empty((self.segments, limits.size), dtype=torch.int32, device=self.device)
        nbytes = N.lib().ebfi_segment_stats_workspace(self.numel, self.segments)
        self.workspace = torch.empty(max(nbytes // 8, 2), dtype=torch.float64, device=self.device)

    @torch.no_grad()
    def run(self, flat):
        N.require_gpu(flat)
        if flat.dtype != torch.float32 or flat.dim() != 1 or not flat.is_contiguous() or flat.numel() != self.numel \
                or flat.device != self.device:
            raise ValueError("SegmentStats.run: expected a contiguous float32 [%d] tensor on %s, got %s %r on %s"
                             % (self.numel, self.device, flat.dtype, tuple(flat.shape), flat.device))
        with torch.cuda.device(self.device):
            rc = N.lib().ebfi_segment_stats(N.ptr(flat), self.numel, N.ptr(self.offsets), self.segments, N.ptr(self.limits),
                                            int(self.limits_host.size), N.ptr(self.moments), N.ptr(self.hist), N.ptr(self.workspace),
                                            self.workspace.numel() * 8, N.stream_ptr(self.device))
        N.check(rc, "ebfi_segment_stats")
        return self.moments, self.hist


def segment_stats(flat, offsets, limits=None):
    """One-off form: builds a SegmentStats for (offsets, flat) and runs it.  offsets: a sequence of S + 1 ints."""
    return SegmentStats(offsets, flat.numel(), flat.device, limits).run(flat)


def histogram_span(limits, counts):
    """(bucket_limit, bucket) of a HistogramProto from a full count row: only the span between the first and the last non-empty
    bucket is kept (an all-empty row gives two empty lists)."""
    nz = np.flatnonzero(np.asarray(counts))
    if nz.size == 0:
        return [], []
    lo, hi = int(nz[0]), int(nz[-1]) + 1
    return [float(v) for v in limits[lo:hi]], [float(v) for v in counts[lo:hi]]
