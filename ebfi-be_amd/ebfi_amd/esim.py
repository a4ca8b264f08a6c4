"""The event simulator of the synthetic-dataset step on the device (csrc/esim.hip).

``EventSimulator(Cp, Cn, refractory_period, log_eps, use_log)`` mirrors the constructor and ``setParameters`` of the
``esim_py.EventSimulator`` that generate_dataset/syn_gopro.py:77-81,115 drives; ``generate`` takes the gray frames as a uint8
tensor on the GPU instead of a folder and returns the events as device tensors.  The law is written out in include/ebfi_hip.h
(ebfi_esim_*) and restated in float64 numpy by tests/esim_ref.py; the kernels give that restatement's bits.

Per chunk of at most ``chunk`` frame intervals: the count kernel writes the events of every pixel and interval
(int32 [n, H, W]); ``torch.cumsum`` turns them into exclusive offsets; the emit kernel runs the identical walk and stores every
event at its own index (layout [interval][y][x][emission]).  The events of all chunks of a call are then put into the law's
order (t, y, x, emission order within the pixel) by two stable ``torch.sort`` passes, first on the pixel, then on t.  Sorting
on t alone would be right except where an event rounds onto a frame time at which another pixel's previous interval has an
event too: with linear levels and round thresholds that happens, and the tie must go by (y, x), not by interval.  The
per-pixel state (`it`, `ref`, `last_t`) stays on the device between chunks and between calls, so the walk's memory is bounded
by the chunk and a sequence can be fed piecewise.

ORDER ACROSS CALLS.  ``generate`` orders the events of ONE call.  Fed piecewise, the concatenated pieces are in the law's order
except for that same tie at the boundary frame's time, which a caller that needs the global order settles by re-sorting the
overlapping tail and head (generate_dataset/syn_gopro.py settle_boundary does).

TABLE CHANGES.  `it` and `ref` are levels of the table they were made with.  ``setParameters`` with another `use_log` /
`log_eps` while a state exists is refused (``reset()`` first): the old levels could lie outside the new table's range, for
which the crossing loop's bound is computed.

The level table L[v] = log(log_eps + v / 255.0) (or v / 255.0) is made HERE, once per parameter set, with numpy in float64 and
handed to the library: the kernels never call log.

Inputs must be GPU tensors; there is no CPU path.
"""
import ctypes

import numpy as np
import torch

from . import _native as N

MAX_CHUNK = N.CONSTANTS["EBFI_ESIM_MAX_CHUNK"]
MIN_THRESHOLD = 1e-3     # Cp / Cn below this are refused (the crossing loop's bound must stay small)


def level_table(log_eps, use_log):
    """float64 [256]: the level of every byte."""
    v = np.arange(256, dtype=np.float64) / 255.0
    return np.log(np.float64(log_eps) + v) if use_log else v


def _host_f64(a):
    return (ctypes.c_double * len(a))(*[float(v) for v in a])


class EventSimulator:
    def __init__(self, Cp, Cn, refractory_period, log_eps, use_log):
        self.reset()
        self.setParameters(Cp, Cn, refractory_period, log_eps, use_log)

    def setParameters(self, Cp, Cn, refractory_period, log_eps, use_log):
        """As esim_py's: new thresholds from the next frame on; the per-pixel state is kept (so the level table must stay)."""
        Cp, Cn, refractory_period, log_eps = float(Cp), float(Cn), float(refractory_period), float(log_eps)
        if not all(np.isfinite(v) for v in (Cp, Cn, refractory_period, log_eps)):
            raise ValueError("EventSimulator: parameters must be finite, got Cp=%r Cn=%r refractory_period=%r log_eps=%r"
                             % (Cp, Cn, refractory_period, log_eps))
        if Cp < MIN_THRESHOLD or Cn < MIN_THRESHOLD:
            raise ValueError("EventSimulator: Cp=%r, Cn=%r must be at least %g" % (Cp, Cn, MIN_THRESHOLD))
        if refractory_period < 0:
            raise ValueError("EventSimulator: refractory_period=%r must be >= 0" % refractory_period)
        if use_log and log_eps <= 0:
            raise ValueError("EventSimulator: log_eps=%r must be positive with use_log" % log_eps)
        levels = level_table(log_eps, bool(use_log))
        if self._state is not None and not np.array_equal(levels, self.levels):
            raise ValueError("EventSimulator.setParameters: use_log / log_eps change the level table while a per-pixel state "
                             "made with the old one exists; reset() first")
        self.Cp, self.Cn, self.refractory_period, self.log_eps, self.use_log = Cp, Cn, refractory_period, log_eps, bool(use_log)
        self.levels = levels
        self._levels_c = _host_f64(self.levels)

    def reset(self):
        """Forget the per-pixel state: the next frame handed to `generate` is a first frame again."""
        self._state = None        # float64 [3, H, W] on the device: it, ref, last_t
        self._last_time = None    # time of the frame the state stands at

    def _check_frames(self, frames):
        N.require_gpu(frames)
        if frames.dtype != torch.uint8 or frames.dim() not in (3, 4) or (frames.dim() == 4 and frames.shape[3] != 3):
            raise ValueError("EventSimulator.generate: expected uint8 [n, H, W] (gray) or [n, H, W, 3] (BGR), got %s %r"
                             % (frames.dtype, tuple(frames.shape)))
        bgr = frames.dim() == 4
        ok = (frames.stride(2) == 3 and frames.stride(3) == 1) if bgr else (frames.stride(2) == 1 or frames.shape[2] == 1)
        if not ok or frames.stride(0) < 0 or frames.stride(1) < 0:
            frames = frames.contiguous()
        return frames, bgr

    @torch.no_grad()
    def generate(self, frames_u8, times, chunk=16):
        """frames_u8: uint8 [m, H, W] gray, or [m, H, W, 3] BGR (gray is then formed on the device); any frame and row
        strides.  times: m float64 seconds (a sequence, a numpy array or a CPU tensor), strictly increasing, and later than
        everything fed before.  With no state the first frame only initialises it.  -> (xs int16, ys int16, ts float64,
        ps int8) device tensors in the order (t, y, x, emission order within the pixel).  Runs on the current stream; each chunk
        reads its event count back to size the output."""
        frames, bgr = self._check_frames(frames_u8)
        times = np.asarray(times.cpu() if isinstance(times, torch.Tensor) else times, dtype=np.float64).reshape(-1)
        m, H, W = (int(v) for v in frames.shape[:3])
        if len(times) != m:
            raise ValueError("EventSimulator.generate: %d frames but %d times" % (m, len(times)))
        chunk = int(chunk)
        if not 1 <= chunk <= MAX_CHUNK:
            raise ValueError("EventSimulator.generate: chunk=%d outside [1, %d]" % (chunk, MAX_CHUNK))
        dev = frames.device
        h = N.lib()
        out = ([], [], [], [])
        with torch.cuda.device_of(frames):
            stream = N.stream_ptr(dev)
            first = 0
            if self._state is None and m > 0:
                state = torch.empty((3, H, W), dtype=torch.float64, device=dev)
                N.check(h.ebfi_esim_init(N.ptr(frames), int(frames.stride(1)), int(bgr), H, W, self._levels_c, N.ptr(state),
                                         stream), "ebfi_esim_init")
                self._state, self._last_time, first = state, float(times[0]), 1
            elif m > 0:
                if tuple(self._state.shape[1:]) != (H, W) or self._state.device != dev:
                    raise ValueError("EventSimulator.generate: frames of %d x %d on %s after a state of %r on %s (reset() first)"
                                     % (H, W, dev, tuple(self._state.shape[1:]), self._state.device))
            strides = (ctypes.c_int64 * 2)(int(frames.stride(0)), int(frames.stride(1)))
            for a in range(first, m, chunk):
                b = min(a + chunk, m)
                n = b - a
                part = frames[a:b]
                t_c = _host_f64([self._last_time] + list(times[a:b]))
                walk = (N.ptr(part), strides, int(bgr), n, H, W, t_c, self._levels_c, self.Cp, self.Cn, self.refractory_period)
                counts = torch.empty((n, H, W), dtype=torch.int32, device=dev)
                N.check(h.ebfi_esim_count(*walk, N.ptr(self._state), N.ptr(counts), stream), "ebfi_esim_count")
                ends = torch.cumsum(counts.view(-1), 0, dtype=torch.int64)
                total = int(ends[-1].item())
                offsets = ends - counts.view(-1)
                xs = torch.empty(total, dtype=torch.int16, device=dev)
                ys = torch.empty(total, dtype=torch.int16, device=dev)
                ts = torch.empty(total, dtype=torch.float64, device=dev)
                ps = torch.empty(total, dtype=torch.int8, device=dev)
                N.check(h.ebfi_esim_emit(*walk, N.ptr(self._state), N.ptr(offsets), total, N.ptr(xs), N.ptr(ys), N.ptr(ts),
                                         N.ptr(ps), stream), "ebfi_esim_emit")
                self._last_time = float(times[b - 1])
                for lst, v in zip(out, (xs, ys, ts, ps)):
                    lst.append(v)
        if not out[0]:
            return (torch.empty(0, dtype=torch.int16, device=dev), torch.empty(0, dtype=torch.int16, device=dev),
                    torch.empty(0, dtype=torch.float64, device=dev), torch.empty(0, dtype=torch.int8, device=dev))
        xs, ys, ts, ps = (v[0] if len(v) == 1 else torch.cat(v) for v in out)
        if ts.numel():
            # [interval][y][x][emission] -> (y, x, interval, emission) -> (t, y, x, interval, emission): two stable sorts
            order = torch.sort(ys.to(torch.int32) * W + xs.to(torch.int32), stable=True)[1]
            ts, by_t = torch.sort(ts[order], stable=True)
            order = order[by_t]
            xs, ys, ps = xs[order], ys[order], ps[order]
        return xs, ys, ts, ps
