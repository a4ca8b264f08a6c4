"""CPU restatement of the event-simulation law of the synthetic-dataset step (include/ebfi_hip.h, ebfi_esim_*), in plain Python
floats (IEEE float64, one rounding per operation) and numpy.  It is the yardstick of the device kernels (test_gpu_esim.py) and is
itself held to hand-worked cases (test_esim_host.py).  Written from the law's text, independently of csrc/esim.hip: an open
`while` instead of the counted loop, one pixel at a time, a global sort at the end instead of chunks.

The simulator the reference drives, esim_py (generate_dataset/syn_gopro.py:77-81,115-116), is neither part of the reference tree
nor installable where this runs, so nothing here is measured against it.  Where this law departs from esim_py:
  * float64 throughout.  esim_py keeps its images and levels in float32 (OpenCV CV_32F) and only the timestamps in double; here
    the level table, `it`, `ref`, `cross` and `t` are all float64, so that device and restatement can agree to the bit.
  * a defined tie order.  esim_py sorts its events by t alone (an unstable sort); with byte inputs exact ties in t are common,
    so the order is fixed as (t, y, x, emission order within the pixel).
  * the level of a byte comes from a 256-entry table, L[v] = log(log_eps + v / 255.0) or v / 255.0, made once with numpy.
  * gray from colour is OpenCV's 8-bit fixed point (4899 R + 9617 G + 1868 B + 8192) >> 14, stated here and nowhere checked
    against cv2 (not installed).
"""
import numpy as np

TOLERANCE = 1e-6


def level_table(log_eps, use_log):
    v = np.arange(256, dtype=np.float64) / 255.0
    if use_log:
        return np.log(np.float64(log_eps) + v)
    return v


def gray_from_bgr(bgr):
    """uint8 [..., 3] stored B, G, R -> uint8 [...]"""
    c = bgr.astype(np.int64)
    return ((4899 * c[..., 2] + 9617 * c[..., 1] + 1868 * c[..., 0] + 8192) >> 14).astype(np.uint8)


class PixelState:
    __slots__ = ("it", "ref", "last_t")

    def __init__(self, level):
        self.it = level
        self.ref = level
        self.last_t = 0.0


def step_pixel(s, itdt, t_prev, t_now, Cp, Cn, refractory):
    """One later frame of one pixel; returns [(t, pol), ...] in emission order and updates `s`."""
    events = []
    it = s.it
    dt = t_now - t_prev
    if abs(it - itdt) > TOLERANCE:
        pol = 1 if itdt >= it else -1
        C = Cp if pol > 0 else Cn
        cross = s.ref
        while True:
            cross = cross + pol * C
            if pol > 0:
                inside = cross > it and cross <= itdt
            else:
                inside = cross < it and cross >= itdt
            if not inside:
                break
            product = (cross - it) * dt
            quotient = product / (itdt - it)
            t = t_prev + quotient
            if s.last_t == 0.0 or (t - s.last_t) >= refractory:
                events.append((t, pol))
                s.last_t = t
            s.ref = cross
    s.it = itdt
    return events


class Simulator:
    """The restated law with state, so that piecewise feeding can be restated too.  frames: uint8 [m, H, W]; times: m floats."""

    def __init__(self, Cp, Cn, refractory_period, log_eps, use_log):
        self.Cp, self.Cn, self.refractory = float(Cp), float(Cn), float(refractory_period)
        self.L = [float(v) for v in level_table(log_eps, use_log)]
        self.state = None
        self.t_prev = None

    def generate(self, frames, times):
        frames = np.asarray(frames)
        assert frames.dtype == np.uint8 and frames.ndim == 3 and len(times) == len(frames)
        m, H, W = frames.shape
        times = [float(t) for t in times]
        start = 0
        if self.state is None and m:
            self.state = [[PixelState(self.L[int(frames[0, y, x])]) for x in range(W)] for y in range(H)]
            self.t_prev = times[0]
            start = 1
        rows = []          # (t, y, x, serial, pol)
        serial = 0
        for k in range(start, m):
            assert times[k] > self.t_prev
            for y in range(H):
                for x in range(W):
                    for t, pol in step_pixel(self.state[y][x], self.L[int(frames[k, y, x])], self.t_prev, times[k], self.Cp,
                                             self.Cn, self.refractory):
                        rows.append((t, y, x, serial, pol))
                        serial += 1
            self.t_prev = times[k]
        rows.sort(key=lambda r: r[:4])          # (t, y, x, emission order): serial grows with k, and within (k, y, x)
        xs = np.array([r[2] for r in rows], dtype=np.int16)
        ys = np.array([r[1] for r in rows], dtype=np.int16)
        ts = np.array([r[0] for r in rows], dtype=np.float64)
        ps = np.array([r[4] for r in rows], dtype=np.int8)
        return xs, ys, ts, ps


def simulate(frames, times, Cp, Cn, refractory_period, log_eps, use_log):
    return Simulator(Cp, Cn, refractory_period, log_eps, use_log).generate(frames, times)


def event_indices(ts, frame_times):
    """The reference packager's rule (generate_dataset/tools/event_packagers.py:204-226) in one expression per frame."""
    ts = np.asarray(ts, dtype=np.float64)
    E = len(ts)
    if E == 0:
        return np.zeros(len(frame_times), dtype=np.int64)
    return np.array([min(E - 1, max(0, int(np.searchsorted(ts, t, "left")) - 1)) for t in frame_times], dtype=np.int64)
