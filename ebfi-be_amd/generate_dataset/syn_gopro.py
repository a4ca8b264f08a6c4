"""The synthetic-dataset step: a folder of high-frame-rate sequences -> one training clip per sequence.

Same path and flags as the reference's generate_dataset/syn_gopro.py (`--root_data_path`, `--path_to_h5`), plus `--seed`.
Every directory under --root_data_path is one sequence:

    rgb/*            colour frames (stored in the clip, BGR)
    mono/*           gray frames the events are simulated from; when the directory is missing or empty, gray is formed from
                     the colour frames on the device (OpenCV's 8-bit BGR -> GRAY fixed point)
    timestamps.txt   one time in seconds per simulated frame

The events come from ebfi_amd.esim.EventSimulator -- the device kernels that stand in for esim_py, which the reference
drives here -- with the reference's thresholds: Cp ~ U(0.2, 0.5), Cn = N(1, 0.1) * Cp, both clamped to [0.2, 0.5], drawn per
sequence in that order from `random.Random(seed)`.  Frames go up chunk by chunk from pinned memory and the events come back
chunk by chunk, so device memory is bounded by the chunk.

Output, under --path_to_h5: `<sequence>.npz` in the layout ebfi_amd.clipdata reads (`train_ours.py --data`): images BGR uint8
[N, H, W, 3] (frame i at time i / fps), xs / ys int16, ts float64, ps int8, and event_idx by the reference packager's rule
min(E - 1, max(0, searchsorted(ts, t_i, 'left') - 1)); and config/config.txt, config/ct.txt as the reference writes them.  HDF5
output is not written (no h5py where this runs; clipdata reads .npz).
"""
import argparse
import os
import random
import sys

import numpy as np

PKG = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if PKG not in sys.path:
    sys.path.insert(0, PKG)

# What config/config.txt records, in the reference's key order and with its values; the thresholds are drawn from it.
SETTINGS = (
    ("Cp_init", 0.1), ("Cn_init", 0.1),
    ("refractory_period", 1e-4), ("log_eps", 1e-3), ("use_log", True),
    ("CT_range", [0.2, 0.5]), ("max_CT", 0.5), ("min_CT", 0.2),
    ("mu", 1), ("sigma", 0.1),
    ("fps", 240),
)
settings = dict(SETTINGS)

DEFAULT_CHUNK = 16     # frames uploaded and simulated at a time

FLAGS = (          # (name, type, default, help): the reference's two, then --seed
    ("--root_data_path", str, "/path/to/data", "directory whose sub-directories are the sequences"),
    ("--path_to_h5", str, "/path/to/output", "directory the clips and config/ are written to"),
    ("--seed", int, 0, "seed of the per-sequence threshold draws"),
)


def get_flags(argv=None):
    parser = argparse.ArgumentParser(description=__doc__.split("\n")[0])
    for name, kind, default, text in FLAGS:
        parser.add_argument(name, type=kind, default=default, help=text)
    return parser.parse_args(argv)


def clamp_threshold(c):
    return min(settings["max_CT"], max(settings["min_CT"], c))


def draw_thresholds(rng):
    """(Cp, Cn) of one sequence from `rng` (a random.Random): one uniform draw over CT_range for Cp, then one normal draw
    (mu, sigma) scaling it into Cn -- the reference's order -- and both clamped to [min_CT, max_CT] afterwards."""
    lo, hi = settings["CT_range"]
    positive = rng.uniform(lo, hi)
    negative = positive * rng.gauss(settings["mu"], settings["sigma"])
    return clamp_threshold(positive), clamp_threshold(negative)


def event_indices(ts, frame_times):
    """event_idx of every stored frame: min(E - 1, max(0, searchsorted(ts, t, 'left') - 1)); 0 for a clip without events."""
    E = len(ts)
    if E == 0:
        return np.zeros(len(frame_times), dtype=np.int64)
    idx = np.searchsorted(ts, np.asarray(frame_times, dtype=np.float64), side='left').astype(np.int64) - 1
    return np.minimum(E - 1, np.maximum(0, idx))


def write_settings(path):
    """config.txt: one `key: value ` line per setting (a blank before the newline, as the reference's file has)."""
    text = "".join("%s: %s \n" % (name, value) for name, value in SETTINGS)
    with open(path, "w") as out:
        out.write(text)


def threshold_record(sequence_dir, thresholds):
    """The line of ct.txt for one sequence."""
    return "%s:Cp=%s, Cn=%s" % (sequence_dir, thresholds[0], thresholds[1])


def write_records(records, path):
    with open(path, "w") as out:
        out.write("".join(r + "\n" for r in records))


def list_frames(directory):
    """Sorted files of `directory` with the extension of the first one listed (the reference's rule); [] when there is none."""
    if not os.path.isdir(directory):
        return []
    names = [f for f in os.listdir(directory) if os.path.isfile(os.path.join(directory, f))]
    if not names:
        return []
    ext = os.path.splitext(names[0])[-1]
    return sorted(os.path.join(directory, f) for f in names if f.endswith(ext))


def read_bgr(path):
    from PIL import Image
    with Image.open(path) as im:
        return np.ascontiguousarray(np.asarray(im.convert('RGB'))[:, :, ::-1])


def read_for_events(path):
    """A frame the events are simulated from: uint8 [H, W] when the file stores 8-bit gray, else BGR uint8 [H, W, 3] (the
    device forms the gray)."""
    from PIL import Image
    with Image.open(path) as im:
        if im.mode == 'L':
            return np.asarray(im).copy()
        if im.mode in ('RGB', 'RGBA', 'P'):
            return np.ascontiguousarray(np.asarray(im.convert('RGB'))[:, :, ::-1])
        raise ValueError('%s: image mode %s is not 8-bit gray or colour' % (path, im.mode))


def read_timestamps(path):
    with open(path) as f:
        return [float(ln) for ln in f if ln.strip()]


def settle_boundary(prev, new):
    """Two consecutive pieces of a piecewise simulation, each (xs, ys, ts, ps) in the law's order (t, y, x, emission), put into
    that order across their boundary.  An event of the later piece can round onto the boundary frame's time and tie with events
    the earlier piece has exactly there, and the tie is ordered by (y, x), not by piece.  Only the overlapping tail and head
    are re-sorted (a stable sort: equal (t, y, x) keep earlier-piece-first, the emission order); usually there is no overlap.
    -> the two pieces, rearranged where needed."""
    if len(prev[2]) == 0 or len(new[2]) == 0 or new[2][0] > prev[2][-1]:
        return prev, new
    a = int(np.searchsorted(prev[2], new[2][0], side='left'))
    b = int(np.searchsorted(new[2], prev[2][-1], side='right'))
    joined = [np.concatenate([u[a:], v[:b]]) for u, v in zip(prev, new)]
    order = np.lexsort((joined[0], joined[1], joined[2]))          # by t, then y, then x; stable
    joined = [v[order] for v in joined]
    cut = len(prev[2]) - a
    return (tuple(np.concatenate([u[:a], j[:cut]]) for u, j in zip(prev, joined)),
            tuple(np.concatenate([j[cut:], v[b:]]) for j, v in zip(joined, new)))


def simulate_sequence(esim, paths, times, chunk, device):
    """Events of the frames at `paths`: chunks of frames staged in pinned memory, uploaded, simulated with the state carried,
    and the events of every chunk copied back and settled against the chunk before (settle_boundary).  -> host arrays xs, ys,
    ts, ps in the law's order over the whole sequence."""
    import torch
    if len(paths) != len(times):
        raise ValueError('%d frames but %d timestamps' % (len(paths), len(times)))
    esim.reset()
    pieces = []
    shape = None
    for a in range(0, len(paths), chunk):
        frames = [read_for_events(p) for p in paths[a:a + chunk]]
        if shape is None:
            shape = frames[0].shape
        for p, f in zip(paths[a:a + chunk], frames):
            if f.shape != shape:
                raise ValueError('%s: frame of shape %r in a sequence of %r' % (p, f.shape, shape))
        stage = torch.empty((len(frames),) + tuple(shape), dtype=torch.uint8, pin_memory=True)
        rows = stage.numpy()
        for k, f in enumerate(frames):
            rows[k] = f
        events = esim.generate(stage.to(device, non_blocking=True), times[a:a + chunk], chunk=chunk)
        piece = tuple(v.cpu().numpy() for v in events)
        if len(piece[2]) == 0:
            continue
        if pieces:
            pieces[-1], piece = settle_boundary(pieces[-1], piece)
        pieces.append(piece)
    dtypes = (np.int16, np.int16, np.float64, np.int8)
    return tuple(np.concatenate([p[i] for p in pieces]) if pieces else np.zeros(0, dt) for i, dt in enumerate(dtypes))


def process_sequence(esim, data_dir, out_dir, chunk, device):
    """One sequence directory -> <out_dir>/<name>.npz; returns the path, or None when the sequence holds no colour frame."""
    rgb_paths = list_frames(os.path.join(data_dir, 'rgb'))
    if not rgb_paths:
        print('no colour frames under %s: nothing written' % os.path.join(data_dir, 'rgb'))
        return None
    fps = settings['fps']
    images = np.stack([read_bgr(p) for p in rgb_paths])
    mono_paths = list_frames(os.path.join(data_dir, 'mono')) or rgb_paths
    times = read_timestamps(os.path.join(data_dir, 'timestamps.txt'))
    xs, ys, ts, ps = simulate_sequence(esim, mono_paths, times, chunk, device)
    frame_times = [idx / fps for idx in range(len(images))]
    out = os.path.join(out_dir, os.path.basename(os.path.normpath(data_dir)) + '.npz')
    np.savez(out, images=images, event_idx=event_indices(ts, frame_times), xs=xs, ys=ys, ts=ts, ps=ps)
    return out


def main(argv=None, chunk=DEFAULT_CHUNK):
    import torch
    from ebfi_amd.esim import EventSimulator
    flags = get_flags(argv)
    if not torch.cuda.is_available():
        raise SystemExit('syn_gopro.py simulates the events on an MI355X; no GPU is visible (there is no CPU path)')
    device = torch.device('cuda', torch.cuda.current_device())
    out_dir = flags.path_to_h5
    os.makedirs(out_dir, exist_ok=True)
    sequences = [os.path.join(flags.root_data_path, name) for name in sorted(os.listdir(flags.root_data_path))]
    sequences = [d for d in sequences if os.path.isdir(d)]

    rng = random.Random(flags.seed)
    fixed = (settings['refractory_period'], settings['log_eps'], settings['use_log'])
    esim = EventSimulator(settings['Cp_init'], settings['Cn_init'], *fixed)
    records = []
    for seq in sequences:
        thresholds = draw_thresholds(rng)          # (drawn for every sequence, also one without frames: the draw order holds)
        records.append(threshold_record(seq, thresholds))
        print(records[-1])
        esim.setParameters(*thresholds, *fixed)
        process_sequence(esim, seq, out_dir, chunk, device)

    notes = os.path.join(out_dir, 'config')
    os.makedirs(notes, exist_ok=True)
    write_settings(os.path.join(notes, 'config.txt'))
    write_records(records, os.path.join(notes, 'ct.txt'))
    print('%d sequences done' % len(sequences))
    return 0


if __name__ == '__main__':
    sys.exit(main())
