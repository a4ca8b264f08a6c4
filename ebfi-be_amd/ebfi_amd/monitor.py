"""What a training run shows while it runs: the TensorBoard log of the reference trainer (train_ours.py:283-319, :594-616) plus
per-layer weight / gradient statistics, for both trainers (train_loop of train_ours.py).  Off unless the config or a flag asks.

Scalars   `train_loss/train` and `learning rate` for every iteration, `steps_per_sec/train` as the average of each flushed interval.
          No host read per iteration: after a step the loss tensor is copied device-to-device into a ring; at each train_log_step,
          at a validation stamp or when the ring is full ONE mean all-reduce and ONE download flush it.  `valid_loss/valid` per
          validation (batch, load), `stamp_<key>` per validation stamp and `stamp_train_loss`.  With gradient clipping on
          (trainer.clip_grad) `grad_norm/total` and `grad_norm/clip_coef` for every iteration: the two floats the norm launches
          leave on the device travel through a second ring that is downloaded with the first.
Images    (trainer.vis.enabled) every train_img_writer_num-th iteration / valid_img_writer_num-th validation batch, sample 0:
          `<side>_HR_events` = event_count_images(Event.sum(1)[:1], 'green_red', black_background=True) and `<side>_blurry_frame`,
          `<side>_sharp_frame`, `<side>_gt_frame` through ONE planar_to_u8 call; the four pictures come back in one download that
          the training thread does not wait for: a writer thread waits for the copy, encodes and writes.  (planar_to_u8 clamps all three frames to
          [0, 1]; the reference clamps only the restored one, which changes nothing for frames that are images.)
Statistics(trainer.telemetry.stats_step > 0) at those iterations ebfi_segment_stats runs on FlatAdam.flat and on the reduced
          packed gradient, FlatGradBucket.flat: `weight_norm/<group>`, `grad_norm/<group>`, `grad_norm/all`,
          `grad_nonfinite/<group>`, `f16/skipped_steps` (the overflow guard's counter) and the histograms `weights/<group>`,
          `grads/<group>` (the span between the first and the last non-empty bucket).  The buffers stay on the device.
Encoding a picture (zlib, CRC32C) takes milliseconds of host time and the training thread has none to spare -- it is what keeps the
device fed -- so rank 0 hands every record to ONE writer thread, in order; the training thread only enqueues.
Every rank keeps a monitor (the ring's all-reduce is a collective); only rank 0 owns a writer, composes images and takes statistics.
"""
import math
import os
import queue
import threading
import time

import numpy as np
import torch

from . import tbevents, telemetry
from .dp import reduce_tensor

TRAIN_IMAGE_TAGS = ("train_HR_events", "train_blurry_frame", "train_sharp_frame", "train_gt_frame")
VALID_IMAGE_TAGS = ("valid_HR_events", "valid_blurry_frame", "valid_sharp_frame", "valid_gt_frame")


def monitor_settings(config, cli_tensorboard=None):
    """The reference's keys trainer.tensorboard and trainer.vis.{enabled, train_img_writer_num, valid_img_writer_num} plus
    trainer.telemetry.{stats_step, group_depth}; every absent key means off.  cli_tensorboard: --tensorboard / --no-tensorboard
    (None: the config decides)."""
    tr = (config or {}).get("trainer", {}) or {}
    vis = tr.get("vis") or {}
    tel = tr.get("telemetry") or {}
    on = bool(tr.get("tensorboard", False)) if cli_tensorboard is None else bool(cli_tensorboard)
    return {"tensorboard": on,
            "vis_enabled": on and bool(vis.get("enabled", False)),
            "train_img_writer_num": max(1, int(float(vis.get("train_img_writer_num", 20)))),
            "valid_img_writer_num": max(1, int(float(vis.get("valid_img_writer_num", 20)))),
            "stats_step": max(0, int(float(tel.get("stats_step", 0)))) if on else 0,
            "group_depth": max(1, int(tel.get("group_depth", 2)))}


def log_directory(config, runid, default_experiment="Ours"):
    tr = (config or {}).get("trainer", {}) or {}
    return os.path.join(tr.get("output_path", "./output"), "log", str(config.get("experiment", default_experiment)), str(runid))


@torch.no_grad()
def device_panels(event, frame, sharp, target, out=None):
    """The four pictures of sample 0 as ONE uint8 [4, H, W, 3] device tensor: the event-count image of Event.sum(1)[:1], then the
    blurry, restored and ground-truth frames through one planar_to_u8 call.  event [B, TB, 2, H, W]; frame / sharp / target
    [>= 1, 3, H, W].  out: the tensor to fill (allocated otherwise)."""
    from .eventvis import event_count_images
    from .frameio import planar_to_u8
    H, W = int(frame.shape[-2]), int(frame.shape[-1])
    if out is None:
        out = torch.empty((4, H, W, 3), dtype=torch.uint8, device=frame.device)
    event_count_images(event[:1].float().sum(1), "green_red", black_background=True, out=out[0:1])
    planar_to_u8(torch.cat([frame[:1].float(), sharp[:1].float(), target[:1].float()]), out=out[1:4])
    return out


def _to_host_async(t):
    """A device tensor -> (host copy in pinned memory, event that fires when it has landed); a host tensor is its own copy."""
    if not t.is_cuda:
        return t.clone(), None
    host = torch.empty(t.shape, dtype=t.dtype, pin_memory=True)
    host.copy_(t, non_blocking=True)
    ev = torch.cuda.Event()
    ev.record(torch.cuda.current_stream(t.device))
    return host, ev


class _WriterThread:
    """Runs (event, fn) jobs in order: waits for the event (a download on its way), then calls fn.  An exception in a job stops
    the writing and is raised in the training thread at the next submit or at close."""

    def __init__(self):
        self._q, self._err = queue.Queue(), None
        self._t = threading.Thread(target=self._run, name="ebfi-monitor-writer", daemon=True)
        self._t.start()

    def _run(self):
        while True:
            job = self._q.get()
            if job is None:
                return
            ev, fn = job
            try:
                if self._err is None:
                    if ev is not None:
                        ev.synchronize()
                    fn()
            except BaseException as err:      # noqa: B902 (handed to the training thread)
                self._err = err

    def _check(self):
        if self._err is not None:
            err, self._err = self._err, None
            raise RuntimeError("ebfi_amd.monitor: the writer thread failed: %r" % (err,)) from err

    def submit(self, ev, fn):
        self._check()
        self._q.put((ev, fn))

    def close(self):
        self._q.put(None)
        self._t.join()
        self._check()


class TrainMonitor:
    def __init__(self, settings, log_dir, rank=0, ring=64, writer=None, panels=None, stats_factory=None):
        """writer: an EventWriter-like object instead of a new tbevents.EventWriter(log_dir) (rank 0 only).  panels: the composer
        of the four pictures (default `device_panels`); stats_factory(offsets, numel, device) -> object with .run(flat) ->
        (moments, hist) and .limits_host (default telemetry.SegmentStats): what the host tests replace."""
        self.s = dict(settings)
        self.rank = int(rank)
        self.writer = None
        if self.rank == 0:
            self.writer = writer if writer is not None else tbevents.EventWriter(log_dir)
        self.panels = panels or device_panels
        self.stats_factory = stats_factory or telemetry.SegmentStats
        self.ring_size = max(1, int(ring))
        self._ring, self._meta = None, []              # device ring of losses; host (iteration, lr) per slot
        # second ring, only with gradient clipping on: [total norm, clipping coefficient] of every step, copied on the device from
        # FlatOptimizer.last_grad_norm and downloaded with the loss ring (the same bits on every rank: no collective)
        self._norm_ring, self.last_grad_norm = None, None
        self._mark = time.perf_counter()               # start of the interval steps_per_sec averages over
        self.last_train_loss = float("nan")
        self._jobs = _WriterThread() if self.writer is not None else None
        self._stats = None                             # (group names, weights' SegmentStats, gradients' SegmentStats)
        self.valid_iter = 0                            # the reference's valid_iter_idx: counts (batch, load) over all stamps

    # ------------------------------------------------------------------------------------------------ engine side
    def attach(self, eng):
        """Before the first step: asks the engine to keep sample 0 of the restored frame when images are on (one small copy inside
        the step, captured with it)."""
        if self.s["vis_enabled"] and self.rank == 0 and hasattr(eng, "keep_panels"):
            eng.keep_panels = True
        return self

    def _segment_stats(self, eng):
        if self._stats is None:
            model_params = {id(p): n for n, p in eng.model.named_parameters()}
            named = [(model_params[id(p)], p) for p in eng.optimizer.params]      # (the flat buffers' own order)
            names, offsets = telemetry.parameter_groups(named, self.s["group_depth"])
            flat = eng.optimizer.flat.data
            self._stats = (names, self.stats_factory(offsets, flat.numel(), flat.device),
                           self.stats_factory(offsets, flat.numel(), flat.device))
        return self._stats

    # ------------------------------------------------------------------------------------------------ training side
    def after_step(self, it, loss, lr, eng=None, batch=None):
        """After the optimiser step of iteration `it`.  loss: what train_step returned (this rank's, a 0-dim tensor); batch: the
        inputs of the iteration's last pass, (Frame, Event, T, GTEx, target) for the stage-2 engine."""
        if self._ring is None:
            self._ring = torch.zeros(self.ring_size, dtype=torch.float32, device=loss.device)
        self._ring[len(self._meta)].copy_(loss.detach().reshape(()))
        norm = getattr(getattr(eng, "optimizer", None), "last_grad_norm", None)
        if norm is not None:
            if self._norm_ring is None:
                self._norm_ring = torch.zeros(self.ring_size, 2, dtype=torch.float32, device=norm.device)
            self._norm_ring[len(self._meta)].copy_(norm)
        self._meta.append((int(it), float(lr)))
        if self.rank == 0:
            if self.s["vis_enabled"] and it % self.s["train_img_writer_num"] == 0 and eng is not None and batch is not None:
                sharp = getattr(eng, "panel_sharp", None)
                if sharp is not None and len(batch) >= 5:
                    self._images(TRAIN_IMAGE_TAGS, it, batch[1], batch[0], sharp, batch[4])
            if self.s["stats_step"] and it % self.s["stats_step"] == 0 and eng is not None:
                self._statistics(it, eng)
        if len(self._meta) == self.ring_size:
            self.flush()

    def flush(self):
        """ONE mean all-reduce and ONE download for the iterations since the last flush; every rank calls it at the same
        iterations.  Returns the reduced loss of the latest iteration (the last flushed one when the ring is empty)."""
        k = len(self._meta)
        if k == 0:
            return self.last_train_loss
        host = reduce_tensor(self._ring[:k].clone()).cpu().numpy()
        # (a copy in every case: on host tensors .cpu() is the ring itself, which later steps overwrite before the writer runs)
        norms = None if self._norm_ring is None else self._norm_ring[:k].to("cpu", copy=True).numpy()
        now = time.perf_counter()
        if self.writer is not None:
            meta, rate = self._meta, k / max(now - self._mark, 1e-9)

            def write():
                for (it, lr), v in zip(meta, host):
                    self.writer.add_scalar("train_loss/train", v, it)
                    self.writer.add_scalar("learning rate", lr, it)
                if norms is not None:
                    for (it, _), (total, coef) in zip(meta, norms):
                        self.writer.add_scalar("grad_norm/total", total, it)
                        self.writer.add_scalar("grad_norm/clip_coef", coef, it)
                self.writer.add_scalar("steps_per_sec/train", rate, meta[-1][0])
                self.writer.flush()
            self._jobs.submit(None, write)
        self._mark = now
        self.last_train_loss = float(host[-1])
        if norms is not None:
            self.last_grad_norm = (float(norms[-1][0]), float(norms[-1][1]))
        self._meta = []
        return self.last_train_loss

    def scalar(self, tag, value, step):
        """One further scalar (a host value the caller read at a log step), written by the writer thread on rank 0."""
        if self.writer is not None:
            self._jobs.submit(None, lambda: self.writer.add_scalar(tag, float(value), int(step)))

    def pause(self, seconds):
        """Takes time that was not training (a validation stamp) off the interval steps_per_sec averages over."""
        self._mark += seconds

    # ------------------------------------------------------------------------------------------------ validation side
    def valid_batch(self, valid_loss, eng=None):
        """After every validation (batch, load): valid_loss is the rank-averaged host value."""
        if self.writer is not None:
            step = self.valid_iter
            self._jobs.submit(None, lambda: self.writer.add_scalar("valid_loss/valid", valid_loss, step))
            panels = getattr(eng, "last_valid_panels", None) if eng is not None else None
            if self.s["vis_enabled"] and self.valid_iter % self.s["valid_img_writer_num"] == 0 and panels is not None:
                frame, event, sharp, target = panels
                self._images(VALID_IMAGE_TAGS, self.valid_iter, event, frame, sharp, target)
        self.valid_iter += 1

    def stamp(self, valid_stamp, val_log):
        """After a validation stamp, on every rank (the ring's flush is a collective)."""
        train_loss = self.flush()
        if self.writer is not None:
            log = dict(val_log)

            def write():
                for key, value in log.items():
                    self.writer.add_scalar("stamp_%s" % key, value, valid_stamp)
                self.writer.add_scalar("stamp_train_loss", train_loss, valid_stamp)
                self.writer.flush()
            self._jobs.submit(None, write)

    # ------------------------------------------------------------------------------------------------ rank 0's device work
    def _images(self, tags, step, event, frame, sharp, target):
        host, ev = _to_host_async(self.panels(event, frame, sharp, target))

        def write():
            pics = host.numpy() if torch.is_tensor(host) else np.asarray(host)
            for tag, pic in zip(tags, pics):
                self.writer.add_image(tag, pic, step)
        self._jobs.submit(ev, write)

    def _statistics(self, step, eng):
        names, wstats, gstats = self._segment_stats(eng)
        copies = [_to_host_async(t) for t in wstats.run(eng.optimizer.flat.data) + gstats.run(eng.bucket.flat)]
        book = getattr(eng, "book", None)
        guard = _to_host_async(book.guard) if book is not None else None
        limits = np.asarray(wstats.limits_host)
        ev = (guard or copies[-1])[1]                  # (the copies are stream-ordered: the last one's event covers them all)

        def write():
            wm, wh, gm, gh = (c[0].numpy() for c in copies)
            w = self.writer
            for s, name in enumerate(names):
                w.add_scalar("weight_norm/%s" % name, math.sqrt(wm[s, 5]), step)
                w.add_scalar("grad_norm/%s" % name, math.sqrt(gm[s, 5]), step)
                w.add_scalar("grad_nonfinite/%s" % name, gm[s, 1], step)
            w.add_scalar("grad_norm/all", math.sqrt(float(gm[:, 5].sum())), step)
            if guard is not None:
                w.add_scalar("f16/skipped_steps", int(guard[0][1]), step)
            for tag, m, h in (("weights", wm, wh), ("grads", gm, gh)):
                for s, name in enumerate(names):
                    lim, cnt = telemetry.histogram_span(limits, h[s])
                    w.add_histogram("%s/%s" % (tag, name), {"min": m[s, 2], "max": m[s, 3], "num": m[s, 0], "sum": m[s, 4],
                                                            "sum_squares": m[s, 5], "bucket_limit": lim, "bucket": cnt}, step)
        self._jobs.submit(ev, write)

    def close(self):
        self.flush()
        if self.writer is not None:
            self._jobs.close()
            self.writer.close()
