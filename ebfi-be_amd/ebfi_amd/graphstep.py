"""What the training engines and the clip interpolator share on the host side: ONE hipGraph capture sequence (`capture`) and ONE
training stepper (`GraphStepper`: accumulation window -> one collective -> one Adam launch, eagerly or replayed from a graph).
ebfi_amd.engine.Engine and ebfi_amd.exposure_engine.ExposureEngine derive from the stepper and differ through the methods below
`_fwd_bwd`; ClipInterpolator only captures.
"""
import contextlib
import sys

import torch

from .dp import is_distributed


def capture(fn, device, warmups, before=None):
    """`warmups` passes of `fn` on a side stream, then `fn` once more captured into a hipGraph -> (graph, what fn returned in the
    capture).  `before`: called ahead of every pass, the captured one included, outside the capture.  A RuntimeError of the capture
    propagates: the caller decides between eager launches and giving up."""
    side = torch.cuda.Stream(device)                       # warm-up off the default stream (allocator, lazy inits)
    side.wait_stream(torch.cuda.current_stream(device))
    with torch.cuda.stream(side):
        for _ in range(warmups):
            if before is not None:
                before()
            fn()
    torch.cuda.current_stream(device).wait_stream(side)
    if before is not None:
        before()
    graph = torch.cuda.CUDAGraph()
    # thread_local: another thread of the process (the RCCL watchdog polling its events) must not invalidate the capture
    with torch.cuda.graph(graph, capture_error_mode="thread_local"):
        out = fn()
    return graph, out


class GraphStepper:
    """The optimiser path of a training engine.  A subclass provides `precision`, `model`, `bank` (or None), `bucket`
    (FlatGradBucket), `optimizer` (FlatAdam) and `_fwd_bwd(*inputs)` -- one forward + backward on loss / accu_step, returning the
    detached loss (or a tuple that starts with it) -- and overrides what it needs of `_guard`, `_begin_micro_step`,
    `_calibrating`, `_graph_key`, `_before_first_capture` and `_publish`."""

    def __init__(self, device, graph=False, accu_step=1, strict_graph=None):
        """strict_graph: a hipGraph capture that fails raises instead of continuing with eager launches.  Default: on when
        the process is one rank of several (a rank that silently runs ~20 % slower drags every rank of the job), off alone."""
        self.device = torch.device(device)
        self.iteration = 0                                  # optimiser steps taken (the reference's train_iter_idx)
        # gradient accumulation (trainer.accu_step, train_ours.py:206,259-277): every call of train_step is one
        # forward+backward on loss / accu_step; the all-reduce and the optimiser step happen on every accu_step-th call
        self.accu_step = max(1, int(accu_step))
        self._micro = 0
        self._accum = None
        self._steps_run = 0                                 # optimiser steps of THIS run (`iteration` continues a resumed count)
        # graph=True: forward + loss + backward + gradient packing are captured once into a hipGraph (per input shape,
        # precision and `_graph_key`) and replayed; the all-reduce and the optimiser step stay eager (train_step_graph).
        self.use_graph = bool(graph) and self.device.type == "cuda"
        self._graphs = {}
        self.graph_capture_failed, self.graph_capture_error = False, None    # set when a capture fell back to eager launches
        self.strict_graph = bool(is_distributed() if strict_graph is None else strict_graph)

    # ------------------------------------------------------------------------------------------------ what the engines override
    def _guard(self):
        """The int32[2] overflow guard whose flag travels with the packed gradient and gates the Adam launch; None: no guard."""
        return None

    def _begin_micro_step(self):
        """Runs EAGERLY before every micro-step, never inside the captured region (where an engine clears its guard)."""

    def _calibrating(self):
        """True while the steps must run eagerly whatever `use_graph` says."""
        return False

    def _graph_key(self):
        """What, besides precision, accu_step and the input shapes, a captured graph depends on."""
        return ()

    def _before_first_capture(self):
        """Runs once, ahead of the warm-up passes of the engine's first capture."""

    def _capture_snapshot(self):
        """State besides the guard that the warm-up passes of a capture change and that must be as found once the graph is
        taken (an engine whose pass trains something of its own); None: nothing."""
        return None

    def _capture_restore(self, snapshot):
        """Puts back what `_capture_snapshot` returned (called only with a snapshot that is not None)."""

    def _publish(self, out, static):
        """`out`: what `_fwd_bwd` returned -> the loss `train_step` returns.  static: `out` is a graph's output buffer, which the
        next replay overwrites: hand out a copy."""
        return out.clone() if static else out

    # ------------------------------------------------------------------------------------------------ one pass
    @property
    def settled(self):
        """True once the steps that are not the steady state are over: the calibration steps (`_calibrating`) and, with
        graph=True, the capture.  (Throughput loggers start their clock here.)"""
        if self._calibrating():
            return False
        return not self.use_graph or bool(self._graphs)

    @contextlib.contextmanager
    def _autocast(self):
        """precision 'bf16' = bf16 matrix-core operands for the 3x3 / 1x1 convs (fp32 storage and
        accumulation, ebfi_amd.conv); everything else, and precision 'fp32', computes in fp32."""
        from . import conv
        prev = conv.get_compute_dtype()
        conv.set_compute_dtype(self.precision)
        try:
            yield
        finally:
            conv.set_compute_dtype(prev)

    def _bank(self):
        """Context of one pass: the weight bank refreshed (ONE pack launch, captured with the step's graph) and active
        while the split-precision mode runs; a no-op otherwise."""
        if self.bank is None or self.precision != "bf16x3":
            return contextlib.nullcontext()
        self.bank.refresh()
        return self.bank.active()

    # ------------------------------------------------------------------------------------------------ averaged weights
    @property
    def has_ema(self):
        opt = getattr(self, "optimizer", None)
        return opt is not None and getattr(opt, "ema", None) is not None

    @contextlib.contextmanager
    def ema_weights(self):
        """Inside: the model computes with the exponential moving average of the weights (FlatOptimizer(ema=...)).  The CONTENTS
        of the flat parameter buffer and of the average are exchanged -- parameters are views of that buffer, so the model, a
        checkpoint written inside and the validator all see the averaged weights -- and exchanged back on exit, bit for bit.
        Buffers that are not parameters (running statistics of norm layers) are shared.  No tensor moves, so the captured
        graphs, the training bank (re-packed from the flat buffer by every training pass), the scale book and the accumulation
        window are left as found.  Nesting is allowed: an inner context changes nothing.  Not for use around `train_step`."""
        if not self.has_ema:
            raise ValueError("this engine keeps no moving average of the weights: build it with ema=(decay, warmup)")
        if getattr(self, "_ema_inside", False):
            yield self
            return
        self.optimizer.swap_ema()
        self._ema_inside = True
        try:
            yield self
        finally:
            self._ema_inside = False
            self.optimizer.swap_ema()

    def _use_ema(self, use_ema):
        """`use_ema` of a validate call -> the context to score under: None = the average when there is one."""
        if use_ema is None:
            use_ema = self.has_ema
        return self.ema_weights() if use_ema else contextlib.nullcontext()

    def _trainable_names(self):
        return [n for n, p in self.model.named_parameters() if p.requires_grad]

    def ema_state(self):
        """The `ema` entry of a checkpoint: {"decay", "warmup", "step", "states"}; `states` has the state_dict layout of the
        model's trainable parameters (name -> tensor, a copy) and holds the AVERAGE whether or not the call happens inside
        `ema_weights()`.  None without an average.  Reads the device's step word: a checkpoint may synchronise."""
        if not self.has_ema:
            return None
        opt = self.optimizer
        decay, warmup = opt.ema
        if getattr(self, "_ema_inside", False):                       # (the buffers hold each other's contents in there)
            views = [p.detach() for p in opt.params]
        else:
            views = opt.ema_views()
        return {"decay": decay, "warmup": warmup, "step": int(float(opt.ema_step)),
                "states": {n: v.clone() for n, v in zip(self._trainable_names(), views)}}

    @torch.no_grad()
    def load_ema_state(self, state=None):
        """Restore the average from a checkpoint's `ema` entry; None (a checkpoint without one, or --reset): start it from the
        current parameters.  decay and warm-up stay this run's.  A name or shape that does not match raises."""
        if not self.has_ema:
            return
        opt = self.optimizer
        if state is None:
            opt.reset_ema()
            return
        names, views = self._trainable_names(), opt.ema_views()
        missing = [n for n in names if n not in state["states"]]
        if missing:
            raise ValueError("checkpoint ema.states lacks %d of the model's trainable parameters (first: %s)" % (len(missing), missing[0]))
        for n, v in zip(names, views):
            src = state["states"][n]
            if tuple(src.shape) != tuple(v.shape):
                raise ValueError("checkpoint ema.states[%s] has shape %r, the model %r" % (n, tuple(src.shape), tuple(v.shape)))
            v.copy_(src.to(v))
        opt.ema_step.fill_(float(state.get("step", 0)))

    # ------------------------------------------------------------------------------------------------ the step
    def _finish_micro_step(self, wire):
        """`wire`: this call's packed gradient (of loss / accu_step) with the overflow flag behind it (FlatGradBucket.wire).
        Sums the calls of one accumulation window in place and, on the window's last call, averages over ranks -- ONE
        collective: the flag travels with the gradients -- and takes the optimiser step.  True when a step was taken."""
        if self.accu_step > 1:
            if self._micro == 0:
                self._accum = wire.clone() if self._accum is None else self._accum.copy_(wire)
            else:
                self._accum.add_(wire)           # (the flags add up too: > 0 if any micro-step raised the guard)
            self._micro += 1
            if self._micro < self.accu_step:
                return False
            self._micro = 0
            wire = self._accum
        self.bucket.adopt(wire)
        self.bucket.reduce_mean_packed()
        guard = self._guard()
        self.optimizer.step(self.bucket.flat, guard=guard, flag=self.bucket.flag if guard is not None else None)
        self.iteration += 1
        self._steps_run += 1
        return True

    def train_step(self, *inputs):
        """One forward+backward on this rank's batch (plus, every `accu_step`-th call, the gradient all-reduce and the
        optimiser step); returns the (unreduced) loss tensor, already divided by accu_step like the reference's."""
        if self.use_graph and not self._calibrating():
            return self.train_step_graph(*inputs)
        self._begin_micro_step()
        self.bucket.zero()
        out = self._fwd_bwd(*inputs)
        self.bucket.gather(self._guard())
        self._finish_micro_step(self.bucket.wire)
        return self._publish(out, False)

    def train_step_graph(self, *inputs):
        """Same step with the launches of forward + loss + backward + gradient packing (~560 for the full model) replayed from
        one hipGraph.  Inputs are copied into static buffers; gradients live in the graph's memory pool, `param.grad`
        are views of the packed buffer, so the eager all-reduce / Adam that follow see ordinary tensors."""
        key = (self.precision,) + tuple(self._graph_key()) + (self.accu_step,) + tuple((tuple(v.shape), v.dtype) for v in inputs)
        entry = self._graphs.get(key)
        if entry is None:
            static_in = [torch.empty_like(v) for v in inputs]
            for s, v in zip(static_in, inputs):
                s.copy_(v)
            # The warm-up passes and the capture run _fwd_bwd (with a scale book: -> book.finish()) outside any accumulation
            # window: a flag they raise (or their three advances of the delayed scales on one batch) must not leak into the
            # window this call belongs to -- with accu_step > 1 the capture can happen mid-window, where nothing clears the guard
            # afterwards (round-4 advisory).  The guard words are restored after the capture; the scales keep what the warm-up
            # passes measured on this batch (restoring them could undo the just-in-time calibration of a slot first met here).
            guard = self._guard()
            saved = None if guard is None else guard.clone()
            snapshot = self._capture_snapshot()
            if not self._graphs:
                self._before_first_capture()

            def packed_pass():
                out = self._fwd_bwd(*static_in)
                self.bucket.gather(guard)
                return out, self.bucket.wire

            try:
                graph, (out, wire) = capture(packed_pass, self.device, 2, before=self.bucket.zero)
            except RuntimeError as err:
                name, reason = type(self).__module__, str(err).splitlines()[0]
                if saved is not None:
                    torch.cuda.synchronize(self.device)
                    guard.copy_(saved)
                if snapshot is not None:
                    torch.cuda.synchronize(self.device)
                    self._capture_restore(snapshot)
                if self.strict_graph:
                    raise RuntimeError("%s: hipGraph capture failed and strict_graph is set (the default for one rank of "
                                       "several): %s" % (name, reason)) from err
                # a capture that cannot be taken must not cost the run: say so and continue with eager launches
                print("%s: hipGraph capture failed (%s); continuing with eager launches" % (name, reason), file=sys.stderr, flush=True)
                self.use_graph = False
                self.graph_capture_failed, self.graph_capture_error = True, reason
                torch.cuda.synchronize(self.device)
                return self.train_step(*inputs)
            if saved is not None:
                guard.copy_(saved)
            if snapshot is not None:
                self._capture_restore(snapshot)
            entry = self._graphs[key] = (graph, static_in, out, wire, [p.grad for p in self.bucket.params])
        graph, static_in, out, wire, grads = entry
        self._begin_micro_step()
        for s, v in zip(static_in, inputs):
            if s.data_ptr() != v.data_ptr():
                s.copy_(v)
        graph.replay()
        self.bucket.adopt(wire)
        for p, g in zip(self.bucket.params, grads):        # (another shape's graph may have re-pointed them)
            p.grad = g
        self._finish_micro_step(wire)
        return self._publish(out, True)
