"""Data parallelism for the training step: one process per GPU, RCCL over xGMI.

The reference wraps the model in DistributedDataParallel (train_ours.py:754) but runs forward AND
backward inside ``model.no_sync()`` on every iteration (train_ours.py:250-272), so its gradient
all-reduce never fires; ranks only share the initial broadcast.  This module implements what that
code evidently intends: identical replicas, per-rank batches, gradients averaged every step.

MI355X-first choices: the whole model is 5.69 M parameters = 22.8 MB of fp32
gradients.  xGMI is point-to-point (7 links per GPU), a ring all-reduce is bound by one link, so
many small buckets would only multiply latency.  We therefore pack ALL gradients into ONE flat
buffer (one gather launch after backward: csrc/optim.hip grad_gather) and issue exactly ONE collective
per optimiser step on it (average = SUM then one fused scale); afterwards ``param.grad`` are views of
that buffer.  The overflow flag of the fp16 backward rides in the same message (one extra element:
SUM > 0 <=> some rank raised it), so a step has one all-reduce, not two.
With gloo (CPU tests) the same code path runs unchanged.
"""
import os

import torch
import torch.distributed as dist

from . import _native as N


def is_distributed():
    """More than one rank -- or EBFI_FORCE_COLLECTIVES=1 with an initialised group of one: the collectives then run at
    world size 1 (bench.py EBFI_BENCH_FORCE_DIST: what a one-GPU box can exercise of the RCCL path)."""
    if not (dist.is_available() and dist.is_initialized()):
        return False
    return dist.get_world_size() > 1 or os.environ.get("EBFI_FORCE_COLLECTIVES") == "1"


@torch.no_grad()
def sync_guard(guard):
    """Overflow guard of the fp16 backward (ebfi_amd.f16scale: int32[2] = [flag of this step, skipped steps]) MAX-reduced over
    ranks with a collective of its own.  The engine does NOT use this any more: FlatGradBucket.gather(guard=...) carries the
    flag inside the gradient message (one collective per step); kept for callers that hold a guard without a bucket."""
    if guard is not None and is_distributed():
        if guard.is_cuda and dist.get_backend() == "gloo":     # (rehearsal fabric: reduce through the host)
            host = guard[0:1].cpu()
            dist.all_reduce(host, op=dist.ReduceOp.MAX)
            guard[0:1].copy_(host)
        else:
            dist.all_reduce(guard[0:1], op=dist.ReduceOp.MAX)
    return guard


@torch.no_grad()
def reduce_tensor(input_tensor, average=True):
    """myutils/utils.py:80-92: barrier + all_reduce(SUM) (+ / world); identity on one rank."""
    if not (dist.is_available() and dist.is_initialized()):
        return input_tensor
    world_size = dist.get_world_size()
    if world_size < 2:
        return input_tensor
    dist.barrier()
    dist.all_reduce(input_tensor)
    if average:
        input_tensor /= world_size
    return input_tensor


@torch.no_grad()
def broadcast_parameters(module, src=0):
    """What the DDP constructor does once (train_ours.py:754): rank `src`'s parameters and buffers
    to everyone, as one flat message per dtype."""
    if not is_distributed():
        return
    tensors = [p.data for p in module.parameters()] + [b.data for b in module.buffers()]
    by_dtype = {}
    for t in tensors:
        by_dtype.setdefault((t.dtype, t.device), []).append(t)
    for group in by_dtype.values():
        flat = torch.cat([t.reshape(-1) for t in group])
        dist.broadcast(flat, src)
        off = 0
        for t in group:
            t.copy_(flat[off:off + t.numel()].view_as(t))
            off += t.numel()


WIRE_PAD = 4               # floats behind the gradients in the wire buffer: [overflow flag, 0, 0, 0] (keeps 16-byte multiples)


class FlatGradBucket:
    """All trainable gradients of `module` in one contiguous buffer, built AFTER backward.

    Autograd hands every parameter a freshly written gradient tensor (the conv kernels already write
    their own outputs), so the cheapest way to a flat buffer is one gather per step (libebfi_hip.so
    `ebfi_grad_gather`: the source pointers travel by value in the kernel arguments, 128 tensors per
    launch, one workgroup per 16384-element chunk; 22.8 MB read + written once) instead of 255 in-place
    accumulations into pre-assigned views plus a memset -- or a 255-piece torch.cat, whose batched copy
    gives every input the same number of workgroups and took 90 us.  ``gather()`` packs,
    ``all_reduce_mean()`` averages over ranks with one collective, and afterwards every ``param.grad``
    is a view of the flat buffer, so optimisers see ordinary ``.grad`` tensors.  ``zero()`` drops the
    gradients (set-to-None) for the next step.

    Wire format: ``wire`` = [numel gradients | flag | 3 zeros]; ``flat`` = wire[:numel].  ``flag`` is the
    overflow guard of the fp16 backward as a float (gather(guard=book.guard) writes guard[0] != 0 there),
    summed over ranks by the SAME all-reduce: a positive value on any rank skips the update on all."""

    def __init__(self, module, dtype=None):
        self.params = [p for p in module.parameters() if p.requires_grad]
        if not self.params:
            raise ValueError("module has no trainable parameters")
        self.dtype = dtype or self.params[0].dtype
        self.numel = sum(p.numel() for p in self.params)
        self.wire = None
        self.flat = None
        self._offsets = []
        off = 0
        for p in self.params:
            self._offsets.append(off)
            off += p.numel()
        self._numels = None                         # ctypes int64 array of the parameters' element counts (native gather)

    @property
    def flag(self):
        """The overflow flag element of the wire buffer (a 1-element view), None before the first gather."""
        return None if self.wire is None else self.wire[self.numel:self.numel + 1]

    def zero(self):
        for p in self.params:
            p.grad = None

    def adopt(self, wire):
        """Make `wire` (a full wire buffer, e.g. a graph's static output or an accumulation buffer) the current one."""
        self.wire = wire
        self.flat = wire[:self.numel]

    def gather(self, guard=None):
        """Pack the per-parameter gradients (missing ones count as zero) into a fresh wire buffer and re-point .grad at it.
        `guard`: int32[2] device tensor of f16scale.ScaleBook (or a CPU tensor in the gloo tests): its flag rides along."""
        dev = self.params[0].device
        grads = []
        for p in self.params:
            g = p.grad
            if g is not None and (g.dtype != self.dtype or not g.is_contiguous()):
                g = g.to(self.dtype).contiguous()
            grads.append(g)
        if dev.type != "cuda" or self.dtype != torch.float32:
            # CPU parameters (host tests, gloo rehearsals) and bucket dtypes the native launch does not pack: one concatenation
            flag = torch.zeros(WIRE_PAD, dtype=self.dtype, device=dev)
            if guard is not None:
                flag[0] = 1.0 if int(guard[0]) != 0 else 0.0
            pieces = [(g if g is not None else torch.zeros_like(p, dtype=self.dtype)).reshape(-1) for g, p in zip(grads, self.params)]
            self.adopt(torch.cat(pieces + [flag]))
        else:
            if guard is not None and not (guard.is_cuda and guard.device == dev and guard.dtype == torch.int32):
                # (the kernel dereferences this pointer: a host tensor -- the gloo tests pass one with CPU parameters -- or
                # another dtype must be staged, never handed over as it is)
                guard = guard.to(device=dev, dtype=torch.int32)
            import ctypes
            from . import _native as N
            n = len(self.params)
            if self._numels is None:
                self._numels = (ctypes.c_int64 * n)(*[p.numel() for p in self.params])
            ptrs = (ctypes.c_void_p * n)(*[None if g is None else g.data_ptr() for g in grads])
            wire = torch.empty(self.numel + WIRE_PAD, dtype=self.dtype, device=dev)
            with torch.cuda.device(dev):
                rc = N.lib().ebfi_grad_gather(ptrs, self._numels, n, N.ptr(wire), self.numel, WIRE_PAD, N.ptr(guard), N.stream_ptr(dev))
            N.check(rc, "ebfi_grad_gather")
            # (the sources may be freed right away: the caching allocator reuses memory in stream order only; inside a graph
            # capture they are pool allocations whose addresses the captured launches keep)
            self.adopt(wire)
        for p, off in zip(self.params, self._offsets):
            p.grad = self.flat[off:off + p.numel()].view_as(p)
        return self.flat

    def reduce_mean_packed(self):
        """Average the already packed wire buffer over ranks in place -- gradients AND the overflow flag in ONE collective
        (no-op on one rank).  The flag ends up as (ranks that raised it) / world: > 0 iff any did."""
        if is_distributed():
            if self.wire.is_cuda and dist.get_backend() == "gloo":
                # rehearsal / CPU-only fabrics: gloo reduces device tensors through tiny staged chunks (seconds for
                # 22.8 MB); one explicit round trip through host memory is two copies and a host all-reduce
                host = self.wire.cpu()
                dist.all_reduce(host, op=dist.ReduceOp.SUM)
                self.wire.copy_(host)
            else:
                dist.all_reduce(self.wire, op=dist.ReduceOp.SUM)
            self.wire.mul_(1.0 / dist.get_world_size())
        return self.flat

    def all_reduce_mean(self, guard=None):
        """gather() + average over ranks in place.  Returns the flat buffer."""
        self.gather(guard)
        return self.reduce_mean_packed()

    def views_intact(self):
        """True while every param.grad aliases the flat buffer (debug / test helper)."""
        if self.flat is None:
            return False
        base = self.flat.untyped_storage().data_ptr()
        return all(p.grad is not None and p.grad.untyped_storage().data_ptr() == base for p in self.params)


SUPPORTED_OPTIMIZERS = ("Adam", "AdamW", "SGD")
# optimizer.args entries that say HOW a process runs the update, not what it computes: this process decides them
_RUN_MODE_ARGS = ("foreach", "fused", "capturable")
_OPTIM_ADAM, _OPTIM_SGD, _OPTIM_DECOUPLED_DECAY, _OPTIM_AMSGRAD, _OPTIM_NESTEROV = (
    N.CONSTANTS["EBFI_OPTIM_" + k] for k in ("ADAM", "SGD", "DECOUPLED_DECAY", "AMSGRAD", "NESTEROV"))


def _refuse_group(name, group):
    """Options the one-launch update does not implement are refused, never ignored."""
    for key in ("maximize", "differentiable"):
        if group.get(key):
            raise ValueError("optimizer %s: %s=True is not supported by the flat one-launch update" % (name, key))
    if torch.is_tensor(group.get("lr")):
        raise ValueError("optimizer %s: a tensor lr is not supported (hyper-parameters travel by value; set "
                         "param_groups[0]['lr'] to a float, as the LR schedulers do)" % name)


def optimizer_arguments(name, args=None):
    """Validate an `optimizer` section (config['optimizer']['name'] / ['args'], the reference's eval(name)(params, **args),
    train_ours.py:770-771) without touching a device -> the arguments FlatOptimizer passes to torch.optim.<name>.
    Supported: Adam, AdamW, SGD, with every argument of the torch class except maximize / differentiable / a tensor lr
    (ValueError); foreach / fused / capturable are run-mode flags this process decides and are dropped.  Torch's own
    constructor checks apply (negative lr, nesterov without momentum, an unknown keyword)."""
    if name not in SUPPORTED_OPTIMIZERS:
        raise ValueError("optimizer '%s' is not supported: the flat one-launch update implements %s"
                         % (name, ", ".join(SUPPORTED_OPTIMIZERS)))
    args = {k: v for k, v in dict(args or {}).items() if k not in _RUN_MODE_ARGS}
    _refuse_group(name, args)
    if "betas" in args:
        args["betas"] = tuple(float(b) for b in args["betas"])
    try:
        getattr(torch.optim, name)([torch.nn.Parameter(torch.zeros(1))], **args)
    except TypeError as e:
        raise ValueError("optimizer %s: %s" % (name, e)) from e
    return args


_NORM_L2, _NORM_INF = N.CONSTANTS["EBFI_NORM_L2"], N.CONSTANTS["EBFI_NORM_INF"]


def clip_arguments(clip):
    """Validate a gradient-clipping setting without touching a device -> (max_norm, norm_type) with norm_type 2.0 or inf, or None.
    `clip`: None, (max_norm, norm_type), {"max_norm": ..., "norm_type": ...} (norm_type defaults to 2) or a bare number."""
    if clip is None:
        return None
    if isinstance(clip, dict):
        unknown = set(clip) - {"max_norm", "norm_type"}
        if unknown or "max_norm" not in clip:
            raise ValueError("clip_grad takes max_norm and norm_type, got %r" % (sorted(clip),))
        clip = (clip["max_norm"], clip.get("norm_type", 2))
    elif isinstance(clip, (int, float)):
        clip = (clip, 2)
    try:
        max_norm, norm_type = clip
        max_norm, norm_type = float(max_norm), float(norm_type)
    except (TypeError, ValueError) as e:
        raise ValueError("clip_grad must be (max_norm, norm_type), got %r" % (clip,)) from e
    if not (max_norm > 0.0 and max_norm != float("inf")):
        raise ValueError("clip_grad: max_norm must be a positive finite number, got %r" % (max_norm,))
    if norm_type not in (2.0, float("inf")):
        raise ValueError("clip_grad: norm_type must be 2 or inf (the total norms the native reduction implements), got %r" % (norm_type,))
    return max_norm, norm_type


def ema_arguments(ema):
    """Validate a weight-average setting without touching a device -> (decay, warmup) or None.
    `ema`: None, (decay, warmup), {"decay": ..., "warmup": ...} (warmup defaults to False; other keys, such as the trainers'
    `validate`, are not this function's) or a bare decay."""
    if ema is None:
        return None
    if isinstance(ema, dict):
        if "decay" not in ema:
            raise ValueError("ema needs a decay, got %r" % (sorted(ema),))
        ema = (ema["decay"], ema.get("warmup", False))
    elif isinstance(ema, (int, float)):
        ema = (ema, False)
    try:
        decay, warmup = ema
        decay, warmup = float(decay), bool(warmup)
    except (TypeError, ValueError) as e:
        raise ValueError("ema must be (decay, warmup), got %r" % (ema,)) from e
    if not (0.0 <= decay < 1.0):
        raise ValueError("ema: decay must lie in [0, 1), got %r" % (decay,))
    return decay, warmup


class FlatOptimizer:
    """torch.optim.Adam, AdamW or SGD over ONE flat parameter buffer.

    The trainable parameters are re-pointed at views of a single contiguous buffer (their values, names and shapes do
    not change), the packed gradient of `FlatGradBucket` becomes that buffer's `.grad`, and the update is one native
    launch over 5.7 M elements (csrc/optim.hip) instead of a multi-tensor pass over 255 tensors.  `inner` is
    ``getattr(torch.optim, name)([flat], **args)``: it owns hyper-parameters and state, torch's defaults and constructor
    checks apply, and LR schedulers work on it.  `state_dict()` / `load_state_dict()` speak torch's per-parameter layout
    of that class -- what the reference's checkpoints hold (train_ours.py:621-671) -- so checkpoints stay interchangeable.

    clip = (max_norm, norm_type), norm_type 2 or inf: torch.nn.utils.clip_grad_norm_ over all parameters, without its 255
    per-tensor norms, its host-visible scalar and its in-place scaling.  `step()` launches the norm of the packed gradient
    (csrc/gradnorm.hip: float64 accumulation in a fixed order -- every rank of a job computes the same bits from the same
    all-reduced buffer) and the update reads the coefficient on the device as its gradient scale.  After a step
    `last_grad_norm` is a float32[2] tensor on the parameters' device, [total norm, coefficient]; the step never reads it back.
    The gradient buffer is only read: `param.grad` and `FlatGradBucket.flat` keep the UNCLIPPED averaged gradient (the
    `grad_norm/` layer statistics of the training monitor therefore show unclipped norms; `grad_norm/total` and
    `grad_norm/clip_coef` say what the update made of them).
    ema = (decay, warmup): `ema_flat`, a buffer beside the parameters that starts as their copy and follows every APPLIED step
    with e <- e + (1 - d)(p - e) in the update's own launch; d = decay, or min(decay, (1 + t) / (10 + t)) with warm-up, t =
    `ema_step` (a device word: a step skipped by the overflow guard neither moves the average nor counts).
    Both are off by default, and with both off `step()` launches exactly what it launched without them.  CPU tensors (host
    tests, gloo rehearsals) take the same laws in torch operations on a temporary."""

    def __init__(self, params, name="Adam", clip=None, ema=None, **args):
        args = optimizer_arguments(name, args)
        self.clip, self.ema = clip_arguments(clip), ema_arguments(ema)
        self.name = name
        self.params = [p for p in params if p.requires_grad]
        if not self.params:
            raise ValueError("no trainable parameters")
        with torch.no_grad():
            flat = torch.cat([p.data.reshape(-1) for p in self.params])
        self._offsets, off = [], 0
        for p in self.params:
            self._offsets.append(off)
            p.data = flat[off:off + p.numel()].view_as(p)
            off += p.numel()
        self.flat = torch.nn.Parameter(flat)
        self.inner = getattr(torch.optim, name)([self.flat], fused=bool(flat.is_cuda), **args)
        # SGD with momentum on the device: 0 until the first APPLIED step (the overflow guard takes a skipped one back), so
        # the kernel knows when `buf <- d` holds.  Private: torch's SGD state has no step and the exported state shows none.
        self._sgd_step = None
        self.last_grad_norm = self._norm_workspace = None
        self.ema_flat = self.ema_step = None
        if self.clip is not None:
            self.last_grad_norm = torch.tensor([0.0, 1.0], dtype=torch.float32, device=flat.device)
        if self.ema is not None:
            self.ema_flat = flat.detach().clone()
            self.ema_step = torch.zeros((), dtype=torch.float32, device=flat.device)

    @property
    def param_groups(self):
        return self.inner.param_groups

    # ------------------------------------------------------------------------------------------------ clipping / average
    def _native_norm(self, flat_grad):
        """The two norm launches on the packed gradient -> last_grad_norm (overwritten in place: a ring may copy from it)."""
        max_norm, norm_type = self.clip
        n = flat_grad.numel()
        need = N.lib().ebfi_grad_norm_workspace(n)
        if self._norm_workspace is None or self._norm_workspace.numel() * 8 < need:
            self._norm_workspace = torch.empty(max(1, need // 8), dtype=torch.float64, device=flat_grad.device)
        with torch.cuda.device_of(flat_grad):
            rc = N.lib().ebfi_grad_norm(N.ptr(flat_grad), n, _NORM_INF if norm_type == float("inf") else _NORM_L2, max_norm,
                                        N.ptr(self.last_grad_norm), N.ptr(self._norm_workspace), self._norm_workspace.numel() * 8,
                                        N.stream_ptr(flat_grad.device))
        N.check(rc, "ebfi_grad_norm")

    def _host_norm(self, flat_grad):
        """The same two numbers in torch operations (CPU tensors): float64 norm, float32 coefficient."""
        max_norm, norm_type = self.clip
        g = flat_grad.detach().double()
        if g.numel() == 0:
            self.last_grad_norm.copy_(torch.tensor([0.0, 1.0]))
            return
        norm = (g.abs().max() if norm_type == float("inf") else (g * g).sum().sqrt()).float()
        coef = torch.tensor(max_norm, dtype=torch.float32) / (norm + torch.tensor(1e-6, dtype=torch.float32))
        coef = torch.where(coef > 1.0, torch.ones_like(coef), coef)            # (a NaN stays)
        self.last_grad_norm.copy_(torch.stack([norm, coef]))

    def _host_average(self):
        """One applied average in torch operations (CPU tensors), every operation rounded to float32 once."""
        decay, warmup = self.ema
        self.ema_step += 1
        t = float(self.ema_step)
        d = min(decay, (1.0 + t) / (10.0 + t)) if warmup else decay
        w = float(torch.tensor(1.0 - d, dtype=torch.float64).float())
        delta = self.flat.detach() - self.ema_flat
        self.ema_flat.add_(delta.mul_(w))

    @torch.no_grad()
    def reset_ema(self):
        """Start the average again from the current parameters (a loaded model without an average of its own)."""
        if self.ema is not None:
            self.ema_flat.copy_(self.flat.detach())
            self.ema_step.zero_()

    @torch.no_grad()
    def swap_ema(self):
        """Exchange the CONTENTS of the parameter buffer and the average (addresses, views and the graphs that hold them stay):
        the model then computes with the averaged weights.  A second call restores both, bit for bit."""
        if self.ema is None:
            raise ValueError("this optimiser keeps no moving average of the weights (ema=None)")
        keep = self.flat.detach().clone()
        self.flat.data.copy_(self.ema_flat)
        self.ema_flat.copy_(keep)

    def ema_views(self):
        """The average in the shapes of `params`, as views of `ema_flat`."""
        return [self.ema_flat[sl].view_as(p) for _, p, sl in self._slices()]

    def step(self, flat_grad, guard=None, flag=None):
        """`flat_grad`: the packed gradient in the order of `params` (FlatGradBucket.flat).  `guard`: int32[2] tensor of
        ebfi_amd.f16scale.ScaleBook -- a non-zero guard[0] skips this update (guard[1] counts the skipped steps).  `flag`:
        FlatGradBucket.flag after the all-reduce -- the ranks' overflow flags summed by the gradient collective; a non-zero
        (or non-finite) value skips the update as well and is written back to guard[0], so every rank takes the same branch."""
        if flat_grad.numel() != self.flat.numel():
            raise ValueError("packed gradient has %d elements, parameters %d" % (flat_grad.numel(), self.flat.numel()))
        if flag is not None and guard is None:
            raise ValueError("an overflow flag needs the guard tensor that counts the skipped steps")
        if self._native_step(flat_grad, guard, flag):
            return
        _refuse_group(self.name, self.inner.param_groups[0])
        if self.clip is not None:
            self._host_norm(flat_grad)
        if guard is not None:                                     # torch's own step (CPU tensors): host-side check
            if flag is not None and not float(flag[0]) == 0.0:
                guard[0] = 1
            if int(guard[0].item()) != 0:
                guard[1] += 1
                return
        # (the scaled gradient is a temporary: the packed buffer keeps the unclipped values, as on the device)
        self.flat.grad = flat_grad if self.clip is None else flat_grad * self.last_grad_norm[1]
        self.inner.step()
        self.flat.grad = None
        if self.ema is not None:
            with torch.no_grad():
                self._host_average()

    def _native_step(self, flat_grad, guard=None, flag=None):
        """The update as ONE bandwidth-bound launch of libebfi_hip.so (csrc/optim.hip, ebfi_optim_step) on the state tensors
        of the inner torch optimiser (which keeps owning hyper-parameters, state and checkpoint layout): every supported
        configuration on a CUDA float32 buffer, whatever param_groups says at this step.  Only CPU tensors take torch's own
        step."""
        from . import _native as N
        grp = self.inner.param_groups[0]
        if not (self.flat.is_cuda and self.flat.dtype == torch.float32 and flat_grad.dtype == torch.float32 and
                flat_grad.is_contiguous()):
            return False
        _refuse_group(self.name, grp)
        dev = self.flat.device
        st = self.inner.state[self.flat]
        zeros = lambda: torch.zeros_like(self.flat.data)
        b1 = b2 = eps = momentum = dampening = 0.0
        if self.name == "SGD":
            kind, flags = _OPTIM_SGD, _OPTIM_NESTEROV if grp["nesterov"] else 0
            momentum, dampening = float(grp["momentum"]), float(grp["dampening"])
            states, word = [None, None, None], None
            if momentum != 0.0:
                if self._sgd_step is None:                        # (a loaded momentum_buffer: the first step has been taken)
                    taken = st.get("momentum_buffer") is not None
                    self._sgd_step = torch.full((), 1.0 if taken else 0.0, dtype=torch.float32, device=dev)
                if st.get("momentum_buffer") is None:
                    st["momentum_buffer"] = zeros()
                states[0], word = st["momentum_buffer"], self._sgd_step
        else:
            kind = _OPTIM_ADAM
            flags = (_OPTIM_DECOUPLED_DECAY if grp.get("decoupled_weight_decay") else 0) | (_OPTIM_AMSGRAD if grp["amsgrad"] else 0)
            (b1, b2), eps = grp["betas"], grp["eps"]
            if "step" not in st:
                st["step"] = torch.zeros((), dtype=torch.float32, device=dev)
            if not (torch.is_tensor(st["step"]) and st["step"].is_cuda):
                st["step"] = torch.as_tensor(float(st["step"]), dtype=torch.float32, device=dev)
            for key in ("exp_avg", "exp_avg_sq") + (("max_exp_avg_sq",) if grp["amsgrad"] else ()):
                if key not in st:
                    st[key] = zeros()
            states, word = [st["exp_avg"], st["exp_avg_sq"], st.get("max_exp_avg_sq") if grp["amsgrad"] else None], st["step"]
        # the bookkeeping torch's own step() wrapper does: step hooks, and the marks the LR schedulers look at
        # (`_opt_called`: without it every scheduler.step() warns "lr_scheduler.step() before optimizer.step()")
        opt = self.inner
        for hook in list(getattr(opt, "_optimizer_step_pre_hooks", {}).values()):
            hook(opt, (), {})
        if word is not None:
            word += 1
        hyper = (float(grp["lr"]), float(b1), float(b2), float(eps), float(grp["weight_decay"]), momentum, dampening)
        if self.clip is None and self.ema is None:                # the default: the one launch it has always been
            with torch.cuda.device_of(self.flat):
                rc = N.lib().ebfi_optim_step(kind, flags, N.ptr(self.flat.data), N.ptr(flat_grad), N.ptr(states[0]), N.ptr(states[1]),
                                             N.ptr(states[2]), N.ptr(word), self.flat.numel(), *hyper, N.ptr(guard), N.ptr(flag),
                                             N.stream_ptr(dev))
            N.check(rc, "ebfi_optim_step")
        else:
            scale = None
            if self.clip is not None:
                self._native_norm(flat_grad)
                scale = self.last_grad_norm[1:2]
            decay, warmup = self.ema if self.ema is not None else (0.0, False)
            if self.ema is not None:
                self.ema_step += 1
            with torch.cuda.device_of(self.flat):
                rc = N.lib().ebfi_optim_step_ex(kind, flags, N.ptr(self.flat.data), N.ptr(flat_grad), N.ptr(states[0]),
                                                N.ptr(states[1]), N.ptr(states[2]), N.ptr(word), self.flat.numel(), *hyper,
                                                N.ptr(guard), N.ptr(flag), N.ptr(scale), N.ptr(self.ema_flat), N.ptr(self.ema_step),
                                                decay, int(warmup), N.stream_ptr(dev))
            N.check(rc, "ebfi_optim_step_ex")
        opt._opt_called = True
        if hasattr(opt, "_step_count"):
            opt._step_count += 1
        for hook in list(getattr(opt, "_optimizer_step_post_hooks", {}).values()):
            hook(opt, (), {})
        return True

    def views_intact(self):
        base = self.flat.untyped_storage().data_ptr()
        return all(p.untyped_storage().data_ptr() == base for p in self.params)

    def _slices(self):
        return [(i, p, slice(off, off + p.numel())) for i, (p, off) in enumerate(zip(self.params, self._offsets))]

    def state_dict(self):
        """torch's state_dict() of the class in question, per parameter.  Adam family: step, exp_avg, exp_avg_sq, and
        max_exp_avg_sq with amsgrad.  SGD: momentum_buffer once a step with momentum has been APPLIED (reads the device's
        step word: a checkpoint may synchronise), nothing before, nothing without momentum."""
        st = self.inner.state.get(self.flat, {})
        grp = self.inner.param_groups[0]
        state = {}
        if self.name == "SGD":
            buf = st.get("momentum_buffer")
            started = buf is not None and (self._sgd_step is None or float(self._sgd_step) > 0.0)
            if started and grp["momentum"] != 0:
                for i, p, sl in self._slices():
                    state[i] = {"momentum_buffer": buf[sl].view_as(p).clone()}
        elif st:
            keys = ("exp_avg", "exp_avg_sq") + (("max_exp_avg_sq",) if grp["amsgrad"] and "max_exp_avg_sq" in st else ())
            for i, p, sl in self._slices():
                state[i] = {"step": st["step"].clone() if torch.is_tensor(st["step"]) else st["step"]}
                state[i].update((k, st[k][sl].view_as(p).clone()) for k in keys)
        group = {k: v for k, v in grp.items() if k != "params"}
        group["lr"] = float(group["lr"])
        group["params"] = list(range(len(self.params)))
        return {"state": state, "param_groups": [group]}

    # param_group entries that describe HOW this process runs the update, not the optimisation state: a checkpoint written
    # by torch.optim.Adam (the reference's) carries fused=None / foreach=None, which would silently turn the single fused
    # launch into the per-tensor path with a host sync per step
    _LOCAL_KEYS = ("params", "fused", "foreach", "capturable", "differentiable")

    def load_state_dict(self, sd):
        """Accepts torch's per-parameter layout of the class (what the reference's checkpoints hold, train_ours.py:621-671);
        hyper-parameters of its param_groups override the constructor's, as in torch.
        Parameters without an entry (never received a gradient before the save), and a buffer the checkpoint does not
        carry (max_exp_avg_sq of an Adam checkpoint loaded into an AMSGrad run), start from zero.  All parameters
        share ONE step counter here (the update is one launch over the flat buffer, missing gradients count as zero), so
        the per-parameter steps of the checkpoint must agree -- they do whenever every parameter had a gradient on every
        step, which is the case for this model; a checkpoint whose steps differ (parameters frozen for part of the run) is
        refused instead of being silently re-timed.  SGD: a checkpoint that holds a momentum_buffer has taken its first step."""
        groups = sd["param_groups"]
        if len(groups) != 1 or len(groups[0]["params"]) != len(self.params):
            raise ValueError("optimizer state has %d parameters in %d group(s), this model trains %d"
                             % (sum(len(g["params"]) for g in groups), len(groups), len(self.params)))
        grp = self.inner.param_groups[0]
        for k, v in groups[0].items():
            if k not in self._LOCAL_KEYS and k in grp:
                grp[k] = v
        _refuse_group(self.name, grp)
        self._sgd_step = None
        if not sd["state"]:
            self.inner.state.pop(self.flat, None)
            return
        ids = groups[0]["params"]
        if self.name == "SGD":
            keys = ("momentum_buffer",)
        else:
            keys = ("exp_avg", "exp_avg_sq") + (("max_exp_avg_sq",) if grp["amsgrad"] else ())
        bufs = {k: torch.zeros_like(self.flat.data) for k in keys}
        step, found = None, False
        for pid, (_, p, sl) in zip(ids, self._slices()):
            e = sd["state"].get(pid)
            if e is None:
                continue
            for k in keys:
                if e.get(k) is not None:
                    bufs[k][sl] = e[k].reshape(-1).to(bufs[k])
                    found = True
            if self.name == "SGD":
                continue
            if step is not None and float(e["step"]) != step:
                raise ValueError("optimizer state holds different step counts per parameter (%g and %g): the flat %s keeps "
                                 "one counter for all parameters" % (step, float(e["step"]), self.name))
            step = float(e["step"])
        if self.name == "SGD":
            if found:
                self.inner.state[self.flat] = bufs
            else:
                self.inner.state.pop(self.flat, None)
            return
        step = 0.0 if step is None else step
        step = torch.tensor(step, dtype=torch.float32, device=self.flat.device if self.flat.is_cuda else "cpu")
        self.inner.state[self.flat] = dict(bufs, step=step)


def build_flat_optimizer(params, optimizer=None, lr=1e-4, betas=(0.9, 0.999), clip=None, ema=None):
    """The engines' optimiser: None -> FlatAdam(lr, betas), exactly what they have always built; otherwise the config's
    optimizer section {"name": ..., "args": {...}}, with the `lr=` / `betas=` keywords filling in what args leaves out
    (betas only where the class has them).  clip / ema: see FlatOptimizer (None, the default: neither)."""
    if optimizer is None:
        return FlatAdam(params, lr=lr, betas=tuple(betas), clip=clip, ema=ema)
    name = optimizer.get("name", "Adam")
    args = dict(optimizer.get("args") or {})
    args.setdefault("lr", lr)
    if name in ("Adam", "AdamW"):
        args.setdefault("betas", tuple(betas))
    return FlatOptimizer(params, name, clip=clip, ema=ema, **args)


class FlatAdam(FlatOptimizer):
    """torch.optim.Adam(params, lr, betas, eps) over one flat parameter buffer: FlatOptimizer with the defaults of the
    shipped configs (no weight decay, no AMSGrad)."""

    def __init__(self, params, lr=1e-4, betas=(0.9, 0.999), eps=1e-8, clip=None, ema=None):
        super().__init__(params, "Adam", clip=clip, ema=ema, lr=lr, betas=betas, eps=eps, amsgrad=False)
