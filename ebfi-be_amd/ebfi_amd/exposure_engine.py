"""Stage-1 engine: pre-training of ExposureDecision alone (reference train_ours_exposuredecision.py:229-259, :546-567).

The reference trains in two stages: this one fits ExposureDecision to the ground-truth exposure duty of the data set with
MSELoss(Ex, ExposureDuty); stage 2 (ebfi_amd.engine.Engine / train_ours.py) loads the result through
model.args.LoadPretrainEX / PretrainedEXPath and optionally freezes it (FrozenEX).

A step = blur-level map on the device -> ExposureDecision up to Conv1 -> duty head + MSE as ONE native node
(ebfi_amd.loss.DutyMSELoss, csrc/dutyhead.hip) -> backward -> gradient packing -> ONE flat all-reduce -> one Adam launch: the
optimiser path of the main engine (ebfi_amd.graphstep.GraphStepper over ebfi_amd.dp).  `Engine` itself is not involved.
"""
import torch

from .blur import Frame2DCP, Frame2Lap
from .dp import FlatGradBucket, broadcast_parameters, build_flat_optimizer
from .graphstep import GraphStepper
from .loss import DutyMSELoss, duty_head
from .model import ExposureDecision

# model.args of config/train_ours_exposuredecision.yml (the reference's shipped values)
DEFAULT_EXPOSURE_ARGS = dict(EventInch=32, BLInch=4, InterCH=64, Group=4, norm=None, activation="LeakyReLU")
BLURRY_FASHIONS = {"DarkCh": 1, "Lap": 1, "RGB": 3, "RGBDark": 4, "RGBLap": 4}      # fashion -> channels of the blur-level tensor
MODEL_NAMES = ("ExposureDecision",)


def check_model_name(name):
    """The reference's config comment lists two names; its script imports the second from a module that does not define it."""
    if name == "ExposureDecisionNoEvents":
        raise NotImplementedError("model.name 'ExposureDecisionNoEvents' is not defined by the reference either (its "
                                  "models/Ours/model_singleframe.py has no such class): use 'ExposureDecision'")
    if name not in MODEL_NAMES:
        raise ValueError("model.name must be 'ExposureDecision' for the stage-1 trainer, got %r" % (name,))
    return name


def check_fashion(fashion):
    if fashion not in BLURRY_FASHIONS:
        raise Exception("Wrong blurry convertion fashion!!")        # (the reference's message, train_ours_exposuredecision.py:247)
    return fashion


def blurry_level(frame, fashion):
    """The BlurryLevel tensor of train_ours_exposuredecision.py:233-247 for Frame [B, 3, H, W], built on the device."""
    check_fashion(fashion)
    if fashion == "DarkCh":
        return Frame2DCP(frame)
    if fashion == "Lap":
        return Frame2Lap(frame)
    if fashion == "RGB":
        return frame
    if fashion == "RGBDark":
        return torch.cat([frame, Frame2DCP(frame)], dim=1)
    return torch.cat([frame, Frame2Lap(frame)], dim=1)


def synthetic_exposure_batch(B, H, W, TB=16, exposure_time=(1, 2, 3, 4, 5, 6, 7, 8, 9, 10, 11, 12, 13, 14, 15),
                             num_frame_per_period=16, device="cuda", seed=123, rank=0, on_device=False):
    """(Frame [B,3,H,W], Event [B,TB,2,H,W], Duty [B,1]) with the statistics of `engine.synthetic_batch`: Frame in [0,1], Event =
    Poisson(0.35) counts; every sample's duty is one of exposure_time / num_frame_per_period (the dataset's ExposureMethod
    Custom).  For smoke and throughput runs: the inputs carry no information about the duty, nothing claims it is learnable.
    on_device: draw with the device generator (see `synthetic_batch`)."""
    dev = torch.device(device)
    times = torch.tensor([float(t) for t in exposure_time], dtype=torch.float32) / float(num_frame_per_period)
    if on_device and dev.type == "cuda":
        g = torch.Generator(device=dev).manual_seed(seed + rank)
        frame = torch.rand(B, 3, H, W, generator=g, device=dev)
        event = torch.poisson(torch.full((B, TB, 2, H, W), 0.35, device=dev), generator=g)
        pick = torch.randint(0, len(times), (B,), generator=g, device=dev)
        return frame, event, times.to(dev)[pick].reshape(B, 1)
    g = torch.Generator(device="cpu").manual_seed(seed + rank)
    frame = torch.rand(B, 3, H, W, generator=g)
    event = torch.poisson(torch.full((B, TB, 2, H, W), 0.35), generator=g)
    pick = torch.randint(0, len(times), (B,), generator=g)
    return tuple(v.to(device) for v in (frame, event, times[pick].reshape(B, 1)))


class ExposureEngine(GraphStepper):
    VALID_KEYS = ("valid_loss", "valid_mae")

    def __init__(self, model_args=None, fashion="RGBLap", device="cuda", precision="fp32", lr=1e-4, seed=None, graph=False,
                 accu_step=1, betas=(0.9, 0.999), strict_graph=None, name="ExposureDecision", optimizer=None, clip_grad=None,
                 ema=None):
        """precision: 'fp32' (exact) or 'bf16x3' (split-precision matrix-core operands, fp32-grade accuracy) for the 3x3
        convolutions; the fp16-operand backward of the main engine is not used here.  graph / accu_step / strict_graph: see
        graphstep.GraphStepper.  optimizer: None = Adam with `lr` / `betas`, or the config's optimizer section {"name", "args"}
        (see Engine).  clip_grad / ema: gradient clipping by total norm and the moving average of the weights, as in Engine."""
        check_model_name(name)
        if precision not in ("fp32", "bf16x3"):
            raise ValueError("precision must be 'fp32' or 'bf16x3'")
        self.fashion = check_fashion(fashion)
        # every period of a load is one micro-step on loss / accu_step; all-reduce and Adam on every accu_step-th (:252-259)
        super().__init__(device, graph=graph, accu_step=accu_step, strict_graph=strict_graph)
        self.precision = precision
        if seed is not None:
            torch.manual_seed(seed)
        self.model_args = dict(DEFAULT_EXPOSURE_ARGS, **(model_args or {}))
        if int(self.model_args["BLInch"]) != BLURRY_FASHIONS[fashion]:
            raise ValueError("model.args.BLInch = %r, but BlurryFashion %s gives %d channels"
                             % (self.model_args["BLInch"], fashion, BLURRY_FASHIONS[fashion]))
        self.model = ExposureDecision(**self.model_args).to(self.device)
        broadcast_parameters(self.model, 0)
        self.model.train()
        self.last_Ex = None
        self.loss = DutyMSELoss(1.0 / self.accu_step)
        self.bucket = FlatGradBucket(self.model)
        self.optimizer = build_flat_optimizer(self.bucket.params, optimizer, lr, betas, clip=clip_grad, ema=ema)
        self.bank = None
        if self.device.type == "cuda" and precision == "bf16x3":
            from . import weightbank
            self.bank = weightbank.build_for(self.model, flat=self.optimizer.flat.data, params=self.optimizer.params)

    def inputs(self, frame, event):
        """(Event viewed as [B, 2*TB, H, W], BlurryLevel) of one period."""
        event = event.reshape(event.size(0), -1, event.size(-2), event.size(-1))
        return event, blurry_level(frame, self.fashion)

    def _fwd_bwd(self, frame, event, duty):
        with self._autocast(), self._bank():
            ev, bl = self.inputs(frame, event)
            loss = self.loss(self.model.ex_map(ev, bl), duty)
            loss.backward()
        return loss.detach(), self.loss.Ex

    def _publish(self, out, static):
        """`last_Ex` holds the [B, 1] estimate of this call."""
        loss, ex = out
        self.last_Ex = ex.clone() if static else ex
        return loss.clone() if static else loss

    @torch.no_grad()
    def predict(self, frame, event):
        """Ex [B, 1] of one period in the engine's precision (module forward, current weights)."""
        with self._autocast(), self._bank():
            return self.model(*self.inputs(frame, event))

    @torch.no_grad()
    def validate(self, batch, load=0, refresh=True, use_ema=None):
        """One (batch, load) of the reference's _valid (train_ours_exposuredecision.py:546-567) -> {"valid_loss", "valid_mae"}:
        0-dim float64 DEVICE tensors.
          valid_loss  sum over the load's periods of MSELoss(Ex, ExposureDuty) -- the reference's value
          valid_mae   mean |Ex - ExposureDuty| over the load's B * NumP estimates
        batch: a collated ebfi_amd.clipdata batch (dict, [B, L, ...]; `load` picks the load) or the tuple (Frame [B,NumP,3,H,W] or
        [B,3,H,W], Event [B,TB,2,H,W], Duty [B,NumP,1] or [B,1]).  refresh: accepted for the call contract of Engine.validate
        (the weight images are re-packed from the current parameters on every call here: one launch).
        use_ema: score the moving average of the weights (`ema_weights()`); None = yes when the engine keeps one.
        Runs in eval mode; module modes, compute dtype, gradients, accumulation window and captured graphs are left as found."""
        if isinstance(batch, dict):
            frames = batch["SeqBlurryF"][:, load]
            event = batch["SeqHREv"][:, load]
            duties = batch["SeqExposureDuty"][:, load]
        else:
            frames, event, duties = batch
        if frames.dim() == 4:
            frames, duties = frames[:, None], duties[:, None]
        num_p = int(frames.shape[1])
        modes = [(m, m.training) for m in self.model.modules()]
        self.model.eval()
        try:
            loss = torch.zeros((), dtype=torch.float64, device=frames.device)
            mae = torch.zeros((), dtype=torch.float64, device=frames.device)
            with self._use_ema(use_ema), self._autocast(), self._bank():
                for i in range(num_p):
                    duty = duties[:, i].reshape(-1, 1).float()
                    # (Ex through the native head's loss-free form: two launches instead of the pooling / sigmoid tail)
                    ex = duty_head(self.model.ex_map(*self.inputs(frames[:, i].contiguous().float(), event.contiguous().float())))
                    diff = ex.double() - duty.double()
                    loss = loss + (diff * diff).mean()
                    mae = mae + diff.abs().mean()
        finally:
            for m, flag in modes:
                m.training = flag
        return {"valid_loss": loss, "valid_mae": mae / num_p}
