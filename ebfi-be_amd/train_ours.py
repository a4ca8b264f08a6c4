#!/usr/bin/env python3
"""train_ours.py -- MI355X counterpart of the reference entry point (train_ours.py:730-824).

Keeps what the hot path needs from the reference trainer: YAML config with `model.name/args`, `optimizer`,
`lr_scheduler`, `trainer.{accu_step, lr_min, iteration_based_train.*}`; one process per GPU (RANK / LOCAL_RANK /
WORLD_SIZE from torch.distributed.run), per-rank seeds (`seed + rank`, train_ours.py:737); the iteration body of
train_ours.py:250-347 in the reference's order -- forward -> Lap+census loss (0.1 weighting flips at 10k iterations,
divided by accu_step) -> backward -> every accu_step-th pass: Adam step, loss all-reduce for logging
(myutils/utils.py:80-92), periodic checkpoint, THEN lr_scheduler.step() (gated by lr_change_rate and lr_min, :335-338);
and the checkpoint layout {model:{name,states}, lr_scheduler:{name,states}, optimizer:{name,states}, config,
trainer:{training_mode, iteration, monitor_best}} (train_ours.py:621-671) with --resume / --reset as in
_resume_checkpoint (:673-716): training continues at trainer.iteration + 1.
Unlike the reference (whose fwd+bwd sits inside model.no_sync()) gradients ARE averaged across ranks every optimiser
step (one flat RCCL all-reduce).  Data: synthetic batches or, with --data, recorded clips through
ebfi_amd.clipdata (the tensor contract of dataloader/h5dataset.py:283-295 from .npz clips, or .h5 when h5py is installed).
Validation (trainer.do_validation, off unless the config switches it on) follows the reference's :309-333 / :392-435 / :545-619:
every valid_step-th iteration Engine.validate scores the validation set (valid_loss = the reference's Charbonnier sum,
valid_psnr, valid_ssim; recorded clips of valid_dataloader / --valid-data, or a fixed set of synthetic batches), `Monitor`
takes the best / early-stop decision of eval_model_performance, a best stamp writes checkpoint-iteration{it}.pth AND
model_best_until_iteration{it}.pth, and trainer.monitor_best travels through --resume.  Unlike the reference, every rank
holds the rank-averaged values and takes the same decision.  The reference's TensorBoard log (:283-319, :594-616) is written by
ebfi_amd.monitor into <output_path>/log/<experiment>/<runid>/ when trainer.tensorboard or --tensorboard asks for it (scalars;
images with trainer.vis.enabled; per-layer weight / gradient statistics with trainer.telemetry.stats_step); off by default.
The reference's perceptual_loss (train_ours.py:765; its net is the default of loss/restore.py:12, 'alex') is an optional term:
`--lpips_weight W` (or trainer.lpips_weight) with `--lpips_lin` / `--lpips_backbone` adds W x LPIPS(Sharp, target), mean over the
batch, to the loss above, differentiated by ebfi_amd.lpips on the device inside the (captured) step; the log line then names the
term.  `--lpips_net {vgg,alex}` (or trainer.lpips_net) selects the trunk: vgg by default, alex for the reference's own.  Off
(W = 0) by default.
The reference's 'GAN' entry (train_ours.py:767: Adversarial(PatchSize=<crop>, gan_type='STGAN')) is an optional term too:
`--gan_weight W` (or trainer.gan: {weight, type: STGAN}) adds W x the generator's loss under a spatio-temporal patch discriminator
that every pass also trains by its own Adamax step (ebfi_amd.gan), inside the (captured) step.  The crop is the PatchSize (square,
a multiple of 16); the option turns dataset.NeedNeighborGT on, so recorded clips deliver the neighbours of every latent frame, and
synthetic batches get two further seeded frames.  The log line shows this rank's `loss_d` (TensorBoard: `train_loss_d/train`),
read only at log steps, and checkpoints gain a key `gan` (discriminator and Adamax states) that --resume restores and --reset
does not; without the term checkpoints are what they were.  Off (W = 0) by default.
Two things the reference trains without, both off by default: `trainer.clip_grad: {max_norm, norm_type}` / `--clip-grad-norm X` clips
every optimiser step's gradient by its total norm (norm_type 2 or inf) inside the update's launch -- the log line then shows
grad_norm, the TensorBoard log `grad_norm/total` and `grad_norm/clip_coef` -- and `trainer.ema: {decay, warmup, validate}` /
`--ema-decay D` keeps an exponential moving average of the weights that validation, the monitor and the best checkpoint score
(validate: false keeps them on the raw iterate) and checkpoints carry as a sixth key, `ema: {decay, warmup, step, states}`, next to
an unchanged `model.states`; --resume restores it, --reset or a checkpoint without it starts it from the loaded weights, and
`infer_ours.py --ema` runs it.

    python -m torch.distributed.run --nproc-per-node 8 --master-addr 127.0.0.1 train_ours.py -c config/train_ours.yml -id run
    python train_ours.py -c config/train_ours.yml -id run --iterations 20
"""
import argparse
import contextlib
import math
import os
import sys
import time

import torch
import torch.distributed as dist
import yaml

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))

from ebfi_amd.dp import reduce_tensor  # noqa: E402
from ebfi_amd.engine import Engine, synthetic_batch, synthetic_batch_from_raw_events  # noqa: E402

TRAINING_MODE = "iteration_based_train"
CHECKPOINT_KEYS = ("model", "lr_scheduler", "optimizer", "config", "trainer")       # train_ours.py:628-644


def init_distributed_mode():
    if "RANK" in os.environ and "WORLD_SIZE" in os.environ:
        rank, world, gpu = int(os.environ["RANK"]), int(os.environ["WORLD_SIZE"]), int(os.environ["LOCAL_RANK"])
    else:
        rank, world, gpu = 0, 1, 0
    torch.cuda.set_device(gpu)
    if world > 1:
        os.environ.setdefault("MASTER_ADDR", "127.0.0.1")
        dist.init_process_group(backend="nccl", init_method="env://", world_size=world, rank=rank,
                                device_id=torch.device("cuda", gpu))
        dist.barrier()
    return rank, world, gpu


def build_lr_scheduler(config, optimizer):
    """`eval(config['lr_scheduler']['name'])(optimizer, **args)` of the reference (train_ours.py:760-761) for the schedulers
    of torch.optim.lr_scheduler; YAML floats such as `step_size: !!float 2e5` are made integral where torch expects it.
    No `lr_scheduler` section -> None.  An unknown name fails loudly instead of training without a schedule."""
    sec = config.get("lr_scheduler")
    if not sec or not sec.get("name"):
        return None
    cls = getattr(torch.optim.lr_scheduler, sec["name"], None)
    if cls is None:
        raise ValueError("lr_scheduler '%s' is not a torch.optim.lr_scheduler class" % sec["name"])
    args = dict(sec.get("args") or {})
    if "step_size" in args:
        args["step_size"] = int(args["step_size"])
    return cls(optimizer, **args)


def trainer_settings(config, cli_iterations=None):
    """iterations / save_period / lr_change_rate from trainer.iteration_based_train (reference layout, train_ours.yml:79-98)
    with the flat keys of this repo's small config as fallback; lr_min and accu_step from trainer."""
    tr = config.get("trainer", {}) or {}
    ib = tr.get("iteration_based_train", {}) or {}
    get = lambda k, d: ib.get(k, tr.get(k, d))
    return {"iterations": int(cli_iterations or float(get("iterations", 100))),
            "save_period": int(get("save_period", 0)),
            "lr_change_rate": max(1, int(get("lr_change_rate", 1))),
            "lr_min": float(tr.get("lr_min", 1e-6)),
            "accu_step": max(1, int(tr.get("accu_step", 1))),
            "log_step": max(1, int(get("train_log_step", 10)))}


def validation_settings(config, cli_valid_data=None):
    """The reference's validation keys (train_ours.yml:86-100, :151-192); every absent key means OFF / the reference's default.
    valid_data: --valid-data, else valid_dataloader.path_to_datalist_txt; None -> `valid_batches` fixed synthetic batches."""
    tr = config.get("trainer", {}) or {}
    ib = tr.get("iteration_based_train", {}) or {}
    vd = config.get("valid_dataloader") or {}
    get = lambda k, d: ib.get(k, tr.get(k, d))
    early = tr.get("early_stop", math.inf)
    return {"do_validation": bool(tr.get("do_validation", False)),
            "valid_step": max(1, int(float(get("valid_step", 5000)))),
            "valid_log_step": max(1, int(float(get("valid_log_step", 50)))),
            "monitor": str(tr.get("monitor", "off")),
            "early_stop": math.inf if early is None else float(early),
            "valid_batches": max(1, int(tr.get("valid_batches", 2))),
            "valid_data": cli_valid_data or vd.get("path_to_datalist_txt"),
            "batch_size": None if vd.get("batch_size") is None else int(vd["batch_size"]),
            "drop_last": bool(vd.get("drop_last", False)),
            "dataset": vd.get("dataset") or {}}


LPIPS_FILES = {"vgg": ("the v0.1 vgg.pth heads", "torchvision's VGG-16 state dict, vgg16-397923af.pth"),
               "alex": ("the v0.1 alex.pth heads", "torchvision's AlexNet state dict, alexnet-owt-7be5be79.pth")}


def perceptual_net(config, args):
    """The trunk of the LPIPS term: --lpips_net, else trainer.lpips_net, else 'vgg'.  Any other name ends the run."""
    tr = config.get("trainer", {}) or {}
    flag = getattr(args, "lpips_net", None)
    net = str(tr.get("lpips_net", "vgg") if flag is None else flag)
    if net not in LPIPS_FILES:
        raise SystemExit("train_ours.py: --lpips_net / trainer.lpips_net must be one of %s, got %r"
                         % (", ".join(sorted(LPIPS_FILES)), net))
    return net


def perceptual_settings(config, args):
    """(weight, lin_path, backbone_path) of the LPIPS term of the training loss: --lpips_weight, else trainer.lpips_weight,
    else 0 = off.  A positive weight without both weight files ends the run: no weight cache is searched.  (The trunk is
    perceptual_net's.)"""
    tr = config.get("trainer", {}) or {}
    weight = float(tr.get("lpips_weight", 0.0) if args.lpips_weight is None else args.lpips_weight)
    if weight < 0:
        raise SystemExit("train_ours.py: --lpips_weight / trainer.lpips_weight must not be negative, got %g" % weight)
    heads, trunk = LPIPS_FILES[perceptual_net(config, args)]
    if weight > 0 and (args.lpips_lin is None or args.lpips_backbone is None):
        missing = " and ".join(f for f, v in (("--lpips_lin", args.lpips_lin), ("--lpips_backbone", args.lpips_backbone)) if v is None)
        raise SystemExit("train_ours.py: an LPIPS weight of %g needs both weight files: --lpips_lin (%s) and "
                         "--lpips_backbone (%s); missing %s" % (weight, heads, trunk, missing))
    return weight, args.lpips_lin, args.lpips_backbone


def perceptual_term(net, lin_path, backbone_path, weight, device):
    """(PerceptualTerm, the log line's note) of a positive weight: VggLPIPS, or AlexLPIPSLoss for net = 'alex'."""
    from ebfi_amd.loss import PerceptualTerm
    from ebfi_amd.lpips import load_alex_lpips, load_vgg_lpips
    if net == "alex":
        model = load_alex_lpips(lin_path, backbone_path, device=device, train=True)
    else:
        model = load_vgg_lpips(lin_path, backbone_path, device=device)
    return PerceptualTerm(model, weight), " (with %g x lpips_%s)" % (weight, net)


def adversarial_settings(config, args):
    """(weight, gan_type) of the STGAN adversarial term (the reference's 'GAN': Adversarial(PatchSize=<crop>, gan_type='STGAN'),
    train_ours.py:767): --gan_weight, else trainer.gan.weight, else 0 = off; the type is trainer.gan.type, 'STGAN' by default and
    the only one implemented.  With the term on the crop (trainer.height x trainer.width) is the discriminator's PatchSize: square
    and a multiple of 16.  Anything else ends the run before any device work."""
    tr = config.get("trainer", {}) or {}
    gan = tr.get("gan") or {}
    flag = getattr(args, "gan_weight", None)
    weight = float(gan.get("weight", 0.0) if flag is None else flag)
    gan_type = str(gan.get("type", "STGAN"))
    if weight < 0:
        raise SystemExit("train_ours.py: --gan_weight / trainer.gan.weight must not be negative, got %g" % weight)
    if weight > 0:
        from ebfi_amd.gan import GAN_TYPES
        if gan_type not in GAN_TYPES:
            raise SystemExit("train_ours.py: trainer.gan.type must be one of %s, got %r" % (", ".join(GAN_TYPES), gan_type))
        H, W = int(tr.get("height", 256)), int(tr.get("width", 256))
        if H != W or H % 16:
            raise SystemExit("train_ours.py: the adversarial term needs a square crop whose side is a multiple of 16 (the "
                             "discriminator's PatchSize), got %d x %d" % (H, W))
    return weight, gan_type


def adversarial_term(patch, gan_type, weight, seed):
    """-> (AdversarialTerm, the log line's note).  The discriminator is initialised from `seed`, identically on every rank."""
    from ebfi_amd.gan import Adversarial, AdversarialTerm
    state = torch.random.get_rng_state()
    torch.manual_seed(int(seed) + 4099)
    try:
        adv = Adversarial(patch, gan_type)
    finally:
        torch.random.set_rng_state(state)                  # (the model's initialisation draws what it drew without the term)
    return AdversarialTerm(adv, weight), " (with %g x %s)" % (weight, gan_type)


def with_neighbours(batch, seed, on_device):
    """A synthetic batch plus two further seeded frames per sample as the neighbours [B, 2, 3, H, W]."""
    target = batch[4]
    dev = target.device if on_device else torch.device("cpu")
    g = torch.Generator(device=dev).manual_seed(int(seed) + 31337)
    nb = torch.rand((target.shape[0], 2) + tuple(target.shape[1:]), generator=g, device=dev)
    return tuple(batch) + (nb.to(target.device),)


def averaging_settings(config, args=None):
    """{"clip_grad": (max_norm, norm_type) | None, "ema": (decay, warmup) | None, "ema_validate": bool} from trainer.clip_grad
    {max_norm, norm_type = 2} and trainer.ema {decay, warmup = false, validate = true}; --clip-grad-norm X and --ema-decay D
    override max_norm and decay (and switch the feature on where the config is silent).  Absent: off.  max_norm <= 0, a
    norm_type other than 2 / inf, a decay outside [0, 1) or an unknown key raise ValueError here, before any device work."""
    from ebfi_amd.dp import clip_arguments, ema_arguments
    tr = config.get("trainer", {}) or {}
    clip, ema = tr.get("clip_grad"), tr.get("ema")
    clip = dict(clip) if isinstance(clip, dict) else (None if clip is None else {"max_norm": clip})
    ema = dict(ema) if isinstance(ema, dict) else (None if ema is None else {"decay": ema})
    if getattr(args, "clip_grad_norm", None) is not None:
        clip = dict(clip or {}, max_norm=args.clip_grad_norm)
    if getattr(args, "ema_decay", None) is not None:
        ema = dict(ema or {}, decay=args.ema_decay)
    validate = True
    if ema is not None:
        unknown = set(ema) - {"decay", "warmup", "validate"}
        if unknown:
            raise ValueError("trainer.ema takes decay, warmup and validate, got %r" % (sorted(ema),))
        validate = bool(ema.pop("validate", True))
    if clip is not None and isinstance(clip.get("norm_type"), str):
        clip["norm_type"] = float(clip["norm_type"])              # (YAML spells infinity `.inf`; 'inf' is accepted too)
    return {"clip_grad": clip_arguments(clip), "ema": ema_arguments(ema), "ema_validate": validate}


def add_averaging_arguments(ap):
    """--clip-grad-norm / --ema-decay of both trainers."""
    ap.add_argument("--clip-grad-norm", dest="clip_grad_norm", type=float, default=None,
                    help="clip every optimiser step's gradient to this total norm (trainer.clip_grad.max_norm; the norm type comes "
                         "from trainer.clip_grad.norm_type, 2 by default) inside the update's launch; default: the config's, else off")
    ap.add_argument("--ema-decay", dest="ema_decay", type=float, default=None,
                    help="keep an exponential moving average of the weights with this decay (trainer.ema.decay) for validation, "
                         "best-model tracking, checkpoints (`ema` key) and infer_ours.py --ema; default: the config's, else off")


def optimizer_settings(config, args=None):
    """{"name", "args"} of the optimiser from the config's `optimizer` section, the reference's
    eval(config['optimizer']['name'])(trainable_params, **config['optimizer']['args']) (train_ours.py:770-771): Adam, AdamW or
    SGD with all of optimizer.args (weight_decay, eps, amsgrad, momentum, ...; torch's defaults where the section is silent,
    except lr: 1e-4 as it has always been here).  -lr / --learning_rate (stage 1) overrides args.lr.  Anything the native update does not implement -- another optimiser,
    maximize, an argument the torch class does not know -- raises ValueError here, before any device work."""
    from ebfi_amd.dp import optimizer_arguments
    sec = config.get("optimizer") or {}
    name = sec.get("name", "Adam")
    oargs = dict(sec.get("args") or {})
    if getattr(args, "learning_rate", None):
        oargs["lr"] = float(args.learning_rate)
    oargs["lr"] = float(oargs.get("lr", 1e-4))
    return {"name": name, "args": optimizer_arguments(name, oargs)}


class Monitor:
    """eval_model_performance of the reference (train_ours.py:155-163, :392-435), host-only.  monitor: 'off' or '<min|max> <key>'.
    `evaluate(log)` -> (stop_training, best): improved means <= / >= the best so far (a tie counts), a missing key warns and
    leaves every counter alone, training stops once not_improved_count > early_stop.  `best` starts at +inf / -inf; with
    monitor 'off' it is None and evaluate never reports a best or a stop (checkpoints then carry monitor_best None)."""

    def __init__(self, monitor="off", early_stop=math.inf, warn=None):
        self.monitor = monitor or "off"
        self.warn = warn or (lambda msg: print(msg, file=sys.stderr, flush=True))
        self.not_improved_count = 0
        if self.monitor == "off":
            self.mode, self.metric, self.best, self.early_stop = "off", None, None, math.inf
            return
        parts = self.monitor.split()
        if len(parts) != 2 or parts[0] not in ("min", "max"):
            raise ValueError("trainer.monitor must be 'off' or '<min|max> <key>', got %r" % (monitor,))
        self.mode, self.metric = parts
        self.best = math.inf if self.mode == "min" else -math.inf
        self.early_stop = math.inf if early_stop is None else float(early_stop)

    def evaluate(self, log):
        if self.mode == "off":
            return False, False
        best = False
        if self.metric not in log:
            self.warn("Warning: Metric '%s' is not found. Ignore this stamp where using this metric to monitor." % self.metric)
        else:
            value = log[self.metric]
            if (self.mode == "min" and value <= self.best) or (self.mode == "max" and value >= self.best):
                self.best, self.not_improved_count, best = value, 0, True
            else:
                self.not_improved_count += 1
        return self.not_improved_count > self.early_stop, best

    def stop_message(self):
        return "Validation performance didn't improve for %s stamps. Training stops." % _fmt_count(self.early_stop)


def _fmt_count(v):
    return "%d" % v if math.isfinite(v) and float(v).is_integer() else "%s" % v


def validation_seeds(seed, count):
    """Seeds of the synthetic validation batches: seed - 1, seed - 2, ...  Every training batch is drawn from
    seed + 1000 * pass + rank >= seed (main loop), so the two sets cannot meet."""
    return [int(seed) - 1 - j for j in range(int(count))]


def best_checkpoint_name(iteration):
    return "model_best_until_iteration%d.pth" % int(iteration)      # train_ours.py:669


def checkpoint_state(eng, scheduler, config, iteration, monitor_best=None):
    """The reference's checkpoint dict (train_ours.py:628-655), key for key; `iteration` = index of the last completed
    optimiser step, resumed at +1 (:695)."""
    sched_name = (config.get("lr_scheduler") or {}).get("name")
    ema = eng.ema_state() if getattr(eng, "has_ema", False) else None
    extra = {} if ema is None else {"ema": ema}       # (a sixth key only when the run keeps an average: model.states stays raw)
    if getattr(eng, "adversarial", None) is not None:   # (likewise `gan`, only with the adversarial term on: the discriminator's
        extra["gan"] = eng.adversarial.checkpoint_state()   # states and its Adamax states in torch's per-parameter layout)
    return dict({"model": {"name": config["model"]["name"], "states": eng.model.state_dict()},
            "lr_scheduler": {"name": sched_name, "states": scheduler.state_dict() if scheduler is not None else {}},
            "optimizer": {"name": config["optimizer"]["name"], "states": eng.optimizer.state_dict()},
            "config": config,
            "trainer": {"training_mode": TRAINING_MODE, "iteration": int(iteration), "monitor_best": monitor_best}}, **extra)


def save_checkpoint(path, eng, scheduler, config, iteration, monitor_best=None, save_best=False):
    """checkpoint-iteration{it}.pth at `path`; save_best: the same state again as model_best_until_iteration{it}.pth beside it
    (train_ours.py:665-671).  Returns the paths written."""
    os.makedirs(os.path.dirname(path), exist_ok=True)
    state = checkpoint_state(eng, scheduler, config, iteration, monitor_best)
    paths = [path] + ([os.path.join(os.path.dirname(path), best_checkpoint_name(iteration))] if save_best else [])
    for p in paths:
        torch.save(state, p)
    return paths


def resume_checkpoint(path, eng, scheduler, config, reset=False, map_location="cpu", monitor=None):
    """Resumer + _resume_checkpoint of the reference (myutils/utils.py:178-215, train_ours.py:673-716): optimiser and
    scheduler states are restored only without --reset and when the training mode matches, each only when the configured
    name equals the checkpoint's; the model is always loaded (strict=False) when its name matches.  monitor: a Monitor whose
    `best` is restored from trainer.monitor_best under the same condition as the optimiser state, and so is the discriminator of
    an engine with the adversarial term from the checkpoint's `gan` entry (:696; a checkpoint written
    without validation carries None and leaves it alone); its not_improved_count restarts at 0.  An engine that keeps a moving
    average of the weights takes it from the checkpoint's `ema` entry under that condition too; with --reset, another training
    mode or a checkpoint without the entry the average starts from the loaded weights.  Returns the first iteration to run."""
    cpt = torch.load(path, map_location=map_location, weights_only=False)
    start = 0
    ema = None
    tr = cpt["trainer"]
    if not reset and tr.get("training_mode") == TRAINING_MODE and getattr(eng, "adversarial", None) is not None \
            and cpt.get("gan") is not None:
        eng.adversarial.load_checkpoint_state(cpt["gan"])    # (--reset, or a checkpoint without the key: a fresh discriminator)
    if not reset and tr.get("training_mode") == TRAINING_MODE:
        if config["optimizer"]["name"] == cpt["optimizer"]["name"]:
            eng.optimizer.load_state_dict(cpt["optimizer"]["states"])
        if scheduler is not None and (config.get("lr_scheduler") or {}).get("name") == cpt["lr_scheduler"]["name"]:
            scheduler.load_state_dict(cpt["lr_scheduler"]["states"])
            for group, lr in zip(eng.optimizer.param_groups, scheduler.get_last_lr()):
                group["lr"] = lr
        start = int(tr["iteration"]) + 1
        ema = cpt.get("ema")
        if monitor is not None and monitor.mode != "off" and tr.get("monitor_best") is not None:
            monitor.best = tr["monitor_best"]
    if config["model"]["name"] == cpt["model"]["name"]:
        eng.model.load_state_dict(cpt["model"]["states"], strict=False)
    if getattr(eng, "has_ema", False):
        eng.load_ema_state(ema if config["model"]["name"] == cpt["model"]["name"] else None)
    eng.iteration = start
    return start


def add_loader_arguments(ap):
    """--loader / --prefetch / --event-noise / --hot-pixels of the recorded-clip readers (train_ours.py and
    train_ours_exposuredecision.py); they apply to the training and the validation set alike."""
    ap.add_argument("--loader", default="device", choices=["device", "host"],
                    help="recorded clips: 'device' uploads the crop window's rows as uint8 and makes the sharp planes and the "
                         "blurry mean in one kernel; 'host' converts and averages whole frames on the host.  The tensors are "
                         "bit-identical")
    ap.add_argument("--prefetch", type=int, default=1,
                    help="recorded clips: batches whose host half (file reads, staging, noise draw) a worker thread prepares "
                         "ahead while the current batch trains; 0 = everything synchronously in the training loop")
    ap.add_argument("--event-noise", dest="event_noise", default="host", choices=["host", "device"],
                    help="recorded clips, data_augment.noise: 'host' draws the event noise as the reference does, bit for bit, on "
                         "one host thread; 'device' draws a counter-based law of the same distribution in the kernel that cuts "
                         "and flips the event stack (ebfi_amd.eventaug) -- other bits, no host work")
    ap.add_argument("--hot-pixels", dest="hot_pixels", action="store_true",
                    help="recorded clips: honour data_augment.hot_pixel (the reference's own guard never lets it run); needs "
                         "--event-noise device")


def add_monitor_arguments(ap):
    """--tensorboard / --no-tensorboard of both trainers: override trainer.tensorboard of the config."""
    ap.add_argument("--tensorboard", dest="tensorboard", action="store_true", default=None,
                    help="write a TensorBoard event file (ebfi_amd.monitor) into <output_path>/log/<experiment>/<runid>/ whatever "
                         "trainer.tensorboard says: scalars, images with trainer.vis.enabled, per-layer statistics with "
                         "trainer.telemetry.stats_step")
    ap.add_argument("--no-tensorboard", dest="tensorboard", action="store_false",
                    help="write no event file whatever trainer.tensorboard says")


def build_monitor(config, args, runid, rank, eng, default_experiment="Ours"):
    """The run's ebfi_amd.monitor.TrainMonitor, attached to the engine, or None when neither the config nor the flag asks for one
    (nothing of ebfi_amd.monitor is imported then)."""
    tr = config.get("trainer", {}) or {}
    on = bool(tr.get("tensorboard", False)) if getattr(args, "tensorboard", None) is None else bool(args.tensorboard)
    if not on:
        return None
    from ebfi_amd import monitor as M
    return M.TrainMonitor(M.monitor_settings(config, on), M.log_directory(config, runid, default_experiment), rank=rank).attach(eng)


DEFAULT_EXPOSURE_TIME = [9, 10, 11, 12, 13, 14, 15]      # ExposureTime of the reference's train_ours.yml (Custom exposure)


def with_noise_law(ds_cfg, event_noise="host", hot_pixels=False):
    """A copy of a dataset section carrying the flags --event-noise / --hot-pixels as the keys `event_noise` and `hot_pixels`
    that `clip_dataset` reads (the flags decide; a section may also name them itself)."""
    return dict(ds_cfg, event_noise=event_noise, hot_pixels=bool(hot_pixels))


def clip_dataset(path, ds_cfg, time_bins, default_exposure_time, device, seed, loader):
    """The recorded-clip dataset of both trainers, for training and validation alike: `ds_cfg` is a dataset section of the config
    with the reference's keys (train_ours.yml:115-150); absent keys take its shipped values, `time_bins` and
    `default_exposure_time` being the calling script's.  Two keys are this project's: `event_noise` ('host', the default, or
    'device') names the noise law and `hot_pixels` (default false) honours data_augment.hot_pixel (`with_noise_law`)."""
    from ebfi_amd import clipdata
    return clipdata.ClipDataset(path, time_bins=int(ds_cfg.get("time_bins", time_bins)),
                                frames_per_period=int(ds_cfg.get("NumFramePerPeriod", 16)),
                                frames_per_blurry=int(ds_cfg.get("NumFramePerBlurry", 16)),
                                exposure_method=ds_cfg.get("ExposureMethod", "Custom"),
                                exposure_time=ds_cfg.get("ExposureTime", default_exposure_time),
                                device=device, seed=seed, frames=loader, noise_mode=ds_cfg.get("event_noise", "host"),
                                **clipdata.dataset_args_from_config(ds_cfg, hot_pixels=bool(ds_cfg.get("hot_pixels", False))))


def real_data_passes(path, config, B, TB, device, rank, world, seed, loader="device", prefetch=1, event_noise="host",
                     hot_pixels=False):
    """Endless stream of (Frame, Event, T, GTEx, LatentF) passes from recorded clips (ebfi_amd.clipdata): the dataset keys
    are the reference's (config train_dataloader.dataset, train_ours.yml:115-150); defaults = its shipped values."""
    from ebfi_amd import clipdata
    ds_cfg = with_noise_law((config.get("train_dataloader") or {}).get("dataset") or {}, event_noise, hot_pixels)
    ds = clip_dataset(path, ds_cfg, TB, DEFAULT_EXPOSURE_TIME, device, seed, loader)
    if len(ds) < B * world:
        raise SystemExit("--data: %d periods in %s, need at least batch_size x world = %d" % (len(ds), path, B * world))
    for batch in clipdata.batches(ds, B, rank=rank, world=world, seed=seed, prefetch=prefetch):
        for inputs in clipdata.model_inputs(batch):
            yield inputs


def validation_batches(vs, config, args, B, H, W, TB, device, rank, world):
    """-> a function that yields this rank's validation batches, the same ones at every stamp, sharded so that every rank gets
    the same count (clipdata.shard_indices).  Recorded clips go through clipdata with the valid_dataloader.dataset section
    (reference keys); without a path: `valid_batches` synthetic periods, made once and kept on the device."""
    from ebfi_amd import clipdata
    from ebfi_amd.engine import synthetic_validation_batch
    ds_cfg = with_noise_law(vs["dataset"], args.event_noise, args.hot_pixels)
    vb = vs["batch_size"] or B
    if vs["valid_data"]:
        ds = clip_dataset(vs["valid_data"], ds_cfg, TB, DEFAULT_EXPOSURE_TIME, device, args.seed, args.loader)
        if len(ds) == 0:
            raise SystemExit("--valid-data: no complete period in %s" % vs["valid_data"])
        return lambda: clipdata.eval_batches(ds, vb, rank=rank, world=world, seed=args.seed, drop_last=vs["drop_last"],
                                             prefetch=args.prefetch)
    seeds = validation_seeds(args.seed, vs["valid_batches"])
    num_f = int(ds_cfg.get("NumFramePerPeriod", 4))
    mine = [synthetic_validation_batch(vb, H, W, TB, num_f, device=device, seed=seeds[j])
            for j in clipdata.shard_indices(len(seeds), rank, world)]
    return lambda: iter(mine)


def run_validation(eng, batches, tracker, stamp, log_step=50, rank=0, telemetry=None, use_ema=None):
    """_valid of the reference (train_ours.py:545-619) for one stamp: every (batch, load) is scored by Engine.validate, averaged
    over ranks (reduce_tensor: ONE collective and ONE host read per (batch, load), none per timestamp) and averaged over the
    stamp by the MetricTracker.  Every rank feeds its tracker with the same reduced values.  Returns tracker.result().
    telemetry: an ebfi_amd.monitor.TrainMonitor that logs every (batch, load), or None.
    use_ema (an engine that keeps a moving average of the weights; trainer.ema.validate): None / True score the average -- the
    whole stamp runs inside ONE eng.ema_weights() -- False the raw iterate."""
    tracker.reset()
    has_ema = bool(getattr(eng, "has_ema", False))
    averaged = has_ema and (use_ema is None or bool(use_ema))
    kw = {"use_ema": False} if has_ema and not averaged else {}
    with (eng.ema_weights() if averaged else contextlib.nullcontext()):
        for k, batch in enumerate(batches()):
            loads = batch["SeqLatentF"].shape[1] if isinstance(batch, dict) else 1
            for load in range(loads):
                vals = eng.validate(batch, load=load, refresh=(k == 0 and load == 0), **kw)      # weights re-packed once per pass
                host = reduce_tensor(torch.stack([vals[key] for key in eng.VALID_KEYS])).tolist()
                for key, v in zip(eng.VALID_KEYS, host):
                    tracker.update(key, v)
                if telemetry is not None:
                    telemetry.valid_batch(host[0], eng)
                if rank == 0 and k % log_step == 0:
                    print("Valid timestamp: %d [batch %d] valid_loss: %.4e" % (stamp, k, host[0]), flush=True)
    return tracker.result()


def train_loop(eng, next_micro_batch, samples_per_pass, unit, st, vs, scheduler, monitor, valid_batches, tracker, out_dir, config,
               rank, world, start, loss_note="", telemetry=None):
    """The iteration body of both trainers, from iteration `start` on: accu_step passes on `next_micro_batch(it, micro)`, log,
    validate, monitor, checkpoint, early stop, scheduler gate.  samples_per_pass / unit: what one pass of one rank adds to the
    logged rate and the word it is logged under ('frames' -> frames/s); loss_note: what the log line says after the loss value
    (the terms it holds beyond the reference's).  telemetry: an ebfi_amd.monitor.TrainMonitor (one per rank) or None; None leaves
    every line below as it runs without one.  Returns the iteration count it ended at."""
    # throughput is counted from the end of the first iteration after which the engine is in its steady state (the first ones
    # pay module load, allocator growth, the just-in-time calibration of the fp16 operand scales and, with --graph, the
    # capture: GraphStepper.settled): what is logged is the steady-state rate, whole job (all ranks)
    t0, samples, it, valid_stamp = None, 0, start, 1
    while it < st["iterations"]:
        for micro in range(st["accu_step"]):
            batch = next_micro_batch(it, micro)
            loss = eng.train_step(*batch)
            if t0 is not None:
                samples += samples_per_pass * world
        log_now = it % st["log_step"] == 0 or it == st["iterations"] - 1
        lr_now = scheduler.get_last_lr()[0] if scheduler is not None else eng.optimizer.param_groups[0]["lr"]
        if telemetry is not None:
            telemetry.after_step(it, loss, lr_now, eng, batch)
            if log_now:                  # (the monitor's ring holds this iteration's loss: its flush is the log line's all-reduce)
                loss = torch.tensor(telemetry.flush())
        elif log_now:                    # the loss all-reduce is for logging only (train_ours.py:278-279): do it when logging
            loss = reduce_tensor(loss.clone())
        if rank == 0 and log_now:
            torch.cuda.synchronize()
            rate = samples / (time.perf_counter() - t0) if t0 is not None and samples else float("nan")
            # with clipping on: the total norm of this iteration's gradient, from the monitor's second ring (its flush just
            # downloaded it) or, without a monitor, read here -- at the log step only, after the synchronisation above
            norm_note, norm = "", getattr(getattr(eng, "optimizer", None), "last_grad_norm", None)
            if norm is not None:
                shown = telemetry.last_grad_norm[0] if telemetry is not None and telemetry.last_grad_norm else float(norm[0])
                norm_note = " grad_norm: %.4e" % shown
            # with the adversarial term: this rank's discriminator loss of the iteration's last pass, read here only
            adv = getattr(eng, "adversarial", None)
            if adv is not None:
                loss_d = float(adv.loss_d)
                norm_note += " loss_d: %.4e" % loss_d
                if telemetry is not None:
                    telemetry.scalar("train_loss_d/train", loss_d, it)
            print("Iteration: %d/%d train_loss: %.4e%s%s learning rate: %.4e  %.1f %s/s"
                  % (it, st["iterations"], loss.item(), loss_note, norm_note, lr_now, rate, unit), flush=True)
        if t0 is None and eng.settled:
            torch.cuda.synchronize()
            t0 = time.perf_counter()
        # validation every valid_step-th iteration, never at 0 (train_ours.py:309-328); all ranks take part and decide alike
        best = stop = False
        if vs["do_validation"] and it % vs["valid_step"] == 0 and it != 0:
            t_valid = time.perf_counter()
            val_log = run_validation(eng, valid_batches, tracker, valid_stamp, vs["valid_log_step"], rank, telemetry=telemetry,
                                     use_ema=vs.get("use_ema"))
            if telemetry is not None:
                telemetry.stamp(valid_stamp, val_log)
                telemetry.pause(time.perf_counter() - t_valid)
            if t0 is not None:           # (the logged rate is the training rate: the stamp's time is taken off the clock)
                t0 += time.perf_counter() - t_valid
            stop, best = monitor.evaluate(val_log)
            if rank == 0:
                print("Valid stamp: %d %s (best %r)" % (valid_stamp, " ".join("%s: %.6e" % (k, val_log[k]) for k in eng.VALID_KEYS),
                                                        monitor.best), flush=True)
                if stop:
                    print(monitor.stop_message(), flush=True)
            valid_stamp += 1
        # periodic checkpoints as train_ours.py:331-333 (saved BEFORE this iteration's scheduler step, like there; also when this
        # stamp is the best so far, then twice: :665-671), plus one after the last iteration -- the one an early stop ends at too
        if rank == 0 and ((st["save_period"] and it % st["save_period"] == 0 and it != 0) or best or stop
                          or it == st["iterations"] - 1):
            path = os.path.join(out_dir, "checkpoint-iteration%d.pth" % it)
            for p in save_checkpoint(path, eng, scheduler, config, it, monitor.best if monitor is not None else None, best):
                print("saved", p, flush=True)
        if stop:
            it += 1
            break
        if scheduler is not None and it % st["lr_change_rate"] == 0 and it != 0 and lr_now >= st["lr_min"]:   # :335-338
            scheduler.step()
        it += 1
    return it


def get_args(argv=None):
    ap = argparse.ArgumentParser()
    ap.add_argument("-c", "--config", default=os.path.join(os.path.dirname(os.path.abspath(__file__)), "config", "train_ours.yml"))
    ap.add_argument("-id", "--runid", default="run")
    ap.add_argument("-r", "--resume", default=None, help="checkpoint to resume from")
    ap.add_argument("--reset", action="store_true", help="with --resume: load the model only, restart optimiser / schedule / count")
    ap.add_argument("-seed", "--seed", type=int, default=123)
    ap.add_argument("--iterations", type=int, default=None)
    ap.add_argument("--precision", default="bf16x3", choices=["fp32", "bf16x3", "bf16"],
                    help="matrix-core operands of the convs: bf16x3 = split bf16 pairs, fp32-grade accuracy (default); fp32 = exact")
    ap.add_argument("--graph", action="store_true", help="replay forward+loss+backward from a captured hipGraph")
    ap.add_argument("--host-data", action="store_true",
                    help="draw every synthetic batch on the host (bit-identical across machines, ~0.5 s per B=8 256x256 batch) "
                         "instead of with the device generator (default: the data path must not be slower than the 20 ms step)")
    ap.add_argument("--no-f16-backward", action="store_true",
                    help="bf16x3 precision: keep the data / weight gradients on the split-precision kernels (3 MFMAs per product) "
                         "instead of the fp16 single-product ones with delayed operand scales (ebfi_amd.f16scale)")
    ap.add_argument("--no-f16-forward", action="store_true",
                    help="keep the 128 -> 1600 KernelConv of Modification on the split-precision kernel in the forward pass "
                         "(default with the fp16 backward: fp16 operands, Engine(forward_f16='filters'))")
    ap.add_argument("--data", default=None,
                    help="recorded clips instead of synthetic batches: a directory of .npz clips (or .h5 in the reference's layout "
                         "when h5py is installed), a datalist .txt, or one clip file (ebfi_amd.clipdata); the dataset section of "
                         "the config (train_dataloader.dataset, reference keys) sets periods / exposure / crop")
    ap.add_argument("--valid-data", default=None,
                    help="validation clips (same forms as --data) instead of valid_dataloader.path_to_datalist_txt; used when "
                         "trainer.do_validation is on (without either: a fixed set of trainer.valid_batches synthetic batches)")
    ap.add_argument("--raw-events", action="store_true",
                    help="build the event tensor from synthetic raw event lists with the device events_to_stack kernel "
                         "(the reference's data path, h5dataset.py:327-352) instead of drawing voxel counts directly")
    ap.add_argument("--lpips_weight", type=float, default=None,
                    help="add W x LPIPS (v0.1; the reference's perceptual_loss) of the restored frame to the "
                         "training loss, differentiated on the device (default: trainer.lpips_weight of the config, else 0 = off); "
                         "needs --lpips_lin and --lpips_backbone")
    ap.add_argument("--gan_weight", type=float, default=None,
                    help="add W x the generator's loss of the STGAN adversarial term (the reference's 'GAN': Adversarial(PatchSize="
                         "crop, gan_type='STGAN')) to the training loss; a patch discriminator is trained beside the model by its own "
                         "Adamax (default: trainer.gan.weight of the config, else 0 = off)")
    ap.add_argument("--lpips_net", type=str, default=None,
                    help="LPIPS: the trunk, vgg or alex (default: trainer.lpips_net of the config, else vgg; the reference "
                         "trains with alex)")
    ap.add_argument("--lpips_lin", type=str, default=None,
                    help="LPIPS: the reference's linear heads, loss/PerceptualSimilarity/models/weights/v0.1/vgg.pth (alex.pth "
                         "with --lpips_net alex)")
    ap.add_argument("--lpips_backbone", type=str, default=None,
                    help="LPIPS: torchvision's VGG-16 state dict (vgg16-397923af.pth of the torch hub cache; "
                         "alexnet-owt-7be5be79.pth with --lpips_net alex)")
    add_loader_arguments(ap)
    add_monitor_arguments(ap)
    add_averaging_arguments(ap)
    return ap.parse_args(argv)


def main(argv=None):
    args = get_args(argv)
    with open(args.config) as fh:
        config = yaml.safe_load(fh)
    lpips_net = perceptual_net(config, args)                                          # (refuses before any device work)
    lpips_weight, lpips_lin, lpips_backbone = perceptual_settings(config, args)      # (likewise)
    gan_weight, gan_type = adversarial_settings(config, args)                         # (likewise)
    optimizer = optimizer_settings(config, args)                                      # (likewise)
    averaging = averaging_settings(config, args)                                      # (likewise)
    tr = config.get("trainer", {}) or {}
    st = trainer_settings(config, args.iterations)
    vs = validation_settings(config, args.valid_data)
    vs["use_ema"] = averaging["ema_validate"]
    rank, world, gpu = init_distributed_mode()
    device = torch.device("cuda", gpu)
    assert config["model"]["name"] == "EVFIAutoEx", "only the EVFIAutoEx hot path is implemented"

    perceptual, loss_note = None, ""
    if lpips_weight > 0:
        perceptual, loss_note = perceptual_term(lpips_net, lpips_lin, lpips_backbone, lpips_weight, device)
    adversarial = None
    if gan_weight > 0:
        adversarial, gan_note = adversarial_term(int(tr.get("height", 256)), gan_type, gan_weight, args.seed)
        loss_note += gan_note
        # the neighbours of every latent frame come with the recorded clips' batches (clipdata, dataset.NeedNeighborGT)
        loader_cfg = config.get("train_dataloader") or {}
        loader_cfg["dataset"] = dict(loader_cfg.get("dataset") or {}, NeedNeighborGT=True)
        config["train_dataloader"] = loader_cfg
    eng = Engine(config["model"]["args"], device=device, precision=args.precision, optimizer=optimizer,
                 seed=args.seed,                                                      # same init on every rank
                 graph=args.graph or bool(tr.get("graph", False)), accu_step=st["accu_step"],
                 backward_f16=False if args.no_f16_backward else None, forward_f16=None if args.no_f16_forward else "filters",
                 perceptual=perceptual, clip_grad=averaging["clip_grad"], ema=averaging["ema"], adversarial=adversarial)
    scheduler = build_lr_scheduler(config, eng.optimizer.inner)
    # monitor / best checkpoint / early stop (train_ours.py:155-163): only with validation on -- otherwise monitor_best stays None
    monitor = Monitor(vs["monitor"], vs["early_stop"],
                      warn=None if rank == 0 else (lambda msg: None)) if vs["do_validation"] else None
    start = resume_checkpoint(args.resume, eng, scheduler, config, reset=args.reset, map_location=device,
                              monitor=monitor) if args.resume else 0
    B, H, W = int(tr.get("batch_size", 8)), int(tr.get("height", 256)), int(tr.get("width", 256))
    TB = int(config["model"]["args"]["TB"])
    out_dir = os.path.join(tr.get("output_path", "./output"), "models", config.get("experiment", "Ours"), args.runid)

    make = synthetic_batch_from_raw_events if args.raw_events else synthetic_batch
    real = real_data_passes(args.data, config, B, TB, device, rank, world, args.seed, args.loader, args.prefetch, args.event_noise,
                            args.hot_pixels) if args.data else None
    valid_batches, tracker = None, None
    if vs["do_validation"]:
        from ebfi_amd.metrics import MetricTracker
        valid_batches = validation_batches(vs, config, args, B, H, W, TB, device, rank, world)
        tracker = MetricTracker(eng.VALID_KEYS)

    def next_micro_batch(it, micro):
        if real is not None:
            # one pass per latent frame of the loaded periods, in the reference's order (train_ours.py:226-251)
            return next(real)
        # one fresh synthetic batch per pass, different on every rank (seed + rank, like the reference); drawn by the
        # device generator unless --host-data: the host draw alone would cap the loop at ~15 frames/s
        batch_seed = args.seed + 1000 * (it * st["accu_step"] + micro)
        batch = make(B, H, W, TB, device=device, seed=batch_seed, rank=rank, on_device=not args.host_data)
        # (with the adversarial term: two further seeded frames per sample as the neighbours)
        return batch if adversarial is None else with_neighbours(batch, batch_seed + rank, not args.host_data)

    telemetry = build_monitor(config, args, args.runid, rank, eng)
    it = train_loop(eng, next_micro_batch, B, "frames", st, vs, scheduler, monitor, valid_batches, tracker, out_dir, config, rank,
                    world, start, loss_note=loss_note, telemetry=telemetry)
    if telemetry is not None:
        telemetry.close()
    if real is not None:
        real.close()                     # (joins the loader's worker thread)
    if rank == 0 and eng.book is not None:
        # fp16 backward (ebfi_amd.f16scale): optimiser steps skipped because an operand left the fp16 range (expected: 0)
        print("fp16 backward: %d of %d optimiser steps skipped by the overflow guard, %d operand scale slots"
              % (eng.book.skipped_steps(), it - start, len(eng.book.index)), flush=True)
    if world > 1:
        dist.destroy_process_group()


if __name__ == "__main__":
    main()
