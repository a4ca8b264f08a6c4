#!/usr/bin/env python3
"""train_ours_exposuredecision.py -- stage 1 of the reference's two-stage recipe on an MI355X: ExposureDecision alone is fitted
to the ground-truth exposure duty of the data (reference train_ours_exposuredecision.py:188-326, :521-592, :703-790).

Stage 2 is train_ours.py with `model.args.LoadPretrainEX: True` and `PretrainedEXPath` pointing at a checkpoint written here
(optionally `FrozenEX: True`).  The checkpoint layout is the reference's: {model:{name:"ExposureDecision", states}, lr_scheduler,
optimizer, config, trainer:{training_mode, iteration, monitor_best}} in checkpoint-iteration{it}.pth /
model_best_until_iteration{it}.pth; `states` is what ExposureDecision.load_pretrain reads.

The iteration body follows the reference: every period of a load is one micro-step -- blur-level map (model.BlurryFashion) ->
ExposureDecision -> MSELoss(Ex, ExposureDuty) / accu_step -> backward -- and every accu_step-th micro-step takes the Adam step,
logs, validates (valid_loss = the reference's sum over a load's periods of MSELoss; valid_mae beside it), saves, then steps the
lr scheduler.  That loop, settings, scheduler, monitor / early stop, checkpoints and resume are train_ours.py's own; the engine is
ebfi_amd.exposure_engine.ExposureEngine.  Data: synthetic batches or, with --data, recorded clips through ebfi_amd.clipdata.
TensorBoard and image dumps of the reference are out of scope.

    python train_ours_exposuredecision.py -c config/train_ours_exposuredecision.yml -id ex --iterations 200
    python -m torch.distributed.run --nproc-per-node 8 --master-addr 127.0.0.1 train_ours_exposuredecision.py -id ex
"""
import argparse
import os
import sys

import torch
import torch.distributed as dist
import yaml

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)

from train_ours import (CHECKPOINT_KEYS, TRAINING_MODE, Monitor, add_averaging_arguments, add_loader_arguments,  # noqa: E402,F401
                        add_monitor_arguments, averaging_settings,
                        best_checkpoint_name, build_lr_scheduler, build_monitor, checkpoint_state, clip_dataset, init_distributed_mode,
                        optimizer_settings, resume_checkpoint, save_checkpoint, train_loop, trainer_settings, validation_seeds, validation_settings, with_noise_law)
from ebfi_amd.exposure_engine import (BLURRY_FASHIONS, check_fashion, check_model_name,  # noqa: E402,F401
                                      synthetic_exposure_batch)

DEFAULT_CONFIG = os.path.join(HERE, "config", "train_ours_exposuredecision.yml")
DEFAULT_EXPOSURE_TIME = list(range(1, 16))          # ExposureTime of the reference's stage-1 config (Custom exposure)


def build_parser():
    ap = argparse.ArgumentParser(description="Stage-1 pre-training of ExposureDecision")
    # the reference's command line (train_ours_exposuredecision.py:774-792)
    ap.add_argument("-c", "--config", default=DEFAULT_CONFIG)
    ap.add_argument("-id", "--runid", default=None, help="run name (default: the config's `id`, else 'run')")
    ap.add_argument("-seed", "--seed", type=int, default=123)
    ap.add_argument("-r", "--resume", default=None, help="checkpoint to resume from")
    ap.add_argument("--reset", action="store_true", help="with --resume: load the model only, restart optimiser / schedule / count")
    ap.add_argument("--limited_memory", action="store_true",
                    help="accepted for the reference's command line (there it switches the sharing strategy of the data loader's "
                         "worker processes; this trainer has none)")
    ap.add_argument("-lr", "--learning_rate", type=float, default=None, help="overrides optimizer.args.lr")
    ap.add_argument("-bs", "--batch_size", type=int, default=None, help="overrides the per-GPU batch size")
    # what train_ours.py adds
    ap.add_argument("--iterations", type=int, default=None)
    ap.add_argument("--precision", default="bf16x3", choices=["fp32", "bf16x3"],
                    help="matrix-core operands of the convs: bf16x3 = split bf16 pairs, fp32-grade accuracy (default); fp32 = exact")
    ap.add_argument("--graph", action="store_true", help="replay forward+loss+backward from a captured hipGraph")
    ap.add_argument("--host-data", action="store_true", help="draw every synthetic batch on the host (bit-identical across machines)")
    ap.add_argument("--data", default=None,
                    help="recorded clips instead of synthetic batches (a directory of .npz / .h5 clips, a datalist .txt or one clip "
                         "file, ebfi_amd.clipdata); train_dataloader.dataset of the config sets periods / exposure / crop")
    ap.add_argument("--valid-data", default=None,
                    help="validation clips instead of valid_dataloader.path_to_datalist_txt (with trainer.do_validation; without "
                         "either: a fixed set of trainer.valid_batches synthetic batches)")
    add_loader_arguments(ap)
    add_monitor_arguments(ap)
    add_averaging_arguments(ap)
    return ap


def exposure_settings(config):
    """What stage 1 reads beyond trainer_settings: model.name (checked), model.BlurryFashion (checked; the reference keeps it
    beside `args`, :113), model.args, TB = EventInch / 2, and the exposure lottery of the synthetic batches (dataset keys)."""
    model = config["model"]
    name = check_model_name(model["name"])
    fashion = check_fashion(model.get("BlurryFashion", (model.get("args") or {}).get("BlurryFashion")))
    margs = {k: v for k, v in (model.get("args") or {}).items() if k != "BlurryFashion"}
    event_inch = int(margs.get("EventInch", 32))
    if event_inch % 2:
        raise ValueError("model.args.EventInch must be 2 * TIME_BINS, got %d" % event_inch)
    ds = ((config.get("train_dataloader") or {}).get("dataset") or {})
    tr = config.get("trainer", {}) or {}
    return {"name": name, "fashion": fashion, "model_args": margs, "TB": event_inch // 2,
            "exposure_time": list(ds.get("ExposureTime", DEFAULT_EXPOSURE_TIME)),
            "frames_per_period": int(ds.get("NumFramePerPeriod", 16)),
            "batch_size": int(tr.get("batch_size", (config.get("train_dataloader") or {}).get("batch_size", 4))),
            "height": int(tr.get("height", 128)), "width": int(tr.get("width", 128))}


def real_data_periods(path, config, es, device, rank, world, seed, loader="device", prefetch=1, event_noise="host",
                      hot_pixels=False):
    """Endless stream of (Frame [B,3,H,W], Event [B,TB,2,H,W], Duty [B,1]) micro-steps from recorded clips: one per period of
    every load of a collated batch, in the reference's order (:221-231)."""
    from ebfi_amd import clipdata
    ds_cfg = with_noise_law((config.get("train_dataloader") or {}).get("dataset") or {}, event_noise, hot_pixels)
    ds = clip_dataset(path, ds_cfg, es["TB"], DEFAULT_EXPOSURE_TIME, device, seed, loader)
    B = es["batch_size"]
    if len(ds) < B * world:
        raise SystemExit("--data: %d periods in %s, need at least batch_size x world = %d" % (len(ds), path, B * world))
    for batch in clipdata.batches(ds, B, rank=rank, world=world, seed=seed, prefetch=prefetch):
        frames, events, duties = batch["SeqBlurryF"], batch["SeqHREv"], batch["SeqExposureDuty"]
        for load in range(frames.shape[1]):
            for i in range(frames.shape[2]):
                yield frames[:, load, i].contiguous(), events[:, load].contiguous(), duties[:, load, i].contiguous()


def validation_batches(vs, es, args, device, rank, world):
    """-> a function that yields this rank's validation batches, the same ones at every stamp (as train_ours.validation_batches):
    recorded clips as collated dicts, or `valid_batches` synthetic (Frame, Event, Duty) periods made once."""
    from ebfi_amd import clipdata
    vb = vs["batch_size"] or es["batch_size"]
    if vs["valid_data"]:
        ds_cfg = with_noise_law(vs["dataset"], args.event_noise, args.hot_pixels)
        ds = clip_dataset(vs["valid_data"], ds_cfg, es["TB"], DEFAULT_EXPOSURE_TIME, device, args.seed, args.loader)
        if len(ds) == 0:
            raise SystemExit("--valid-data: no complete period in %s" % vs["valid_data"])
        return lambda: clipdata.eval_batches(ds, vb, rank=rank, world=world, seed=args.seed, drop_last=vs["drop_last"],
                                             prefetch=args.prefetch)
    seeds = validation_seeds(args.seed, vs["valid_batches"])
    mine = [synthetic_exposure_batch(vb, es["height"], es["width"], es["TB"], es["exposure_time"], es["frames_per_period"],
                                     device=device, seed=seeds[j]) for j in clipdata.shard_indices(len(seeds), rank, world)]
    return lambda: iter(mine)


def main(argv=None):
    args = build_parser().parse_args(argv)
    with open(args.config) as fh:
        config = yaml.safe_load(fh)
    tr = config.get("trainer", {}) or {}
    st = trainer_settings(config, args.iterations)
    vs = validation_settings(config, args.valid_data)
    es = exposure_settings(config)
    if args.batch_size:
        es["batch_size"] = int(args.batch_size)
    optimizer = optimizer_settings(config, args)      # (-lr overrides optimizer.args.lr; refuses before any device work)
    averaging = averaging_settings(config, args)      # (trainer.clip_grad / trainer.ema, --clip-grad-norm / --ema-decay; likewise)
    vs["use_ema"] = averaging["ema_validate"]
    rank, world, gpu = init_distributed_mode()
    device = torch.device("cuda", gpu)
    from ebfi_amd.exposure_engine import ExposureEngine
    from ebfi_amd.metrics import MetricTracker

    eng = ExposureEngine(es["model_args"], fashion=es["fashion"], device=device, precision=args.precision,
                         optimizer=optimizer, seed=args.seed,
                         graph=args.graph or bool(tr.get("graph", False)), accu_step=st["accu_step"], name=es["name"],
                         clip_grad=averaging["clip_grad"], ema=averaging["ema"])
    scheduler = build_lr_scheduler(config, eng.optimizer.inner)
    monitor = Monitor(vs["monitor"], vs["early_stop"],
                      warn=None if rank == 0 else (lambda msg: None)) if vs["do_validation"] else None
    start = resume_checkpoint(args.resume, eng, scheduler, config, reset=args.reset, map_location=device,
                              monitor=monitor) if args.resume else 0
    B, H, W, TB = es["batch_size"], es["height"], es["width"], es["TB"]
    runid = args.runid or str(config.get("id") or "run")
    out_dir = os.path.join(tr.get("output_path", "./output"), "models", config.get("experiment", "ExposurePretrain"), runid)

    real = real_data_periods(args.data, config, es, device, rank, world, args.seed, args.loader, args.prefetch, args.event_noise,
                             args.hot_pixels) if args.data else None
    valid_batches, tracker = None, None
    if vs["do_validation"]:
        valid_batches = validation_batches(vs, es, args, device, rank, world)
        tracker = MetricTracker(eng.VALID_KEYS)

    def next_micro_batch(it, micro):
        if real is not None:
            return next(real)
        return synthetic_exposure_batch(B, H, W, TB, es["exposure_time"], es["frames_per_period"], device=device,
                                        seed=args.seed + 1000 * (it * st["accu_step"] + micro), rank=rank,
                                        on_device=not args.host_data)

    telemetry = build_monitor(config, args, runid, rank, eng, default_experiment="ExposurePretrain")
    train_loop(eng, next_micro_batch, B, "samples", st, vs, scheduler, monitor, valid_batches, tracker, out_dir, config, rank, world,
               start, telemetry=telemetry)
    if telemetry is not None:
        telemetry.close()
    if real is not None:
        real.close()                     # (joins the loader's worker thread)
    if world > 1:
        dist.destroy_process_group()


if __name__ == "__main__":
    main()
