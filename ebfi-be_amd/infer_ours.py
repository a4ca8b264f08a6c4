#!/usr/bin/env python3
"""infer_ours.py -- MI355X counterpart of the reference inference entry point (infer_ours.py:40-152 loop, :156-172 model,
:193-220 flags, :222-375 main; scripts/infer_ours.sh).

Accepts the reference's command line unchanged:

    python infer_ours.py --model_path /path/to/model --data_list /path/to/test.txt --output_path /path/to/output \\
        --scale 2 --ori_scale down2 --time_bins 16 --num_frame_per_period 16 --num_frame_per_blurry 3 \\
        --num_period_per_seq 2 --sliding_window_seq 2 --num_period_per_load 1 --sliding_window_load 1 \\
        --exposure_method Fixed --noise_enabled

loads the checkpoint in the reference layout (`cpt['config']['model']`, `cpt['model']['states']`), reads every clip of the
list (one path per line, like `pd.read_csv(data_list, header=None)`) through ebfi_amd.clipdata -- periods, exposure, event
normalisation and binning, centre crop and event noise as dataloader/h5dataset.py does them; `.npz` clips, or `.h5` in the
reference's layout when h5py is installed -- walks the dataset's sequences / loads / latent timestamps in the reference's
order (infer_ours.py:82-118) with `model(Frame, Event, T, GTEx)[-1]` per timestamp (ebfi_amd.engine.ClipInterpolator: the
timestamp-independent prefix once per load, the rest replayed from a hipGraph; bit-identical to the per-timestamp call) and
writes, per clip, `<output_path>/<clip name>/restored.npz` (`restored` float32 [loads, NumF, 3, H, W], `blurry`,
`exposure_duty`, `timestamps`) and -- with --png, when PIL is importable -- the reference's image tree
`<clip name>/img/{restored_frame/%09d_%d.png, blurry_frame/%09d.png, gt_frame/%09d_%d.png}`.  --event_png (PIL again) adds the
tree's fourth directory, `img/event/{load}_TB{bin:09d}.png`: the reference's event-count image of every time bin of every load
(infer_ours.py:139-142: plot_event_cnt with 'blue_red', a white background and percentile normalisation), made on the device
by ebfi_amd.eventvis -- one call over all bins and one download per load, after the timed model interval -- bit-identical to
the array the reference's function returns; it works with --real_blur too, and --png alone writes what it always wrote.

Every restored timestamp is scored against the clip's sharp frame (infer_ours.py:120-128; --no-metrics switches it off): PSNR,
SSIM and MSE as loss/restore.py:43-92 and nn.MSELoss define them, computed on the device by ebfi_amd.metrics -- one call per
load, after the timed model interval -- and written as the reference writes them (:136-152, :340-417):
`<clip name>/inference.yml` (`evaluation results`: the clip's averages; `evaluation step results`: the per-timestamp psnr list)
and, after the last clip, `inference_all.yml` (per-clip breakdown, mean over clips) and `inference_all_step.yml` (per-step mean
over the shortest list); `restored.npz` also carries `psnr` / `ssim` / `mse` [loads, NumF].  LPIPS (AlexNet, v0.1, the
reference's fourth metric) is scored too when both of its weight files are named -- `--lpips_lin` the reference's
loss/PerceptualSimilarity/models/weights/v0.1/alex.pth, `--lpips_backbone` torchvision's AlexNet state dict
(alexnet-owt-7be5be79.pth) -- by ebfi_amd.lpips on the device, after the timed interval like the others: `lpips` then appears
in the three yml files and in restored.npz.  Without them the key is left out and stderr says so.  `--lpips_net vgg` scores
the VGG-16 variant instead (the two flags then name v0.1/vgg.pth and torchvision's vgg16-397923af.pth): the yml key stays
`lpips`, restored.npz gains `lpips_net`, and stderr names the net beside each clip's value.

`--real_blur` (the second block of scripts/infer_ours.sh) reads the clips as exposure-stamped recordings of a real camera
(ebfi_amd.clipdata.RealBlurClipDataset, the counterpart of dataloader/h5dataset_realdata.py): every stored frame is a blurry
input, its exposure duty comes from the frame's `exposure_begin_t` / `exposure_end_t` stamps, and each load is restored at
`--interp_num` timestamps `linspace(0, 1, interp_num)`.  Such clips have no sharp ground truth, so nothing is scored: no
inference.yml / inference_all*.yml, no gt_frame/ directory, --lpips_* unused (stderr says so once).  Both ends of the run are
device work (ebfi_amd.frameio): a frame is uploaded as uint8 and made planar float by a kernel that also applies the centre
crop; a load's restored frames are clamped, quantised (the reference's truncating cast, infer_ours.py:135) and interleaved by a
second kernel, one launch and one download per load.  `restored.npz` then holds `restored_u8` uint8 [loads, interp_num, H, W, 3],
`blurry_u8` [loads, H, W, 3] (the cast the reference applies to the blurry frame it saves), `exposure_duty`, `timestamps` and
`period`; --save_float adds the float32 `restored` [loads, interp_num, 3, H, W] (at 260x346 and 256 timestamps that is 276 MB
per load, hence not the default).  --png writes `img/restored_frame/%09d_%d.png` and `img/blurry_frame/%09d.png` from the uint8
arrays.

Not done here (out of the hot path's scope): the reference's other event plots (3-D clouds, image grids).  A knob this reader cannot honour is
reported on stderr, never dropped silently.  Without --data_list the script runs a synthetic clip (BASELINE.json configs 1 / 2 / 5):

    python infer_ours.py --model_path output/models/Ours/run/checkpoint-iteration99.pth --batch 4 --height 256 --width 256
    python infer_ours.py --batch 1 --height 128 --width 128 --rand-init
    (train_ours.py names a checkpoint after the LAST COMPLETED iteration, counted from 0 like the reference: a 100-iteration
    run writes checkpoint-iteration99.pth and is resumed at iteration 100)
"""
import argparse
import json
import os
import sys
import time

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))

from ebfi_amd.engine import DEFAULT_MODEL_ARGS, synthetic_batch  # noqa: E402
from models.Ours.model_singleframe import EVFIAutoEx  # noqa: E402,F401  (resolved by name, like the reference's eval())

# the dataset defaults infer_ours.py:223-236 starts from before the flags override them
REFERENCE_DATASET_DEFAULTS = dict(scale=4, ori_scale="down4", time_bins=1, interp_num=16, NumFramePerPeriod=16, NumFramePerBlurry=9,
                                  NumPeriodPerSeq=2, SlidingWindowSeq=2, NumPeriodPerLoad=2, SlidingWindowLoad=2,
                                  ExposureMethod="Fixed", ExposureTime=None, DeblurPretrain=False,
                                  noise=dict(enabled=True, noise_std=1.0, noise_fraction=0.05), center_crop=None,
                                  hot_pixel=dict(enabled=True, hot_pixel_std=2.0, hot_pixel_fraction=0.001))


def warn(msg):
    print("infer_ours.py: " + msg, file=sys.stderr, flush=True)


def load_model(model_path, device, ema=False):
    """ema: load the checkpoint's exponential moving average of the weights (its `ema.states`, written by a training run with
    trainer.ema / --ema-decay) over the model: trainable parameters from the average, everything else from model.states."""
    averaged = None
    if model_path is None:
        if ema:
            raise SystemExit("infer_ours.py: --ema needs a checkpoint (--model_path)")
        name, margs, states = "EVFIAutoEx", dict(DEFAULT_MODEL_ARGS), None
    else:
        assert os.path.isfile(model_path), model_path
        cpt = torch.load(model_path, map_location="cpu", weights_only=False)
        name, margs, states = cpt["config"]["model"]["name"], cpt["config"]["model"]["args"], cpt["model"]["states"]
        if ema:
            if not isinstance(cpt.get("ema"), dict) or not cpt["ema"].get("states"):
                raise SystemExit("infer_ours.py: --ema: %s holds no averaged weights (no `ema` entry: it was written by a run "
                                 "without trainer.ema / --ema-decay)" % model_path)
            averaged = cpt["ema"]["states"]
    model = globals()[name](**margs)
    if states is not None:
        model.load_state_dict(states)
    if averaged is not None:
        unknown = model.load_state_dict(averaged, strict=False).unexpected_keys
        if unknown:
            raise SystemExit("infer_ours.py: --ema: ema.states names parameters the model does not have (first: %s)" % unknown[0])
    return model.to(device).eval(), margs


def get_flags(argv=None):
    ap = argparse.ArgumentParser(description=__doc__.split("\n\n")[0])
    # ---- the reference's flags, same names / types / defaults (infer_ours.py:193-220) ----
    ap.add_argument("--model_path", type=str, default=None)
    ap.add_argument("--data_list", type=str, default=None)
    ap.add_argument("--device", type=str, default="cuda:0")
    ap.add_argument("--output_path", type=str, default=None, help="required with --data_list (the reference requires it always)")
    ap.add_argument("--scale", type=int, default=None)
    ap.add_argument("--ori_scale", type=str, default=None)
    ap.add_argument("--time_bins", type=int, default=None)
    ap.add_argument("--interp_num", type=int, default=None)
    ap.add_argument("--num_frame_per_period", type=int, default=None)
    ap.add_argument("--num_frame_per_blurry", type=int, default=None)
    ap.add_argument("--num_period_per_seq", type=int, default=None)
    ap.add_argument("--sliding_window_seq", type=int, default=None)
    ap.add_argument("--num_period_per_load", type=int, default=None)
    ap.add_argument("--sliding_window_load", type=int, default=None)
    ap.add_argument("--exposure_method", type=str, default=None)
    ap.add_argument("--exposure_time", type=str, default=None)
    ap.add_argument("--deblur_pretrain", default=False, action="store_true")
    ap.add_argument("--noise_std", type=float, default=None)
    ap.add_argument("--noise_enabled", default=True, action="store_false",
                    help="as in the reference this flag SWITCHES THE EVENT NOISE OFF (store_false; 'false for real-world data')")
    ap.add_argument("--center_crop_size", type=int, nargs="+", default=None)
    ap.add_argument("--real_blur", default=False, action="store_true")
    ap.add_argument("--ema", action="store_true",
                    help="run the checkpoint's exponential moving average of the weights (its `ema` entry) instead of the raw "
                         "iterate; ends with a message when the checkpoint holds none")
    # ---- this implementation's own ----
    ap.add_argument("--png", action="store_true", help="also write the reference's PNG tree (needs PIL)")
    ap.add_argument("--event_png", action="store_true",
                    help="also write img/event/{load}_TB{bin:09d}.png, the reference's event-count image of every time bin of "
                         "every load (blue_red, white background, normalised; needs PIL)")
    ap.add_argument("--save_float", action="store_true",
                    help="with --real_blur: also store the float32 `restored` array in restored.npz (uint8 `restored_u8` only by default)")
    ap.add_argument("--no-metrics", action="store_true",
                    help="with --data_list: do not score the restored frames against the clip's sharp frames (PSNR / SSIM / MSE)")
    ap.add_argument("--lpips_lin", type=str, default=None,
                    help="LPIPS: the reference's linear heads, loss/PerceptualSimilarity/models/weights/v0.1/alex.pth (with "
                         "--lpips_backbone, the metrics also score LPIPS)")
    ap.add_argument("--lpips_backbone", type=str, default=None,
                    help="LPIPS: torchvision's AlexNet state dict (alexnet-owt-7be5be79.pth of the torch hub cache)")
    ap.add_argument("--lpips_net", type=str, default="alex", choices=("alex", "vgg"),
                    help="LPIPS: the trunk, the reference's perceptual_loss(net=...).  With vgg, --lpips_lin names v0.1/vgg.pth "
                         "and --lpips_backbone torchvision's VGG-16 state dict (vgg16-397923af.pth); the yml key stays `lpips`")
    ap.add_argument("--data_seed", type=int, default=123, help="base of the per-item seeds (noise draw); the reference seeds "
                                                                "python's generator with 123 and draws one seed per item")
    ap.add_argument("--event-noise", dest="event_noise", default="host", choices=["host", "device"],
                    help="with --data_list: 'host' draws the event noise as the reference does, bit for bit, on one host thread "
                         "(about a second per 720 x 1280 load); 'device' draws a counter-based law of the same distribution in "
                         "the kernel that cuts the event stack (ebfi_amd.eventaug)")
    ap.add_argument("--hot-pixels", dest="hot_pixels", action="store_true",
                    help="with --data_list and --event-noise device: honour the reference's hot_pixel section (std 2.0 on a "
                         "fraction 0.001 of the pixels, switched with the noise by --noise_enabled; the reference's own guard "
                         "never lets it run)")
    ap.add_argument("--batch", type=int, default=4, help="synthetic mode (no --data_list)")
    ap.add_argument("--height", type=int, default=256)
    ap.add_argument("--width", type=int, default=256)
    ap.add_argument("--num_ts", type=int, default=16, help="synthetic mode: latent timestamps per clip (NumI of the reference loop)")
    ap.add_argument("--seed", type=int, default=123)
    ap.add_argument("--precision", default="bf16x3", choices=["fp32", "bf16x3", "bf16"],
                    help="matrix-core operands of the convs: bf16x3 = split bf16 pairs, fp32-grade accuracy (default); fp32 = exact")
    ap.add_argument("--rand-init", action="store_true",
                    help="without --model_path: draw O(1)-gain random weights instead of the reference's x0.1 initialisation, "
                         "whose output is the constant 0.5 (benchmark / profile runs: the printed mean then depends on the data)")
    ap.add_argument("--no-graph", action="store_true", help="launch every kernel eagerly instead of replaying a captured hipGraph")
    ap.add_argument("--group", type=int, default=None,
                    help="latent timestamps computed per pass, as one batch (default: as many as keep B * k * H * W within a pixel "
                         "budget; 1 = one per pass, bit-identical to the reference loop's per-timestamp call)")
    ap.add_argument("--no-hoist", action="store_true",
                    help="recompute the timestamp-independent prefix (feature extractors, exposure decision) for every timestamp")
    return ap.parse_args(argv)


def dataset_settings(flags):
    """infer_ours.py:222-340: the reference's defaults overridden by the flags that were given, in its key names; plus the list
    of warnings for what this reader cannot honour (returned, so that tests can see them)."""
    ds = {k: (dict(v) if isinstance(v, dict) else v) for k, v in REFERENCE_DATASET_DEFAULTS.items()}
    for flag, key in (("scale", "scale"), ("ori_scale", "ori_scale"), ("time_bins", "time_bins"), ("interp_num", "interp_num"),
                      ("num_frame_per_period", "NumFramePerPeriod"), ("num_frame_per_blurry", "NumFramePerBlurry"),
                      ("num_period_per_seq", "NumPeriodPerSeq"), ("sliding_window_seq", "SlidingWindowSeq"),
                      ("num_period_per_load", "NumPeriodPerLoad"), ("sliding_window_load", "SlidingWindowLoad"),
                      ("exposure_method", "ExposureMethod"), ("exposure_time", "ExposureTime")):
        v = getattr(flags, flag)
        if v is not None:
            ds[key] = v
    ds["DeblurPretrain"] = bool(flags.deblur_pretrain)
    if flags.noise_std is not None:
        ds["noise"].update(enabled=True, noise_std=flags.noise_std, noise_fraction=0.05)
    ds["noise"]["enabled"] = bool(flags.noise_enabled)           # (:329-331: the flag decides last)
    ds["event_noise"] = getattr(flags, "event_noise", "host")    # (this implementation's own: the law, and the hot pixels)
    ds["hot_pixel"]["enabled"] = bool(flags.noise_enabled)       # (:345: switched together with the noise)
    ds["hot_pixels"] = ((ds["hot_pixel"]["hot_pixel_std"], ds["hot_pixel"]["hot_pixel_fraction"])
                        if getattr(flags, "hot_pixels", False) and ds["hot_pixel"]["enabled"] else None)
    if flags.center_crop_size is not None:
        ds["center_crop"] = list(flags.center_crop_size) * (2 if len(flags.center_crop_size) == 1 else 1)
    notes = []
    factor = {"ori": 1, "down2": 2, "down4": 4, "down8": 8, "down16": 16}.get(str(ds["ori_scale"]))
    if factor is None or int(ds["scale"]) != factor:
        notes.append("scale %r with ori_scale %r selects down-scaled ground-truth groups of the reference's HDF5 layout; this reader "
                     "opens a clip's 'ori' groups only: running on them" % (ds["scale"], ds["ori_scale"]))
    if int(ds["NumPeriodPerLoad"]) != 1:
        notes.append("num_period_per_load %r: the reference's own loop feeds `SeqBlurryF[idxL].squeeze(1)` to the model, which is a "
                     "frame only for one period per load (scripts/infer_ours.sh passes 1); running with 1" % (ds["NumPeriodPerLoad"],))
        ds["NumPeriodPerLoad"] = 1
        ds["SlidingWindowLoad"] = 1
    if isinstance(ds["ExposureTime"], str):
        # (the reference declares the flag as a string and indexes it like a list; a list of integers is what it needs)
        try:
            ds["ExposureTime"] = [int(v) for v in ds["ExposureTime"].replace(",", " ").split()]
        except ValueError:
            notes.append("exposure_time %r is not a list of integers: ignored" % (ds["ExposureTime"],))
            ds["ExposureTime"] = None
    if ds["DeblurPretrain"]:
        notes.append("deblur_pretrain: the reference's loop never reads the flag after storing it; ignored here too")
    ds["real_blur"] = bool(flags.real_blur)
    if flags.real_blur:
        notes.append("real_blur: the clips are read as exposure-stamped recordings (one period per stored frame, the exposure duty "
                     "from its exposure_begin_t / exposure_end_t stamps, %d timestamps per load); they hold no sharp ground truth, "
                     "so nothing is scored and no inference*.yml is written" % int(ds["interp_num"]))
    if flags.interp_num is not None and not flags.real_blur:
        notes.append("interp_num only applies to --real_blur in the reference; ignored")
    return ds, notes


def write_png(path, chw):
    from PIL import Image
    arr = (chw.clamp(0, 1).cpu().numpy().transpose(1, 2, 0) * 255).astype("uint8")      # (infer_ours.py:137: truncating cast)
    Image.fromarray(arr).save(path)


def mean_per_step(lists):
    """infer_ours.py:175-190 (process): the mean over the clips of each step's value, over the length of the shortest list."""
    n = min((len(v) for v in lists), default=0)
    return [float(np.mean([v[i] for v in lists])) for i in range(n)]


def write_results(path, content):
    """The reference's Logger_yaml (myutils/utils.py:218-230): one yaml.dump of the dict.  Without PyYAML the same dict goes to
    `<path minus .yml>.json` (reported on stderr).  Returns the path written."""
    try:
        import yaml
    except ImportError:
        yaml = None
    if yaml is None:
        path = os.path.splitext(path)[0] + ".json"
        warn("PyYAML is not importable: writing %s as JSON" % path)
        with open(path, "w") as f:
            json.dump(content, f, indent=1, sort_keys=True)
        return path
    with open(path, "w") as f:
        yaml.dump(content, f)
    return path


def summarise_clips(results, info):
    """infer_ours.py:386-417: the contents of inference_all.yml and inference_all_step.yml from the per-clip results
    [(clip name, {metric: clip average}, {"psnr": per-step list})]."""
    breakdown, means, breakdown_step, means_step = {}, {}, {}, {}
    for name, result, result_step in results:
        for k, v in result.items():
            breakdown.setdefault(k, {})[name] = float(v)
            means.setdefault(k, []).append(float(v))
        for k, v in result_step.items():
            breakdown_step.setdefault(k, {})[name] = [float(x) for x in v]
            means_step.setdefault(k, []).append(list(v))
    all_ = {"info": [info], "breakdown results for each data": breakdown,
            "mean results for the whole data": {k: float(np.mean(v)) for k, v in means.items()}}
    all_step = {"info": [info], "breakdown results for each data": breakdown_step,
                "mean results for the whole data (based on min length)": {k: mean_per_step(v) for k, v in means_step.items()}}
    return all_, all_step


@torch.no_grad()
def infer_clip(interp, data_path, ds_cfg, root_path, device, seed, png=False, metrics=True, info="", lpips=None, event_png=False):
    """infer_body of the reference for one clip: every sequence, every load, every latent timestamp; returns
    (frames written, seconds inside the model, (result, result_step) or None without metrics).  lpips: an
    ebfi_amd.lpips.AlexLPIPS or VggLPIPS that scores LPIPS as a fourth metric, or None."""
    from ebfi_amd import clipdata
    from ebfi_amd.metrics import MetricTracker, frame_metrics
    name = os.path.basename(data_path)
    data = clipdata.ClipDataset(data_path, time_bins=int(ds_cfg["time_bins"]), frames_per_period=int(ds_cfg["NumFramePerPeriod"]),
                                frames_per_blurry=int(ds_cfg["NumFramePerBlurry"]), exposure_method=ds_cfg["ExposureMethod"],
                                exposure_time=ds_cfg["ExposureTime"], crop=ds_cfg["center_crop"], crop_mode="center", flips=False,
                                device=device, seed=seed, noise_mode=ds_cfg.get("event_noise", "host"), hot_pixels=ds_cfg.get("hot_pixels"),
                                noise=(ds_cfg["noise"]["noise_std"], ds_cfg["noise"]["noise_fraction"]) if ds_cfg["noise"]["enabled"] else None)
    seqs = clipdata.sequence_items(len(data), ds_cfg["NumPeriodPerSeq"], ds_cfg["SlidingWindowSeq"], ds_cfg["NumPeriodPerLoad"],
                                   ds_cfg["SlidingWindowLoad"])
    img_path = os.path.join(root_path, "img")
    os.makedirs(root_path, exist_ok=False)                # (like the reference: an existing result is never overwritten)
    if png:
        for sub in ("blurry_frame", "gt_frame", "restored_frame"):
            os.makedirs(os.path.join(img_path, sub), exist_ok=False)
    if event_png:
        os.makedirs(os.path.join(img_path, "event"), exist_ok=False)
    restored, blurry, duties, stamps, loads = [], [], [], [], []
    scores = []                                            # per load: [3 (psnr, ssim, mse) or 4 (+ lpips), NumF]
    lpips_net = getattr(lpips, "NET", "alex")              # (the yml key stays `lpips`, the reference's, whatever the net)
    track = MetricTracker(["mse", "psnr", "ssim"] + (["lpips"] if lpips is not None else []))
    step = {"psnr": []}
    iL = iF = -1
    spent = 0.0
    for si, seq in enumerate(seqs):
        for (left, right) in seq:
            iL += 1
            item = data.__getitem__(left, seed=seed + 7919 * si + left)
            frame = item["SeqBlurryF"][0]                  # [1(NumP), 3, H, W] -> batch of one, like the reference's batch_size 1
            event = item["SeqHREv"]                        # [1(L), TB, 2, H, W]
            ts = item["RelativeLatentTs"][0, 0]            # [NumF]
            duty = item["SeqExposureDuty"][0]              # [1, 1]
            torch.cuda.synchronize(device)
            t0 = time.perf_counter()
            pred = interp(frame.contiguous(), event.contiguous(), duty.contiguous(), [float(v) for v in ts.tolist()])
            torch.cuda.synchronize(device)
            spent += time.perf_counter() - t0
            if metrics:                                    # (after the timed interval: the frames/s line keeps its meaning)
                psnr, ssim, mse = frame_metrics(pred[0], item["SeqLatentF"][0, 0])
                per_load = [psnr, ssim, mse]
                if lpips is not None:
                    per_load.append(lpips(pred[0], item["SeqLatentF"][0, 0], normalize=True))
            restored.append(pred[0].cpu().numpy())          # [NumF, 3, H, W]
            if metrics:
                sc = torch.stack(per_load).cpu().numpy()
                scores.append(sc)
                for v in sc.T:                             # (per timestamp, in the reference's order)
                    step["psnr"].append(float(v[0]))
                    track.update("mse", float(v[2]))
                    track.update("psnr", float(v[0]))
                    track.update("ssim", float(v[1]))
                    if lpips is not None:
                        track.update("lpips", float(v[3]))
            blurry.append(frame[0].cpu().numpy())
            duties.append(float(duty.item()))
            stamps.append(ts.cpu().numpy())
            loads.append(left)
            for i in range(pred.shape[1]):
                iF += 1
                if png:
                    write_png(os.path.join(img_path, "restored_frame", "{:09d}_{}.png".format(iF, iL)), pred[0, i])
                    write_png(os.path.join(img_path, "gt_frame", "{:09d}_{}.png".format(iF, iL)), item["SeqLatentF"][0, 0, i])
            if png:
                write_png(os.path.join(img_path, "blurry_frame", "%09d.png" % iL), frame[0])
            if event_png:
                write_event_pngs(os.path.join(img_path, "event"), iL, event[0])
    if restored:
        extra = {}
        if metrics:
            sc = np.stack(scores)
            extra = dict(psnr=sc[:, 0], ssim=sc[:, 1], mse=sc[:, 2])
            if lpips is not None:
                extra["lpips"] = sc[:, 3]
                if lpips_net != "alex":                    # (an AlexNet run writes what it always wrote)
                    extra["lpips_net"] = np.array(lpips_net)
        np.savez(os.path.join(root_path, "restored.npz"), restored=np.stack(restored), blurry=np.stack(blurry),
                 exposure_duty=np.array(duties, dtype=np.float32), timestamps=np.stack(stamps), period=np.array(loads), **extra)
    print("%s: %d loads, %d frames restored -> %s" % (name, iL + 1, iF + 1, root_path), flush=True)
    if not metrics:
        return iF + 1, spent, None
    result = track.result()
    write_results(os.path.join(root_path, "inference.yml"), {"info": [info], "evaluation results": result,
                                                              "evaluation step results": step})
    print("%s: psnr %.4f  ssim %.4f  mse %.6g over %d frames" % (name, result["psnr"], result["ssim"], result["mse"], iF + 1),
          flush=True)
    if lpips is not None and lpips_net != "alex":
        warn("%s: lpips (%s) %.6g over %d frames" % (name, lpips_net, result["lpips"], iF + 1))
    return iF + 1, spent, (result, step)


def write_png_u8(path, hwc):
    from PIL import Image
    Image.fromarray(hwc).save(path)


def write_event_pngs(event_dir, iL, stack):
    """infer_ours.py:139-142 for one load: stack [TB, 2, H, W] on the device -> event/{iL}_TB{idx:09d}.png per time bin.  One
    native call over all bins, one download."""
    from ebfi_amd.eventvis import event_count_images
    imgs = event_count_images(stack, color_scheme="blue_red", black_background=False, is_norm=True).cpu().numpy()
    for idx in range(imgs.shape[0]):
        write_png_u8(os.path.join(event_dir, "{}_TB{:09d}.png".format(iL, idx)), imgs[idx])


@torch.no_grad()
def infer_clip_real(interp, data_path, ds_cfg, root_path, device, seed, png=False, save_float=False, event_png=False):
    """infer_body of the reference with real_blur (infer_ours.py:81-118, :135-138) for one clip: every sequence of the dataset
    is one item, every load of it one frame, every load restored at the interp_num timestamps; nothing is scored.  Returns
    (frames written, seconds inside the model)."""
    from ebfi_amd import clipdata
    from ebfi_amd.frameio import planar_to_u8
    name = os.path.basename(data_path)
    data = clipdata.RealBlurClipDataset(data_path, time_bins=int(ds_cfg["time_bins"]), interp_num=int(ds_cfg["interp_num"]),
                                        periods_per_seq=ds_cfg["NumPeriodPerSeq"], sliding_window_seq=ds_cfg["SlidingWindowSeq"],
                                        periods_per_load=ds_cfg["NumPeriodPerLoad"], sliding_window_load=ds_cfg["SlidingWindowLoad"],
                                        crop=ds_cfg["center_crop"], device=device, noise_mode=ds_cfg.get("event_noise", "host"),
                                        hot_pixels=ds_cfg.get("hot_pixels"),
                                        noise=(ds_cfg["noise"]["noise_std"], ds_cfg["noise"]["noise_fraction"]) if ds_cfg["noise"]["enabled"] else None)
    img_path = os.path.join(root_path, "img")
    os.makedirs(root_path, exist_ok=False)                # (like the reference: an existing result is never overwritten)
    if png:
        for sub in ("blurry_frame", "restored_frame"):
            os.makedirs(os.path.join(img_path, sub), exist_ok=False)
    if event_png:
        os.makedirs(os.path.join(img_path, "event"), exist_ok=False)
    restored_u8, restored, blurry_u8, duties, stamps, loads = [], [], [], [], [], []
    iL = iF = -1
    spent = 0.0
    for si, seq in enumerate(data.items):
        item = data.__getitem__(si, seed=seed + 7919 * si + seq[0][0])
        for idxL, (left, right) in enumerate(seq):
            iL += 1
            frame = item["SeqBlurryF"][idxL]               # [1(NumP), 3, H, W] -> batch of one
            event = item["SeqHREv"][idxL:idxL + 1]         # [1, TB, 2, H, W]
            ts = item["RelativeLatentTs"][idxL, 0]         # [interp_num]
            duty = item["SeqExposureDuty"][idxL]           # [1, 1]
            torch.cuda.synchronize(device)
            t0 = time.perf_counter()
            pred = interp(frame.contiguous(), event.contiguous(), duty.contiguous(), [float(v) for v in ts.tolist()])
            torch.cuda.synchronize(device)
            spent += time.perf_counter() - t0
            u8 = planar_to_u8(pred[0]).cpu().numpy()        # [interp_num, H, W, 3]: one launch, one download per load
            b8 = planar_to_u8(frame).cpu().numpy()[0]      # (infer_ours.py:137: the same cast on the blurry frame)
            restored_u8.append(u8)
            if save_float:
                restored.append(pred[0].cpu().numpy())
            blurry_u8.append(b8)
            duties.append(float(duty.item()))
            stamps.append(ts.cpu().numpy())
            loads.append(left)
            for i in range(u8.shape[0]):
                iF += 1
                if png:
                    write_png_u8(os.path.join(img_path, "restored_frame", "{:09d}_{}.png".format(iF, iL)), u8[i])
            if png:
                write_png_u8(os.path.join(img_path, "blurry_frame", "%09d.png" % iL), b8)
            if event_png:
                write_event_pngs(os.path.join(img_path, "event"), iL, event[0])
    if restored_u8:
        extra = dict(restored=np.stack(restored)) if save_float else {}
        np.savez(os.path.join(root_path, "restored.npz"), restored_u8=np.stack(restored_u8), blurry_u8=np.stack(blurry_u8),
                 exposure_duty=np.array(duties, dtype=np.float32), timestamps=np.stack(stamps), period=np.array(loads), **extra)
    print("%s: %d loads, %d frames restored -> %s" % (name, iL + 1, iF + 1, root_path), flush=True)
    return iF + 1, spent


def noise_law_name(ds_cfg):
    """The active event-noise law, for the summary line."""
    hot = ", hot pixels std %g fraction %g" % tuple(ds_cfg["hot_pixels"]) if ds_cfg.get("hot_pixels") else ""
    if not ds_cfg["noise"]["enabled"]:
        return "off" + hot
    return "%s law, std %g on a fraction %g of the cells%s" % (ds_cfg.get("event_noise", "host"), ds_cfg["noise"]["noise_std"],
                                                             ds_cfg["noise"]["noise_fraction"], hot)


def run_data_list(flags, interp, device):
    ds_cfg, notes = dataset_settings(flags)
    for n in notes:
        warn(n)
    print({k: v for k, v in ds_cfg.items()}, flush=True)
    if flags.output_path is None:
        raise SystemExit("infer_ours.py: --output_path is required with --data_list")
    os.makedirs(flags.output_path, exist_ok=True)
    from ebfi_amd import clipdata
    paths = clipdata.list_clips(flags.data_list) if flags.data_list.endswith(".txt") else [flags.data_list]
    png, event_png = flags.png, flags.event_png
    if png or event_png:
        try:
            import PIL  # noqa: F401
        except ImportError:
            warn("%s needs PIL, which is not importable: writing restored.npz only"
                 % " / ".join(f for f, on in (("--png", png), ("--event_png", event_png)) if on))
            png = event_png = False
    metrics = not flags.no_metrics and not flags.real_blur      # (the real_blur note has said that nothing is scored)
    lpips = None
    if metrics and flags.lpips_lin is not None:
        from ebfi_amd.lpips import load_lpips
        lpips = load_lpips(flags.lpips_net, flags.lpips_lin, flags.lpips_backbone, device=device)
    elif metrics:
        from ebfi_amd.metrics import LPIPS_UNAVAILABLE
        warn(LPIPS_UNAVAILABLE + "; psnr / ssim / mse only")
    frames, spent, results = 0, 0.0, []
    for k, data_path in enumerate(paths):
        print("processing %s" % data_path, flush=True)
        if flags.real_blur:
            n, s = infer_clip_real(interp, data_path, ds_cfg, os.path.join(flags.output_path, os.path.basename(data_path)), device,
                                   seed=flags.data_seed + 100003 * k, png=png, save_float=flags.save_float,
                                   event_png=event_png)
            frames, spent = frames + n, spent + s
            continue
        n, s, r = infer_clip(interp, data_path, ds_cfg, os.path.join(flags.output_path, os.path.basename(data_path)), device,
                             seed=flags.data_seed + 100003 * k, png=png, metrics=metrics,
                             info="inference %s on %s" % ([flags.model_path], data_path), lpips=lpips,
                             event_png=event_png)
        frames, spent = frames + n, spent + s
        if r is not None:
            results.append((os.path.basename(data_path),) + r)
    print("restored %d frames of %d clip(s) in %.3f s inside the model: %.1f frames/s; event noise: %s"
          % (frames, len(paths), spent, frames / max(spent, 1e-9), noise_law_name(ds_cfg)))
    if metrics:
        # (written once every clip is done: a run refused half-way leaves an earlier run's summaries as they were)
        all_, all_step = summarise_clips(results, "inference %s \n on %s" % ([flags.model_path], paths))
        write_results(os.path.join(flags.output_path, "inference_all.yml"), all_)
        write_results(os.path.join(flags.output_path, "inference_all_step.yml"), all_step)


@torch.no_grad()
def main(argv=None):
    a = get_flags(argv)
    if (a.lpips_lin is None) != (a.lpips_backbone is None):
        raise SystemExit("infer_ours.py: LPIPS needs both weight files: --lpips_lin (the v0.1 alex.pth heads) and --lpips_backbone "
                         "(torchvision's AlexNet state dict); got only %s" % ("--lpips_lin" if a.lpips_backbone is None else "--lpips_backbone"))
    if a.lpips_lin is not None and (a.no_metrics or a.data_list is None or a.real_blur):
        warn("--lpips_lin / --lpips_backbone are unused: %s" % ("--no-metrics switches the scoring off" if a.no_metrics
                                                                 else "only a --data_list run is scored" if a.data_list is None
                                                                 else "--real_blur clips have no ground truth to score against"))
    if a.event_png and a.data_list is None:
        warn("--event_png only applies to a --data_list run (the synthetic mode writes no files); ignored")
    if a.save_float and not (a.real_blur and a.data_list is not None):
        warn("--save_float only applies to a --real_blur run (the synthetic-blur path always stores the float32 array); ignored")
    torch.manual_seed(a.seed)
    device = torch.device(a.device)
    if device.type != "cuda":
        raise SystemExit("infer_ours.py: the MI355X path needs a cuda device (got --device %s); there is no CPU fallback" % a.device)
    torch.cuda.set_device(device)
    model, margs = load_model(a.model_path, device, ema=a.ema)
    if a.rand_init and a.model_path is None:
        with torch.no_grad():
            for p in model.parameters():
                if p.dim() > 1:
                    p.copy_(torch.randn_like(p) * (1.2 / p[0].numel() ** 0.5))
                else:
                    p.add_(0.05 * torch.randn_like(p))
    from ebfi_amd.engine import ClipInterpolator
    # Frame / Event are the same for every latent timestamp of a load (reference loop infer_ours.py:113-118): the part of the
    # forward that does not depend on T -- padding, both feature extractors, Frame2Lap + ExposureDecision (6.2 of 91 GMAC) --
    # runs ONCE per load, the per-timestamp part is replayed from a captured hipGraph (ebfi_amd.engine.ClipInterpolator).
    # --no-hoist keeps the plain model(Frame, Event, T, GTEx) call per timestamp (bit-identical outputs).
    interp = ClipInterpolator(model, precision=a.precision, graph=not a.no_graph, hoist=not a.no_hoist, group=a.group)
    if a.data_list is not None:
        if a.time_bins is not None and int(a.time_bins) != int(margs["TB"]):
            raise SystemExit("infer_ours.py: --time_bins %d but the model was built with TB=%d" % (a.time_bins, margs["TB"]))
        if a.time_bins is None:
            a.time_bins = int(margs["TB"])          # (the reference's default of 1 cannot feed a TB-bin model)
        return run_data_list(a, interp, device)
    frame, event, _, gtex, _ = synthetic_batch(a.batch, a.height, a.width, margs["TB"], device=device, seed=a.seed)
    stamps = [i / float(a.num_ts) for i in range(a.num_ts)]
    out = torch.empty(a.batch, a.num_ts, 3, a.height, a.width, device=device)
    for _ in range(2):
        interp(frame, event, gtex, stamps, out=out)        # untimed: module load, allocator, graph capture (per group size)
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    interp(frame, event, gtex, stamps, out=out)   # one clip: the prefix once + num_ts replays
    torch.cuda.synchronize()
    dt = time.perf_counter() - t0
    print("interpolated %d frames of %dx%d in %.3f s: %.1f frames/s (%d timestamp(s) per pass); output %s, mean %.4f std %.4f, peak memory %.1f GB"
          % (a.batch * a.num_ts, a.height, a.width, dt, a.batch * a.num_ts / dt, interp.last_group, tuple(out.shape), out.mean().item(),
             out.std().item(), torch.cuda.max_memory_allocated(device) / 1e9))


if __name__ == "__main__":
    main()
