#!/usr/bin/env python3
"""`train_ours.py --data` on recorded clips at the shipped shape (720 x 1280 clips of 33 frames, NumFramePerPeriod 16, random crop
256, flips, batch 8): the steady-state rate of each loader arm, each a fresh child process, and the frame kernel and the event
kernel of the device loader in isolation (library event pairs; HBM fraction from their ProfScope bytes).
profiles/loader_real_data.md is its output.

usage: python tools/loaderbench.py --work DIR [--iterations 320] [--arms host,device,default,synthetic] [--kernel]
                                   [--tree OTHER_CHECKOUT]    # adds the arm 'other': that tree's train_ours.py --data, no flags
The arms 'noise-host' and 'noise-device' train with data_augment.noise on (std 1.0 on a fraction 0.05 of the cells) under
--event-noise host / device; run them alternating with 'default' (no noise), e.g.
    --arms default,noise-device,noise-host,default,noise-device
The clips (four, about 91 MB each) and the config are written under DIR once."""
import argparse
import os
import re
import subprocess
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "ebfi-be_amd"))

ARMS = {"host": ["--loader", "host", "--prefetch", "0"], "device": ["--loader", "device", "--prefetch", "0"], "default": [],
        "other": [], "noise-host": ["--event-noise", "host"], "noise-device": ["--event-noise", "device"]}
NOISE_ARMS = ("noise-host", "noise-device")          # these read the config whose noise section is enabled
HBM_GBS = 8000.0          # MI355X peak, for the fraction only


def setup(work):
    import yaml
    from ebfi_amd import clipdata
    clips = os.path.join(work, "clips")
    os.makedirs(clips, exist_ok=True)
    for k in range(4):
        path = os.path.join(clips, "clip%d.npz" % k)
        if not os.path.exists(path):
            clipdata.write_synthetic_clip(path, num_imgs=33, H=720, W=1280, seed=k)
    cfg = yaml.safe_load(open(os.path.join(ROOT, "ebfi-be_amd", "config", "train_ours.yml")))
    cfg["trainer"]["output_path"] = os.path.join(work, "output")
    cfg["trainer"]["iteration_based_train"].update(train_log_step=40, save_period=0)
    cfg["train_dataloader"] = {"dataset": {
        "scale": 1, "ori_scale": "ori", "time_bins": 16, "NumFramePerPeriod": 16, "NumFramePerBlurry": 16,
        "ExposureMethod": "Custom", "ExposureTime": [9, 10, 11, 12, 13, 14, 15],
        "data_augment": {"enabled": True, "augment": ["RandomCrop", "CenterCrop", "HorizontalFlip", "VertivcalFlip", "Noise", "HotPixel"],
                         "random_crop": {"enabled": True, "size": [256, 256]}, "center_crop": {"enabled": False, "size": [256, 256]},
                         "flip": {"enabled": True, "horizontal_prob": 0.5, "vertical_prob": 0.5},
                         "noise": {"enabled": False, "noise_std": 1.0, "noise_fraction": 0.05}}}}
    cfg_path = os.path.join(work, "loaderbench.yml")
    yaml.safe_dump(cfg, open(cfg_path, "w"))
    cfg["train_dataloader"]["dataset"]["data_augment"]["noise"]["enabled"] = True
    noise_path = os.path.join(work, "loaderbench_noise.yml")
    yaml.safe_dump(cfg, open(noise_path, "w"))
    return clips, cfg_path, noise_path


def run_arm(name, tree, cfg_path, clips, iterations, limit):
    cmd = [sys.executable, os.path.join(tree, "ebfi-be_amd", "train_ours.py"), "-c", cfg_path, "--iterations", str(iterations)]
    if name != "synthetic":
        cmd += ["--data", clips] + ARMS[name]
    t = time.perf_counter()
    out = subprocess.run(cmd, capture_output=True, text=True, timeout=limit)
    if out.returncode != 0:
        raise SystemExit("arm %s failed (%d):\n%s" % (name, out.returncode, out.stderr[-3000:]))
    rates = re.findall(r"Iteration: (\d+)/\d+ .* ([0-9.]+) frames/s", out.stdout)
    last_it, frames_s = rates[-1]
    return {"arm": name, "iterations": int(last_it) + 1, "frames_s": float(frames_s), "it_s": float(frames_s) / 8,
            "wall_s": time.perf_counter() - t}


def event_kernel():
    """ebfi_event_augment on one 16 x 2 x 256 x 256 item cut from the transposed view of a 720 x 1280 stack."""
    import torch
    from ebfi_amd import _native as N
    from ebfi_amd.eventaug import augment_events, noise_table
    stack = torch.poisson(torch.full((2, 16, 720, 1280), 0.3, device="cuda")).transpose(0, 1)
    out = []
    for what, table, j in (("no noise", (), 512), ("std 1.0 fraction 0.05", noise_table(1.0, 0.05), 512),
                           ("std 1.0 fraction 0.05, odd column", noise_table(1.0, 0.05), 513)):
        fn = lambda: augment_events(stack, (200, j, 256, 256), True, False, 126, table)
        for _ in range(5):
            fn()
        torch.cuda.synchronize()
        N.prof_reset()
        N.prof_enable(True)
        for _ in range(100):
            fn()
        torch.cuda.synchronize()
        N.prof_enable(False)
        n, ms, _, by = N.prof_collect()["event_augment"]
        us = 1e3 * ms / n
        out.append({"what": what, "us": us, "bytes": by / n, "gbs": by / n / us * 1e-3, "hbm": by / n / us * 1e-3 / HBM_GBS})
    return out


def kernel():
    import torch
    from ebfi_amd import _native as N
    from ebfi_amd.frameio import period_to_planar
    rows = torch.randint(0, 256, (16, 256, 1280, 3), dtype=torch.uint8).cuda()          # one item's staged rows
    out = []
    for j in (512, 513):                                                                 # dword loads / byte loads
        fn = lambda: period_to_planar(rows, 12, window=(0, j, 256, 256), reverse_channels=True, flip_h=True)
        for _ in range(5):
            fn()
        torch.cuda.synchronize()
        N.prof_reset()
        N.prof_enable(True)
        for _ in range(100):
            fn()
        torch.cuda.synchronize()
        N.prof_enable(False)
        n, ms, _, by = N.prof_collect()["period_frames_u8"]
        us = 1e3 * ms / n
        out.append({"j": j, "us": us, "bytes": by / n, "gbs": by / n / us * 1e-3, "hbm": by / n / us * 1e-3 / HBM_GBS})
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--work", required=True)
    ap.add_argument("--iterations", type=int, default=320)
    ap.add_argument("--arms", default="host,device,default,synthetic")
    ap.add_argument("--tree", default=None)
    ap.add_argument("--kernel", action="store_true")
    ap.add_argument("--limit", type=float, default=420.0, help="seconds per arm")
    args = ap.parse_args()
    clips, cfg_path, noise_path = setup(args.work)
    print("| arm | iterations | frames/s | iterations/s | wall s |\n|---|---|---|---|---|", flush=True)
    for name in [a for a in args.arms.split(",") if a]:
        tree = args.tree if name == "other" else ROOT
        r = run_arm(name, tree, noise_path if name in NOISE_ARMS else cfg_path, clips, args.iterations, args.limit)
        print("| %(arm)s | %(iterations)d | %(frames_s).1f | %(it_s).2f | %(wall_s).0f |" % r, flush=True)
    if args.kernel:
        print("\n| window column | us per item | bytes | GB/s | of %.0f GB/s |\n|---|---|---|---|---|" % HBM_GBS)
        for r in kernel():
            print("| %(j)d | %(us).1f | %(bytes).0f | %(gbs).0f | %(hbm).3f |" % r, flush=True)
        print("\n| event kernel | us per item | bytes | GB/s | of %.0f GB/s |\n|---|---|---|---|---|" % HBM_GBS)
        for r in event_kernel():
            print("| %(what)s | %(us).1f | %(bytes).0f | %(gbs).0f | %(hbm).3f |" % r, flush=True)


if __name__ == "__main__":
    main()
