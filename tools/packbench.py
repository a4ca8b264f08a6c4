#!/usr/bin/env python3
"""The two weight-pack launches of a training step (the bf16 pair pack, profiler row pack_table_bf16, and ebfi_pack_table_f16) on
the bank of the default model with every image packed, library event pairs, plus sha1 digests of both packed buffers so that
two trees can be compared bit for bit.  --engine: also the pack of an Engine's training bank once three eager steps and the
capture have settled which bf16 images it packs (ebfi_amd.weightbank, pack_on_demand).  usage: python tools/packbench.py"""
import hashlib
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "ebfi-be_amd"))
import torch  # noqa: E402

from ebfi_amd import _native as N  # noqa: E402
from ebfi_amd import f16scale, weightbank  # noqa: E402
from ebfi_amd.engine import DEFAULT_MODEL_ARGS  # noqa: E402
from ebfi_amd.model import EVFIAutoEx  # noqa: E402

torch.manual_seed(0)
net = EVFIAutoEx(**DEFAULT_MODEL_ARGS).cuda().train()
bank = weightbank.build_for(net, fwd16="filters")
bank.attach_scale_book(f16scale.ScaleBook("cuda"))
bank.refresh()
torch.cuda.synchronize()
sha = lambda t: hashlib.sha1(t.view(torch.int16).cpu().numpy().tobytes()).hexdigest()[:16]
print("library %s" % N.LIB_PATH)
print("bf16 table %d entries, fp16 table %d entries; packed %s  packed16 %s"
      % (bank.table.numel(), bank.table16.numel(), sha(bank.packed), sha(bank.packed16)))
for _ in range(3):
    bank.refresh()
torch.cuda.synchronize()
N.prof_reset()
N.prof_enable(True)
for _ in range(20):
    bank.refresh()
torch.cuda.synchronize()
N.prof_enable(False)
for k, v in sorted(N.prof_collect().items()):
    if v[0]:
        print("  %-18s %4.1f x %7.1f us" % (k, v[0] / 20, 1e3 * v[1] / v[0]))
if "--engine" in sys.argv:
    from ebfi_amd.engine import Engine, synthetic_batch  # noqa: E402
    del bank, net
    eng = Engine(DEFAULT_MODEL_ARGS, device="cuda", precision="bf16x3", lr=1e-4, seed=123, graph=True)
    batch = synthetic_batch(8, 256, 256, DEFAULT_MODEL_ARGS.get("TB", 16), device="cuda", seed=123)
    for _ in range(eng.calibration_steps + 2):
        eng.train_step(*batch)
    torch.cuda.synchronize()
    b = eng.bank
    imgs = b.packed_images()
    print("engine bank: %d of %d bf16 images in the per-step pack, %d of %d pair entries"
          % (len(imgs), len(b._images), b._n_entries, sum(n for _, _, n in b._images.values())))
    N.prof_reset()
    N.prof_enable(True)
    for _ in range(20):
        b.refresh()
    torch.cuda.synchronize()
    N.prof_enable(False)
    for k, v in sorted(N.prof_collect().items()):
        if v[0]:
            print("  %-18s %4.1f x %7.1f us" % (k, v[0] / 20, 1e3 * v[1] / v[0]))
