#!/usr/bin/env python3
"""The two weight-pack launches of a training step (ebfi_pack_table_bf16 / ebfi_pack_table_f16) on the bank of the default
model, library event pairs, plus sha1 digests of both packed buffers so that two builds can be compared bit for bit
(EBFI_DEV=1 EBFI_LIB_PATH=<other build> for the other arm).  usage: python tools/packbench.py"""
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
