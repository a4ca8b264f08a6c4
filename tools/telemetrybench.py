"""Device time of ebfi_segment_stats on the 5.7 M-element flat buffers of the full model (parameter groups at depth 2): device
events around one call (three launches), 20 repetitions after 3 warm-up calls.  Numbers: profiles/telemetry.md."""
import os, sys
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "ebfi-be_amd"))
import torch
from ebfi_amd import telemetry
from ebfi_amd.engine import DEFAULT_MODEL_ARGS
from ebfi_amd.model import EVFIAutoEx

net = EVFIAutoEx(**DEFAULT_MODEL_ARGS)
named = [(n, p) for n, p in net.named_parameters() if p.requires_grad]
names, offsets = telemetry.parameter_groups(named, 2)
n = offsets[-1]
print("elements", n, "segments", len(names))
for label, flat in (("weights-like (x0.1 init)", torch.cat([p.detach().reshape(-1) for _, p in named]).cuda()),
                    ("gradient-like (normal x 1e-4)", torch.randn(n, device="cuda") * 1e-4),
                    ("all zero (one bin)", torch.zeros(n, device="cuda"))):
    st = telemetry.SegmentStats(offsets, n, "cuda")
    for _ in range(3):
        st.run(flat)
    torch.cuda.synchronize()
    times = []
    for _ in range(20):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record(); st.run(flat); b.record(); b.synchronize()
        times.append(a.elapsed_time(b))
    times.sort()
    print("%-32s median %.3f ms  min %.3f  max %.3f  (%.0f GB/s at the median)" % (label, times[10], times[0], times[-1], n * 4 / times[10] / 1e6))
