#!/usr/bin/env python3
"""Golden fixture for ebfi_amd.unet at kernel_size=5, the reference's default: RUNS THE REFERENCE'S OWN
models/model_misc/unet.py on the CPU in float64 and stores what it returned.

    python tests/golden/make_unet_k5_golden.py <path of the reference checkout>     # rewrites tests/golden/unet_k5_small.npz

tests/golden/make_unet_golden.py with tests/unet_ref.py's CFG["kernel_size"] set to 5 for the run: the same import of the
reference's three files by path, the same five CASES, two carried calls and one backward per case, weights from
unet_ref.fill_state(seed, case) and inputs from unet_ref.make_inputs(seed + 1000, case), the same entries per case (X_names,
X_shapes, X_out, X_states, X_grads) and `seeds` [5].  Only data is written; the file stays under 300 KiB.

The seed of a case is searched over 1 .. 64 for the widest margin between the smallest ReLU pre-activation of both calls and
zero (tests/test_conv5x5_host.py asserts a margin >= 1e-5 and no ReLU mask flipped by float32 for the stored seeds).
"""
import os
import sys

import numpy as np
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
OUT = os.path.join(HERE, "unet_k5_small.npz")
sys.path.insert(0, os.path.dirname(HERE))
sys.path.insert(0, HERE)
import unet_ref as R  # noqa: E402
from make_unet_golden import import_reference, margin  # noqa: E402

SEEDS = range(1, 65)


def main(ref):
    R.CFG["kernel_size"] = 5
    unet = import_reference(ref)
    out, seeds = {}, []
    for case in R.CASES:
        seed = max(SEEDS, key=lambda s: margin(case, s))
        torch.manual_seed(0)
        net = getattr(unet, R.CASES[case]["net"])(R.unet_kwargs(case)).double()
        sd = net.state_dict()
        expect = R.names_and_shapes(case)
        assert [(k, tuple(v.shape)) for k, v in sd.items()] == expect, "the restatement's name list differs from the reference's"
        net.load_state_dict(R.fill_state(seed, case))
        xs, cots = R.make_inputs(seed + 1000, case)
        outs = [R.module_outputs(net(x)) for x in xs]
        loss = sum((c * o).sum() for c, o in zip(cots, outs))
        params = dict(net.named_parameters())
        grads = torch.autograd.grad(loss, [params[n] for n, _ in expect])
        seeds.append(seed)
        out[case + "_names"] = np.array([n for n, _ in expect])
        out[case + "_shapes"] = np.array([str(tuple(s)) for _, s in expect])
        out[case + "_out"] = np.stack([o.detach().numpy() for o in outs])
        out[case + "_states"] = np.concatenate([s.detach().numpy().reshape(-1) for s in R.flat_states(net.states)])
        out[case + "_grads"] = R.grad_table(grads)
        print("case %s: seed %d, margin %.3g, out %s" % (case, seed, margin(case, seed), out[case + "_out"].shape))
    out["seeds"] = np.array(seeds)
    assert all(np.isfinite(v).all() for k, v in out.items() if v.dtype.kind == "f")
    np.savez_compressed(OUT, **out)
    print("wrote %s (%d bytes)" % (OUT, os.path.getsize(OUT)))


if __name__ == "__main__":
    if len(sys.argv) != 2:
        sys.exit(__doc__)
    main(sys.argv[1])
