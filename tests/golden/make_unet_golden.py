#!/usr/bin/env python3
"""Golden fixture for ebfi_amd.unet: RUNS THE REFERENCE'S OWN models/model_misc/unet.py (UNetFlow, UNetRecurrent,
SRUNetRecurrent over its submodules.py and model_util.py) on the CPU in float64 and stores what it returned.

    python tests/golden/make_unet_golden.py <path of the reference checkout>     # rewrites tests/golden/unet_small.npz

The three files are imported unchanged, by path, as a package of their own name (`reference_model_misc`), so that neither this
project's `models` package nor the reference's other models are touched.  Only data is written.

Every case of tests/unet_ref.py CASES makes two consecutive calls with different inputs and the recurrent state carried between
them, forms loss = sum(cot1 * out1) + sum(cot2 * out2) and runs one backward through both calls.  Weights come from
unet_ref.fill_state(seed, case) and inputs from unet_ref.make_inputs(seed + 1000, case), so the fixture carries seeds, not
tensors.  The seed of a case is searched (1 .. 24) for the widest margin between the smallest ReLU pre-activation of both calls
and zero: on an input where float32 itself flips a ReLU mask a comparison against float32's own error proves nothing.  Stored
per case X:
  X_names, X_shapes        the reference module's state-dict keys and shapes
  X_out [2, ...]           both calls' outputs (UNetFlow: cat(image, flow))
  X_states                 the final states, each flattened, one after the other (ConvLSTM: hidden then cell per encoder;
                           ConvGRU: the state)
  X_grads [P, 9]           the sum and the first 8 elements (zero-padded) of every parameter's gradient
and `seeds` [5], the seed of each case in the order of CASES.  (Few, large entries: the file stays under 300 KiB.)
"""
import importlib
import os
import sys
import types

import numpy as np
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
OUT = os.path.join(HERE, "unet_small.npz")
sys.path.insert(0, os.path.dirname(HERE))
import unet_ref as R  # noqa: E402

SEEDS = range(1, 25)


def import_reference(ref):
    pkg = types.ModuleType("reference_model_misc")
    pkg.__path__ = [os.path.join(ref, "models", "model_misc")]
    sys.modules["reference_model_misc"] = pkg
    return importlib.import_module("reference_model_misc.unet")


def margin(case, seed):
    xs, cots = R.make_inputs(seed + 1000, case)
    got = R.run(case, R.fill_state(seed, case), xs, cots)
    return min(float(p.abs().min()) for p in got["preacts"])


def main(ref):
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
