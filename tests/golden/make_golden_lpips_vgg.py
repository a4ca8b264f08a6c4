#!/usr/bin/env python3
"""Writes tests/golden/lpips_vgg_v01_lin.npz: the five LPIPS v0.1 linear heads of the VGG-16 variant, as plain float32 arrays
`lin0` .. `lin4` of shapes [64], [128], [256], [512], [512] (the `lin{l}.model.1.weight` tensors [1, C, 1, 1] of the reference's
loss/PerceptualSimilarity/models/weights/v0.1/vgg.pth, flattened).  The .pth is a pickle and is not committed; this file holds
data only.  1472 numbers.  The VGG-16 trunk is not stored: the tests draw a seeded random one.

    python tests/golden/make_golden_lpips_vgg.py <reference checkout>
"""
import os
import sys

import numpy as np
import torch

HERE = os.path.dirname(os.path.abspath(__file__))


def main(ref):
    path = os.path.join(ref, "loss", "PerceptualSimilarity", "models", "weights", "v0.1", "vgg.pth")
    sd = torch.load(path, map_location="cpu", weights_only=True)
    out = {}
    for l, c in enumerate((64, 128, 256, 512, 512)):
        w = sd["lin%d.model.1.weight" % l]
        assert tuple(w.shape) == (1, c, 1, 1), (l, tuple(w.shape))
        out["lin%d" % l] = w.reshape(-1).to(torch.float32).numpy()
    dst = os.path.join(HERE, "lpips_vgg_v01_lin.npz")
    np.savez(dst, **out)
    print("wrote", dst, {k: v.shape for k, v in out.items()})


if __name__ == "__main__":
    if len(sys.argv) != 2:
        raise SystemExit(__doc__)
    main(sys.argv[1])
