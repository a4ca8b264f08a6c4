"""The fixtures of the deformable PS-ROI pooling tests, shared by the CPU tests (which assert that the float32 and float64
geometry agree on them) and the GPU tests (which hold the kernels against both).  Seeded random ROIs and offsets plus the
named special ROIs; everything is float32 data, generated once per process."""
import collections
import functools

import numpy as np

Case = collections.namedtuple(
    "Case", "name B D G H W R P part spp nc scale trans_std no_trans inp rois trans")

_SHAPES = {
    # name: (B, D, G, H, W, R, P, part, spp, nc, scale, trans_std, extra trans rows, seed, special ROIs)
    "A": (2, 3, 1, 5, 5, 4, 3, 3, 4, 1, 1.0 / 4, 0.1, 0, 4, ()),
    "B": (2, 8, 1, 9, 12, 6, 7, 7, 4, 2, 1.0 / 4, 0.1, 3, 12,
          ((0, 200, 200, 230, 230), (1, 10, 6, 10, 6), (0, 2.5, 3.5, 20.5, 17.5), (1, -30, -20, 9, 11))),
    "C": (1, 2, 2, 8, 8, 5, 4, 2, 2, 1, 1.0 / 2, 0.2, 0, 13, ((0, 0, 0, 15, 15),)),
    "D": (1, 6, 1, 7, 11, 5, 5, 3, 3, 3, 1.0 / 3, 0.3, 0, 7, ((0, -9, 4, 40, 12),)),
}

# fixture E: B's shape, no offsets, dyadic ROIs (extent 7 or 14 map pixels: sub-bins of 1/4 and 1/2), so that samples sit
# exactly on -0.5, on W - 0.5 = 11.5 / H - 0.5 = 8.5 and on integer coordinates, in float32 and float64 alike
_E_ROIS = ((0, 0, 0, 27, 27), (1, 0, 0, 55, 55), (0, 20, 8, 47, 35), (1, 4, 4, 31, 59), (0, 8, 0, 63, 27),
           (1, 2, 2, 29, 29))

NAMES = ("A", "B", "C", "D", "E")


@functools.lru_cache(maxsize=None)
def case(name):
    if name == "E":
        b = case("B")
        return b._replace(name="E", no_trans=True, nc=1, rois=np.array(_E_ROIS, np.float32), trans=None)
    B, D, G, H, W, R, P, part, spp, nc, scale, tstd, extra, seed, special = _SHAPES[name]
    rng = np.random.RandomState(seed)
    nrand = R - len(special)
    ext = W / scale                                      # the image extent the map stands for
    xy = rng.rand(nrand, 2) * 0.75 * ext
    wh = rng.rand(nrand, 2) * 0.5 * ext
    rnd = np.concatenate([rng.randint(0, B, (nrand, 1)).astype(np.float64), xy, xy + wh], axis=1)
    rois = np.concatenate([np.array(special, np.float64).reshape(-1, 5), rnd]).astype(np.float32)
    inp = rng.randn(B, D * G * G, H, W).astype(np.float32)
    trans = rng.randn(R + extra, 2 * nc, part, part).astype(np.float32)
    for a in (inp, rois, trans):
        a.setflags(write=False)
    return Case(name, B, D, G, H, W, R, P, part, spp, nc, scale, tstd, False, inp, rois, trans)


def law_args(c):
    """The positional tail shared by psroi_ref.forward / backward after (inp, rois, trans)."""
    return (c.scale, c.P, c.D, c.G, c.part, c.spp, c.trans_std)
