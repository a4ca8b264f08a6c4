"""Deformable PS-ROI pooling without a GPU: the numpy restatement pinned against itself and against finite differences,
the agreement of its float32 and float64 geometry on the committed fixtures, and the host contract of the new entry
points, ops and modules."""
import ctypes

import numpy as np
import pytest
import torch

import psroi_cases as K
import psroi_ref as R
from ebfi_amd import _native as N
from ebfi_amd import dcn

F32, F64 = np.float32, np.float64


def _rand(seed, *shape):
    return np.random.RandomState(seed).randn(*shape)


# ------------------------------------------------------------------ the restatement pins itself
@pytest.mark.parametrize("dtype", [F32, F64])
@pytest.mark.parametrize("name", ["A", "B", "C", "D"])
def test_constant_input_pools_to_the_constant(name, dtype):
    """Up to the roundings of the law itself: the four weights of a sample are products of rounded (1 - dx), (1 - dy) and
    their three adds round (under 6 half-ulps on the sample), then at most 15 adds and one division (16 more): 11 ulps
    bound the relative error of a bin, 16 are allowed.  (It is exact on most bins; not on all of them in float32.)"""
    c = K.case(name)
    tol = 16 * np.finfo(dtype).eps
    for value in (1.0, 0.75, -3.0):
        out, count = R.forward(np.full(c.inp.shape, value), c.rois, c.trans, *K.law_args(c), dtype=dtype)
        assert (count > 0).any() and (count == 0).any()
        assert np.abs(out[count > 0] - value).max() <= tol * abs(value)
        assert (out[count == 0] == 0).all()


def test_linear_ramp_gives_the_mean_coordinates():
    """Bilinear interpolation is exact on a*x + b*y, so a bin is a*mean(w) + b*mean(h): the coordinates of steps 1-7,
    written out here with scalars and a non-zero trans, independently of geometry()."""
    B, H, W, P, part, spp, scale, tstd, a, b = 1, 40, 48, 3, 3, 4, 0.25, 0.1, 0.5, -0.25
    rois = np.array([[0, 33.0, 41.0, 110.0, 97.0], [0, 50.5, 30.5, 81.5, 120.5]])
    trans = _rand(3, 2, 2, part, part)
    ys, xs = np.meshgrid(np.arange(H, dtype=F64), np.arange(W, dtype=F64), indexing="ij")
    inp = (a * xs + b * ys)[None, None]
    out, count = R.forward(inp, rois, trans, scale, P, 1, 1, part, spp, tstd, dtype=F64)
    assert (count == spp * spp).all()          # all samples inside: no clamping, which would bend the ramp
    ts = float(np.float32(tstd))
    for n, (_, x1, y1, x2, y2) in enumerate(rois):
        rnd = lambda v: np.floor(v + 0.5)      # (positive coordinates here)
        sw, sh = rnd(x1) * scale - 0.5, rnd(y1) * scale - 0.5
        rw, rh = (rnd(x2) + 1) * scale - 0.5 - sw, (rnd(y2) + 1) * scale - 0.5 - sh
        for ph in range(P):
            for pw in range(P):
                w0 = pw * rw / P + sw + trans[n, 0, ph, pw] * ts * rw
                h0 = ph * rh / P + sh + trans[n, 1, ph, pw] * ts * rh
                mw = np.mean([w0 + i * rw / P / spp for i in range(spp)])
                mh = np.mean([h0 + i * rh / P / spp for i in range(spp)])
                assert abs(out[n, 0, ph, pw] - (a * mw + b * mh)) < 1e-12


@pytest.mark.parametrize("dtype", [F32, F64])
@pytest.mark.parametrize("name", ["A", "B", "C", "D"])
def test_zero_trans_is_no_trans_bit_for_bit(name, dtype):
    c = K.case(name)
    o0, c0 = R.forward(c.inp, c.rois, np.zeros_like(c.trans), *K.law_args(c), dtype=dtype)
    o1, c1 = R.forward(c.inp, c.rois, None, *K.law_args(c), no_trans=True, dtype=dtype)
    assert np.array_equal(o0, o1) and np.array_equal(c0, c1)


def test_half_integer_corners_round_away_from_zero():
    assert R.c_round(np.array([2.5, 3.5, -2.5, -0.5, 0.49999997], F32)).tolist() == [3.0, 4.0, -3.0, -1.0, 0.0]
    assert np.round(np.array([2.5], F32))[0] == 2.0          # what half-to-even would have given
    rois = np.array([[0, 2.5, 3.5, 20.5, 17.5]], F32)
    for dtype in (F32, F64):
        g = R.geometry(rois, None, 1, 9, 12, 0.25, 7, 7, 4, 0.0, no_trans=True, dtype=dtype)
        # sw = 3 / 4 - 0.5, sh = 4 / 4 - 0.5: the first sample of bin (0, 0)
        assert g.w[0, 0, 0, 0, 0, 0] == 0.25 and g.h[0, 0, 0, 0, 0, 0] == 0.5
        assert g.rw[0] == 22 * 0.25 - 0.5 - 0.25 and g.rh[0] == 19 * 0.25 - 0.5 - 0.5


def test_bins_share_a_part_cell():
    c = K.case("C")                                          # P = 4, part = 2
    g = R.geometry(c.rois, c.trans, c.B, c.H, c.W, c.scale, c.P, c.part, c.spp, c.trans_std, c.G, dtype=F64)
    assert g.part_h.tolist() == [0, 0, 1, 1]
    # bins (0, 0) and (1, 1) read the same offset: apart by exactly one bin each way (up to the rounding of the adds)
    bw, bh = g.rw / c.P, g.rh / c.P
    assert np.allclose(g.w[:, 0, 1, 1] - g.w[:, 0, 0, 0], bw[:, None, None], rtol=0, atol=1e-12)
    assert np.allclose(g.h[:, 0, 1, 1] - g.h[:, 0, 0, 0], bh[:, None, None], rtol=0, atol=1e-12)
    # and only cell (0, 0) moves them
    t2 = c.trans.copy()
    t2[:, :, 0, 0] += 1.0
    g2 = R.geometry(c.rois, t2, c.B, c.H, c.W, c.scale, c.P, c.part, c.spp, c.trans_std, c.G, dtype=F64)
    moved = (g2.w != g.w) | (g2.h != g.h)
    assert moved[:, :, :2, :2].all() and not moved[:, :, 2:, :].any() and not moved[:, :, :, 2:].any()
    # the gradient of that cell collects both bins
    go = _rand(5, c.R, c.D, c.P, c.P)
    _, gt = R.backward(go, c.inp, c.rois, c.trans, *K.law_args(c), dtype=F64)
    for keep in ((0, 0), (1, 1)):
        one = np.zeros_like(go)
        one[:, :, keep[0], keep[1]] = go[:, :, keep[0], keep[1]]
        _, part_gt = R.backward(one, c.inp, c.rois, c.trans, *K.law_args(c), dtype=F64)
        assert np.abs(part_gt[:, :, 0, 0]).max() > 0 and np.abs(part_gt[:, :, 1, 1]).max() == 0
    assert np.abs(gt[:, :, 0, 0]).max() > 0


def test_zero_width_roi_is_a_tenth_wide():
    rois = np.array([[0, 10, 6, 9, 5]], F32)                # ew - sw = 0 exactly: (9 + 1) * s - 0.5 - (10 * s - 0.5)
    for dtype in (F32, F64):
        g = R.geometry(rois, None, 1, 9, 12, 0.25, 7, 7, 4, 0.0, no_trans=True, dtype=dtype)
        assert g.rw.dtype == dtype and g.rw[0] == dtype(np.float32(0.1)) and g.rh[0] == dtype(np.float32(0.1))


def test_batch_index_outside_the_batch_pools_nothing():
    c = K.case("B")
    rois = c.rois.copy()
    rois[2:6, 0] = [c.B, -1, 0.5, np.nan]
    out, count = R.forward(c.inp, rois, c.trans, *K.law_args(c), dtype=F64)
    assert (out[2:6] == 0).all() and (count[2:6] == 0).all()
    gi, gt = R.backward(np.ones_like(out), c.inp, rois, c.trans, *K.law_args(c), dtype=F64)
    assert (gt[2:6] == 0).all() and np.isfinite(gi).all()


# ------------------------------------------------------------------ float64 backward against finite differences
def test_float64_backward_matches_central_differences():
    """The reference's gradient-check shape (testcuda.py:134-166) with trans_std = 0.1: at its 0.0 the trans gradient is
    identically zero.  Elements whose perturbation changes a sample's inclusion, floor or ceil are left out: the law is
    not differentiable there (and defines its own value)."""
    c = K.case("A")
    inp = c.inp.astype(F64) * 0.01
    trans = c.trans.astype(F64)
    args = K.law_args(c)
    go = _rand(7, c.R, c.D, c.P, c.P)
    gi, gt = R.backward(go, inp, c.rois, trans, *args, dtype=F64)
    loss = lambda i, t: float((R.forward(i, c.rois, t, *args, dtype=F64)[0] * go).sum())
    geo = lambda t: R.geometry(c.rois, t, c.B, c.H, c.W, c.scale, c.P, c.part, c.spp, c.trans_std, c.G, dtype=F64)
    same = lambda g, h: all(np.array_equal(getattr(g, k), getattr(h, k)) for k in ("inc", "x0", "x1", "y0", "y1"))
    step = 1e-6

    fd_i = np.zeros_like(inp)
    for idx in np.ndindex(*inp.shape):                       # the input moves no sample: every element is checked
        p, m = inp.copy(), inp.copy()
        p[idx] += step
        m[idx] -= step
        fd_i[idx] = (loss(p, trans) - loss(m, trans)) / (2 * step)
    err_i = np.abs(fd_i - gi).max() / np.abs(fd_i).max()

    g0, fd_t, checked = geo(trans), np.zeros_like(trans), np.zeros(trans.shape, bool)
    for idx in np.ndindex(*trans.shape):
        p, m = trans.copy(), trans.copy()
        p[idx] += step
        m[idx] -= step
        if same(geo(p), g0) and same(geo(m), g0):
            checked[idx] = True
            fd_t[idx] = (loss(inp, p) - loss(inp, m)) / (2 * step)
    assert checked.sum() >= checked.size // 2
    err_t = np.abs(fd_t - gt)[checked].max() / np.abs(fd_t[checked]).max()
    print("finite differences: grad_input %.3e, grad_trans %.3e (%d of %d cells)" % (err_i, err_t, checked.sum(), checked.size))
    assert np.abs(gt).max() > 0 and np.abs(gi).max() > 0
    assert err_i < 1e-6 and err_t < 1e-6


# ------------------------------------------------------------------ the fixtures
@pytest.mark.parametrize("name", K.NAMES)
def test_fixture_geometry_agrees_in_float32_and_float64(name):
    """What lets the GPU tests hold fp32 kernels against the float64 oracle: on the committed seeds no sample changes its
    inclusion or its corners between the two precisions.  Each fixture has empty, partial and full bins."""
    c = K.case(name)
    g32, g64 = (R.geometry(c.rois, c.trans, c.B, c.H, c.W, c.scale, c.P, c.part, c.spp, c.trans_std, c.G, c.no_trans, d)
                for d in (F32, F64))
    for k in ("inc", "x0", "x1", "y0", "y1"):
        a, b = getattr(g32, k), getattr(g64, k)
        if k != "inc":                                       # corners matter where the sample is included
            a, b = np.where(g32.inc, a, 0), np.where(g64.inc, b, 0)
        assert np.array_equal(a, b), k
    count = g32.inc.sum(axis=(4, 5))
    full = c.spp * c.spp
    assert (count == 0).any() and (count == full).any() and ((count > 0) & (count < full)).any()


def test_fixture_e_puts_samples_on_the_boundaries():
    c = K.case("E")
    g = R.geometry(c.rois, None, c.B, c.H, c.W, c.scale, c.P, c.part, c.spp, c.trans_std, c.G, True, F32)
    on = lambda a, v: ((a == v) & g.inc).any()
    assert on(g.w, -0.5) and on(g.h, -0.5) and on(g.w, c.W - 0.5) and on(g.h, c.H - 0.5)
    assert ((g.dx == 0) & (g.w > 0) & (g.w < c.W - 1) & g.inc).any()
    assert ((g.w > c.W - 0.5) & ~g.inc).any()


# ------------------------------------------------------------------ host contract
def test_argument_errors_do_not_touch_the_gpu():
    """Every device pointer is the address 8: a call that got past its checks would fault."""
    lib = N.lib()
    fake, ERR_ARG = ctypes.c_void_p(8), N.CONSTANTS["EBFI_ERR_ARG"]

    def fwd(inp=fake, rois=fake, trans=fake, out=fake, count=fake, B=2, C=8, H=9, W=12, R=6, nc=2, no_trans=0, D=8, G=1,
            P=7, part=7, spp=4, dtype=N.EBFI_F32):
        return lib.ebfi_dcn_pooling_forward(inp, rois, trans, out, count, B, C, H, W, R, nc, no_trans, 0.25, D, G, P, part,
                                            spp, 0.1, dtype, None)

    def bwd(go=fake, inp=fake, rois=fake, trans=fake, count=fake, gi=fake, gt=fake, Rt=9, B=2, C=8, H=9, W=12, R=6, nc=2,
            no_trans=0, D=8, G=1, P=7, part=7, spp=4, dtype=N.EBFI_F32):
        return lib.ebfi_dcn_pooling_backward(go, inp, rois, trans, count, gi, gt, Rt, B, C, H, W, R, nc, no_trans, 0.25, D,
                                             G, P, part, spp, 0.1, dtype, None)

    for call in (fwd, bwd):
        assert call(inp=None) == ERR_ARG and b"null" in lib.ebfi_last_error()
        assert call(rois=None) == ERR_ARG and call(trans=None) == ERR_ARG
        for size in ("B", "C", "H", "W", "nc", "D", "G", "P", "part", "spp"):
            assert call(**{size: 0}) == ERR_ARG, size
        assert call(R=-1) == ERR_ARG
        assert call(C=9) == ERR_ARG and b"group_size" in lib.ebfi_last_error()
        assert call(G=2) == ERR_ARG                          # C must be D * G * G = 32
        assert call(nc=3) == ERR_ARG and b"classes" in lib.ebfi_last_error()
        assert call(dtype=N.EBFI_F32_BF16X3MMA) == ERR_ARG
        assert call(R=0) == 0                                # no-op: nothing is launched
    assert fwd(out=None) == ERR_ARG
    assert bwd(go=None) == ERR_ARG and bwd(count=None) == ERR_ARG and bwd(gi=None) == ERR_ARG and bwd(gt=None) == ERR_ARG
    assert bwd(Rt=5) == ERR_ARG


def test_cpu_tensors_are_refused():
    x, rois, off = torch.zeros(1, 4, 6, 6), torch.tensor([[0.0, 0, 0, 8, 8]]), torch.zeros(1, 2, 3, 3)
    with pytest.raises(NotImplementedError):
        dcn.dcn_v2_pooling(x, rois, off, 0.5, 3, 4, False, 1, 3, 4, 0.1)
    with pytest.raises(NotImplementedError):
        dcn.dcn_v2_pooling_forward(x, rois, x.new(), True, 0.5, 4, 1, 3, 3, 4, 0.0)
    with pytest.raises(NotImplementedError):
        dcn.dcn_v2_pooling_backward(torch.zeros(1, 4, 3, 3), x, rois, off, torch.zeros(1, 4, 3, 3), False, 0.5, 4, 1, 3, 3,
                                    4, 0.1)
    with pytest.raises(NotImplementedError):
        dcn.DCNv2Pooling(0.5, 3, 4, True)(x, rois, off)
    with pytest.raises(AssertionError):                      # the module check: C == output_dim * group_size ** 2
        dcn.DCNv2Pooling(0.5, 3, 4, True, group_size=2)(x, rois, off)


def test_the_shim_exports_the_pooling_names():
    import models.DCNv2.dcn_v2 as shim
    for name in ("_DCNv2Pooling", "dcn_v2_pooling", "DCNv2Pooling", "DCNPooling", "dcn_v2_pooling_forward",
                 "dcn_v2_pooling_backward", "DCN", "DCN_sep", "DCNv2", "_DCNv2", "dcn_v2_conv"):
        assert getattr(shim, name) is getattr(dcn, name)
    assert shim.dcn_v2_pooling == dcn._DCNv2Pooling.apply


def test_dcnpooling_parameters_follow_the_reference():
    m = dcn.DCNPooling(spatial_scale=0.25, pooled_size=7, output_dim=4, no_trans=False, trans_std=0.1, deform_fc_dim=32)
    assert sorted(m.state_dict()) == sorted("offset_mask_fc.%d.%s" % (i, p) for i in (0, 2, 4) for p in ("weight", "bias"))
    assert m.offset_mask_fc[0].weight.shape == (32, 7 * 7 * 4) and m.offset_mask_fc[4].weight.shape == (7 * 7 * 3, 32)
    assert not m.offset_mask_fc[4].weight.any() and not m.offset_mask_fc[4].bias.any()
    assert m.offset_mask_fc[0].weight.any()
    assert m.part_size == 7 and m.sample_per_part == 4 and m.group_size == 1
    plain = dcn.DCNPooling(spatial_scale=0.25, pooled_size=7, output_dim=4, no_trans=True)
    assert not hasattr(plain, "offset_mask_fc") and not plain.state_dict()
    assert dcn.DCNPooling(0.25, 7, 4, False).deform_fc_dim == 1024
