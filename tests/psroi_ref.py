"""Deformable PS-ROI pooling restated in numpy, parametrised by dtype (the law of include/ebfi_hip.h, section
"DCNv2 deformable PS-ROI pooling").

Every operation rounds in `dtype`.  With float64 this is the oracle the device values are held against; with float32 it
is the position law itself: which samples are included and on which corners they land, hence `count`, is what the
kernels must reproduce exactly.  The parameters `spatial_scale` and `trans_std` reach the kernels as fp32 numbers, so
both dtypes start from their fp32 values, and the 0.1 of the minimum ROI extent is float32(0.1) in both.

geometry()  -> Geometry: per sample inclusion, floor / ceil corners, dx, dy  (arrays [R, nc, P, P, spp, spp])
forward()   -> (out, count)                 [R, D, P, P]
backward()  -> (grad_input, grad_trans)     [B, C, H, W], shape of trans
"""
import collections

import numpy as np

Geometry = collections.namedtuple(
    "Geometry", "inc x0 x1 y0 y1 dx dy w h batch valid rw rh part_h part_w gh gw")


def c_round(v):
    """C round(): half away from zero (numpy's round is half to even).  Exact: v - trunc(v) is."""
    t = np.trunc(v)
    return t + np.where(np.abs(v - t) >= 0.5, np.copysign(np.ones_like(v), v), np.zeros_like(v))


def _params(dtype, spatial_scale, trans_std):
    f = np.dtype(dtype).type
    return f, f(np.float32(spatial_scale)), f(np.float32(trans_std))


def geometry(rois, trans, B, H, W, spatial_scale, pooled_size, part_size, sample_per_part, trans_std, group_size=1,
             no_trans=False, dtype=np.float64):
    f, scale, tstd = _params(dtype, spatial_scale, trans_std)
    P, part, spp, G = int(pooled_size), int(part_size), int(sample_per_part), int(group_size)
    rois = np.asarray(rois).astype(f)
    R = rois.shape[0]
    nc = 1 if no_trans else np.asarray(trans).shape[1] // 2
    half, one, zero = f(0.5), f(1), f(0)
    with np.errstate(invalid="ignore", over="ignore"):
        bi = rois[:, 0]
        valid = (bi >= 0) & (bi < B) & (bi == np.floor(bi))
        batch = np.where(valid, bi, zero).astype(np.int64)
        sw = c_round(rois[:, 1]) * scale - half
        sh = c_round(rois[:, 2]) * scale - half
        ew = (c_round(rois[:, 3]) + one) * scale - half
        eh = (c_round(rois[:, 4]) + one) * scale - half
        rw = np.fmax(ew - sw, f(np.float32(0.1)))
        rh = np.fmax(eh - sh, f(np.float32(0.1)))
        bw, bh = rw / f(P), rh / f(P)
        sbw, sbh = bw / f(spp), bh / f(spp)
        p = np.arange(P).astype(f)
        part_of = np.floor(p / f(P) * f(part)).astype(np.int64)                     # [P], for rows and columns alike
        g_of = np.clip(np.floor(p * f(G) / f(P)).astype(np.int64), 0, G - 1)
        if no_trans:
            tx = ty = np.zeros((R, 1, P, P), f)
        else:
            t = np.asarray(trans).astype(f)[:R].reshape(R, nc, 2, part, part)
            tx = t[:, :, 0][:, :, part_of[:, None], part_of[None, :]] * tstd        # [R, nc, P(ph), P(pw)]
            ty = t[:, :, 1][:, :, part_of[:, None], part_of[None, :]] * tstd
        r4 = lambda v: v[:, None, None, None]
        w0 = p[None, None, None, :] * r4(bw) + r4(sw)
        w0 = w0 + tx * r4(rw)
        h0 = p[None, None, :, None] * r4(bh) + r4(sh)
        h0 = h0 + ty * r4(rh)
        i = np.arange(spp).astype(f)
        r6 = lambda v: v[:, None, None, None, None, None]
        w = w0[..., None, None] + i[None, None, None, None, None, :] * r6(sbw)      # [R, nc, ph, pw, ih, iw]
        h = h0[..., None, None] + i[None, None, None, None, :, None] * r6(sbh)
        w, h = np.broadcast_arrays(w, h)
        skip = (w < -half) | (w > f(W) - half) | (h < -half) | (h > f(H) - half)
        inc = ~skip & r6(valid)
        wc = np.fmin(np.fmax(w, zero), f(W) - one)
        hc = np.fmin(np.fmax(h, zero), f(H) - one)
        fw, fh = np.floor(wc), np.floor(hc)
        return Geometry(inc, fw.astype(np.int64), np.ceil(wc).astype(np.int64), fh.astype(np.int64),
                        np.ceil(hc).astype(np.int64), wc - fw, hc - fh, w, h, batch, valid, rw, rh,
                        part_of, part_of, g_of, g_of)


def _expand(geo, inp, D, G, nc):
    """Per output element and sample: the four corner values and the index arrays, all [R, D, P, P, spp, spp]."""
    cls = np.arange(D) // (D // nc)
    sel = lambda a: a[:, cls]
    inc, x0, x1, y0, y1, dx, dy = (sel(a) for a in (geo.inc, geo.x0, geo.x1, geo.y0, geo.y1, geo.dx, geo.dy))
    chan = (np.arange(D)[:, None, None] * G + geo.gh[None, :, None]) * G + geo.gw[None, None, :]      # [D, ph, pw]
    chan = np.broadcast_to(chan[None, :, :, :, None, None], inc.shape)
    b = np.broadcast_to(geo.batch[:, None, None, None, None, None], inc.shape)
    # a sample that is not included reads pixel 0 and is dropped below
    z = lambda a: np.where(inc, a, 0)
    x0, x1, y0, y1 = z(x0), z(x1), z(y0), z(y1)
    U = [inp[b, chan, yy, xx] for yy, xx in ((y0, x0), (y1, x0), (y0, x1), (y1, x1))]               # U00 U01 U10 U11
    return inc, (b, chan, x0, x1, y0, y1), dx, dy, U


def forward(inp, rois, trans, spatial_scale, pooled_size, output_dim, group_size, part_size, sample_per_part, trans_std,
            no_trans=False, dtype=np.float64):
    f = np.dtype(dtype).type
    inp = np.asarray(inp).astype(f)
    B, C, H, W = inp.shape
    D, G, spp = int(output_dim), int(group_size), int(sample_per_part)
    assert C == D * G * G
    geo = geometry(rois, trans, B, H, W, spatial_scale, pooled_size, part_size, spp, trans_std, G, no_trans, dtype)
    nc = geo.inc.shape[1]
    assert D % nc == 0
    inc, _, dx, dy, (U00, U01, U10, U11) = _expand(geo, inp, D, G, nc)
    one = f(1)
    with np.errstate(invalid="ignore", over="ignore"):
        val = (one - dx) * (one - dy) * U00 + (one - dx) * dy * U01 + dx * (one - dy) * U10 + dx * dy * U11
        val = np.where(inc, val, f(0))
        total = np.zeros(inc.shape[:4], f)
        for ih in range(spp):
            for iw in range(spp):
                total = total + val[..., ih, iw]
        count = inc.sum(axis=(4, 5)).astype(f)
        out = np.where(count > 0, total / np.where(count > 0, count, one), f(0))
    return out, count


def backward(grad_out, inp, rois, trans, spatial_scale, pooled_size, output_dim, group_size, part_size, sample_per_part,
             trans_std, no_trans=False, dtype=np.float64):
    f, _, tstd = _params(dtype, spatial_scale, trans_std)
    inp = np.asarray(inp).astype(f)
    go = np.asarray(grad_out).astype(f)
    B, C, H, W = inp.shape
    D, G, spp = int(output_dim), int(group_size), int(sample_per_part)
    geo = geometry(rois, trans, B, H, W, spatial_scale, pooled_size, part_size, spp, trans_std, G, no_trans, dtype)
    nc = geo.inc.shape[1]
    inc, (b, chan, x0, x1, y0, y1), dx, dy, (U00, U01, U10, U11) = _expand(geo, inp, D, G, nc)
    one, zero = f(1), f(0)
    count = inc.sum(axis=(4, 5)).astype(f)
    dv = np.where(count > 0, go / np.where(count > 0, count, one), zero)[..., None, None]
    grad_in = np.zeros_like(inp)
    with np.errstate(invalid="ignore", over="ignore"):
        for q, yy, xx in (((one - dx) * (one - dy), y0, x0), ((one - dx) * dy, y1, x0), (dx * (one - dy), y0, x1),
                          (dx * dy, y1, x1)):
            np.add.at(grad_in, (b, chan, yy, xx), np.where(inc, q * dv, zero))
        if no_trans:
            return grad_in, np.zeros(0, f)
        grad_trans = np.zeros(np.asarray(trans).shape, f)
        r6 = lambda v: v[:, None, None, None, None, None]
        diff_x = (U11 * dy + U10 * (one - dy) - U01 * dy - U00 * (one - dy)) * tstd * dv * r6(geo.rw)
        diff_y = (U11 * dx + U01 * (one - dx) - U10 * dx - U00 * (one - dx)) * tstd * dv * r6(geo.rh)
        R = inc.shape[0]
        cls = np.arange(D) // (D // nc)
        n = np.broadcast_to(np.arange(R)[:, None, None, None, None, None], inc.shape)
        c2 = np.broadcast_to(2 * cls[None, :, None, None, None, None], inc.shape)
        ph = np.broadcast_to(geo.part_h[None, None, :, None, None, None], inc.shape)
        pw = np.broadcast_to(geo.part_w[None, None, None, :, None, None], inc.shape)
        np.add.at(grad_trans, (n, c2, ph, pw), np.where(inc, diff_x, zero))
        np.add.at(grad_trans, (n, c2 + 1, ph, pw), np.where(inc, diff_y, zero))
    return grad_in, grad_trans
