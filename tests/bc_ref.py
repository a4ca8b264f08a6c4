"""The law of ebfi_amd.bcloss (BrightnessConstancy and Sobel), restated twice.

In numpy, float64, with closed-form gradients: written from the description of the law, not from the reference's text.
tests/test_bc_host.py holds it against the reference's own float64 run (tests/golden/bc_small.npz); the GPU tests evaluate it
where a fixture would be too large.

In torch (``t_*``), in whatever dtype and on whatever device its inputs have, through ``grid_sample`` and autograd: the eager
baseline of tools/bcbench.py (its scatter runs with float atomics on a GPU).

Shapes: flow [B, 2, H, W] (channel 0 horizontal, channel 1 vertical, in units of S = max(H, W)); images [B, 1, H, W];
cnt [B, C, H, W]; avg [B, 2, H, W] (AveragedIWE of the masked flow, handed in: it carries no gradient).
"""
import numpy as np
import torch
import torch.nn.functional as TF

D = np.float64


# ------------------------------------------------------------------ numpy, float64
def coordinates(flow, res):
    """(ix, iy) [B, H, W]: g = 2 * (p - f * S) / (n - 1) - 1, then ((g + 1) * n - 1) / 2 (align_corners = False)."""
    H, W = res
    S = D(max(H, W))
    flow = np.asarray(flow, D)
    col, row = np.arange(W, dtype=D)[None, None, :], np.arange(H, dtype=D)[None, :, None]
    gx = 2.0 * (col - flow[:, 0] * S) / (W - 1) - 1.0
    gy = 2.0 * (row - flow[:, 1] * S) / (H - 1) - 1.0
    return ((gx + 1.0) * W - 1.0) / 2.0, ((gy + 1.0) * H - 1.0) / 2.0


def coordinate_slopes(res):
    """(d ix / d fx, d iy / d fy)."""
    H, W = res
    S = D(max(H, W))
    return -S * W / (W - 1), -S * H / (H - 1)


def _corners(ix, iy, H, W):
    """Per corner (tl, tr, bl, br): (y, x, weight, inside), and the fractions (tx, ty).  A non-finite coordinate: nothing inside."""
    ok = np.isfinite(ix) & np.isfinite(iy) & (ix >= -1) & (ix < W) & (iy >= -1) & (iy < H)
    sx, sy = np.where(ok, ix, 0.0), np.where(ok, iy, 0.0)
    x0, y0 = np.floor(sx), np.floor(sy)
    tx, ty = sx - x0, sy - y0
    x0, y0 = x0.astype(np.int64), y0.astype(np.int64)
    out = []
    for c in range(4):
        y, x = y0 + (c >> 1), x0 + (c & 1)
        w = (tx if c & 1 else 1.0 - tx) * (ty if c >> 1 else 1.0 - ty)
        inside = ok & (y >= 0) & (y < H) & (x >= 0) & (x < W)
        out.append((y, x, w, inside))
    return out, tx, ty


def sample(img, ix, iy):
    """Bilinear sample with zero padding of img [B, H, W] -> (value, d value / d ix, d value / d iy)."""
    img = np.asarray(img, D)
    B, H, W = img.shape
    corners, tx, ty = _corners(ix, iy, H, W)
    b = np.arange(B)[:, None, None]
    v = [np.where(inside, img[b, np.clip(y, 0, H - 1), np.clip(x, 0, W - 1)], 0.0) for y, x, _, inside in corners]
    value = sum(c[2] * vc for c, vc in zip(corners, v))
    dx = (1.0 - ty) * (v[1] - v[0]) + ty * (v[3] - v[2])
    dy = (1.0 - tx) * (v[2] - v[0]) + tx * (v[3] - v[1])
    return value, dx, dy


def sample_adjoint(g, ix, iy):
    """The scatter: gradient [B, H, W] into the sampled image of d loss / d value = g."""
    B, H, W = g.shape
    corners, _, _ = _corners(ix, iy, H, W)
    out = np.zeros((B, H, W), D)
    b = np.broadcast_to(np.arange(B)[:, None, None], g.shape)
    for y, x, w, inside in corners:
        np.add.at(out, (b[inside], y[inside], x[inside]), (g * w)[inside])
    return out


def sobel(x):
    """(gradx, grady) of x [..., H, W]: replication pad, correlation with the two kernels, / 8."""
    x = np.asarray(x, D)
    p = np.pad(x, [(0, 0)] * (x.ndim - 2) + [(1, 1), (1, 1)], mode="edge")
    H, W = x.shape[-2:]
    win = lambda a, c: p[..., a:a + H, c:c + W]
    gx = (win(0, 2) - win(0, 0)) + 2.0 * (win(1, 2) - win(1, 0)) + (win(2, 2) - win(2, 0))
    gy = (win(2, 0) - win(0, 0)) + 2.0 * (win(2, 1) - win(0, 1)) + (win(2, 2) - win(0, 2))
    return gx / 8.0, gy / 8.0


def sobel_adjoint(ggx, ggy):
    """Gradient into x of the pair of incoming gradients: the transposed correlation, then the pad's fold onto the border."""
    ggx, ggy = np.asarray(ggx, D), np.asarray(ggy, D)
    H, W = ggx.shape[-2:]
    p = np.zeros(ggx.shape[:-2] + (H + 2, W + 2), D)
    ka = np.array([[-1, 0, 1], [-2, 0, 2], [-1, 0, 1]], D) / 8.0
    kb = np.array([[-1, -2, -1], [0, 0, 0], [1, 2, 1]], D) / 8.0
    for a in range(3):
        for c in range(3):
            p[..., a:a + H, c:c + W] += ka[a, c] * ggx + kb[a, c] * ggy
    p[..., 1, :] += p[..., 0, :]
    p[..., H, :] += p[..., H + 1, :]
    p[..., :, 1] += p[..., :, 0]
    p[..., :, W] += p[..., :, W + 1]
    return p[..., 1:H + 1, 1:W + 1].copy()


def flow_mask(cnt):
    """[B, 1, H, W]: 1 where the channel sum is positive, the sum itself elsewhere."""
    s = np.asarray(cnt).sum(axis=1, keepdims=True)
    return np.where(s > 0, np.ones_like(s), s)


def masked_flow(flow, cnt):
    """What AveragedIWE reads, in the dtype of the flow."""
    return (flow * flow_mask(cnt).astype(flow.dtype)).astype(flow.dtype)


def generative(flow, img, cnt, avg, res):
    """(loss, grad_flow [B, 2, H, W], grad_img [B, 1, H, W])."""
    H, W = res
    S = D(max(H, W))
    m = np.asarray(flow_mask(cnt), D)
    f = np.asarray(flow, D) * m
    ix, iy = coordinates(f, res)
    sx_img, sy_img = sobel(np.asarray(img, D)[:, 0])
    sx, sx_dx, sx_dy = sample(sx_img, ix, iy)
    sy, sy_dx, sy_dy = sample(sy_img, ix, iy)
    avg = np.asarray(avg, D)
    r = (avg[:, 0] - avg[:, 1]) + (sx * f[:, 0] + sy * f[:, 1]) * S
    loss = (r ** 2).sum()
    gp = 2.0 * r * S
    dix, diy = coordinate_slopes(res)
    gfx = gp * sx + gp * (f[:, 0] * sx_dx + f[:, 1] * sy_dx) * dix
    gfy = gp * sy + gp * (f[:, 0] * sx_dy + f[:, 1] * sy_dy) * diy
    grad_flow = np.stack([gfx, gfy], axis=1) * m
    grad_img = sobel_adjoint(sample_adjoint(gp * f[:, 0], ix, iy), sample_adjoint(gp * f[:, 1], ix, iy))
    return loss, grad_flow, grad_img[:, None]


def temporal(flow, prev_img, img, res, weight):
    """(loss, grad_flow, grad_prev_img, grad_img)."""
    ix, iy = coordinates(flow, res)
    v, dx, dy = sample(np.asarray(prev_img, D)[:, 0], ix, iy)
    r = np.asarray(img, D)[:, 0] - v
    loss = weight * np.abs(r).sum()
    gr = weight * np.sign(r)
    dix, diy = coordinate_slopes(res)
    grad_flow = np.stack([-gr * dx * dix, -gr * dy * diy], axis=1)
    return loss, grad_flow, sample_adjoint(-gr, ix, iy)[:, None], gr[:, None]


def total_variation(img, weight):
    """(loss, grad_img) for img [B, C, H, W]."""
    img = np.asarray(img, D)
    dh, dw = img[:, :, :-1] - img[:, :, 1:], img[:, :, :, :-1] - img[:, :, :, 1:]
    loss = weight * (np.abs(dh).sum() + np.abs(dw).sum())
    g = np.zeros_like(img)
    g[:, :, :-1] += np.sign(dh)
    g[:, :, 1:] -= np.sign(dh)
    g[:, :, :, :-1] += np.sign(dw)
    g[:, :, :, 1:] -= np.sign(dw)
    return loss, weight * g


def kinks(flow, cnt, prev_img, img, res, tol_coord=1e-3, tol_l1=1e-4):
    """Boolean [B, H, W]: pixels at which float32 and float64 may take different branches -- a sample coordinate of either
    sampling term within tol_coord of an integer (the bilinear gradient with respect to the grid jumps there), or an L1
    argument below tol_l1 (temporal residual, or a TV difference the pixel takes part in)."""
    bad = np.zeros(np.asarray(flow)[:, 0].shape, bool)
    for f in (np.asarray(flow, D), np.asarray(flow, D) * np.asarray(flow_mask(cnt), D)):
        for c in coordinates(f, res):
            bad |= np.abs(c - np.rint(c)) < tol_coord
    ix, iy = coordinates(flow, res)
    bad |= np.abs(np.asarray(img, D)[:, 0] - sample(np.asarray(prev_img, D)[:, 0], ix, iy)[0]) < tol_l1
    x = np.asarray(img, D)[:, 0]
    dh, dw = np.abs(x[:, :-1] - x[:, 1:]) < tol_l1, np.abs(x[:, :, :-1] - x[:, :, 1:]) < tol_l1
    bad[:, :-1] |= dh
    bad[:, 1:] |= dh
    bad[:, :, :-1] |= dw
    bad[:, :, 1:] |= dw
    return bad


# ------------------------------------------------------------------ torch, any dtype and device
def t_grid(flow, res):
    H, W = res
    S = max(H, W)
    col = torch.arange(W, dtype=flow.dtype, device=flow.device)[None, None, :]
    row = torch.arange(H, dtype=flow.dtype, device=flow.device)[None, :, None]
    gx = 2 * (col - flow[:, 0] * S) / (W - 1) - 1
    gy = 2 * (row - flow[:, 1] * S) / (H - 1) - 1
    return torch.stack([gx, gy], dim=3)


def t_sobel(x):
    x = x.reshape(-1, 1, x.shape[2], x.shape[3])
    a = torch.tensor([[-1, 0, 1], [-2, 0, 2], [-1, 0, 1]], dtype=x.dtype, device=x.device)[None, None]
    b = torch.tensor([[-1, -2, -1], [0, 0, 0], [1, 2, 1]], dtype=x.dtype, device=x.device)[None, None]
    p = TF.pad(x, (1, 1, 1, 1), mode="replicate")
    return TF.conv2d(p, a) / 8, TF.conv2d(p, b) / 8


def t_generative(flow, img, cnt, avg, res):
    s = cnt.sum(dim=1, keepdim=True)
    f = flow * torch.where(s > 0, torch.ones_like(s), s)
    grid = t_grid(f, res)
    gx, gy = t_sobel(img)
    sx = TF.grid_sample(gx, grid, mode="bilinear", padding_mode="zeros", align_corners=False)
    sy = TF.grid_sample(gy, grid, mode="bilinear", padding_mode="zeros", align_corners=False)
    r = (avg[:, 0:1] - avg[:, 1:2]) + (sx * f[:, 0:1] + sy * f[:, 1:2]) * max(res)
    return (r ** 2).sum()


def t_temporal(flow, prev_img, img, res, weight):
    v = TF.grid_sample(prev_img, t_grid(flow, res), mode="bilinear", padding_mode="zeros", align_corners=False)
    return weight * (img - v).abs().sum()


def t_total_variation(img, weight):
    return weight * ((img[:, :, :-1] - img[:, :, 1:]).abs().sum() + (img[:, :, :, :-1] - img[:, :, :, 1:]).abs().sum())
