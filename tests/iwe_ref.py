"""The law of ebfi_amd.iwe, restated twice.

In numpy, serially, float32: what the reference's myutils/iwe.py and loss/flow.py compute with one thread -- every pixel
receives its addends in ascending list position, each product and sum rounded to float32.  tests/test_iwe_host.py holds this
restatement against the reference's own outputs (tests/golden/iwe_small.npz) bit for bit; the GPU tests use it where a fixture
would be too large.

In torch (``t_*``), in whatever dtype and on whatever device its inputs have: the float64 oracle of the loss and its gradient
(autograd), and the eager baseline of tools/iwebench.py.

Event layout: events[b, n] = (ts, y, x, p).
"""
import numpy as np
import torch

F = np.float32


# ------------------------------------------------------------------ numpy, serial, float32
def event_flow(flow, events, res):
    """[B, N, 2] = (vertical, horizontal) flow at each event's source pixel y * W + x."""
    B = flow.shape[0]
    flat = flow.reshape(B, 2, -1)
    at = (events[:, :, 1] * F(res[1]) + events[:, :, 2]).astype(np.int64)
    return np.stack([np.take_along_axis(flat[:, 1], at, 1), np.take_along_axis(flat[:, 0], at, 1)], axis=2).astype(F)


def get_interpolation(events, flow_ev, tref, res, scaling, round_idx=False):
    """(idx, weights), float32 [B, M, 1]."""
    H, W = res
    warped = (events[:, :, 1:3] + (F(tref) - events[:, :, 0:1]) * flow_ev * F(scaling)).astype(F)
    if round_idx:
        corner = np.rint(warped)                                     # half to even, as torch.round
        weights = np.ones_like(corner)
    else:
        top, left = np.floor(warped[:, :, 0:1]), np.floor(warped[:, :, 1:2])
        bottom, right = np.floor(warped[:, :, 0:1] + F(1)), np.floor(warped[:, :, 1:2] + F(1))
        corner = np.concatenate([np.concatenate(c, axis=2) for c in ((top, left), (top, right), (bottom, left), (bottom, right))],
                                axis=1)
        weights = np.maximum(F(0), F(1) - np.abs(np.concatenate([warped] * 4, axis=1) - corner)).astype(F)
    outside = (corner[:, :, 0:1] < 0) | (corner[:, :, 0:1] >= H) | (corner[:, :, 1:2] < 0) | (corner[:, :, 1:2] >= W)
    mask = np.where(outside, F(0), F(1))
    corner = corner * mask
    weights = (weights[:, :, 0:1] * weights[:, :, 1:2]) * mask
    idx = corner[:, :, 0:1] * F(W) + corner[:, :, 1:2]
    return idx.astype(F), weights.astype(F)


def interpolate(idx, weights, res, polarity_mask=None, reverse=False):
    """[B, 1, H, W]: the serial scatter; ``reverse`` walks the list backwards (the order test)."""
    H, W = res
    B, M = idx.shape[:2]
    w = weights if polarity_mask is None else (weights * polarity_mask).astype(F)
    at = idx.astype(np.int64)
    out = np.zeros((B, H * W), F)
    order = range(M - 1, -1, -1) if reverse else range(M)
    for b in range(B):
        for m in order:
            out[b, at[b, m, 0]] = F(out[b, at[b, m, 0]] + w[b, m, 0])
    return out.reshape(B, 1, H, W)


def deblur_events(flow, events, res, scaling=128, round_idx=True, polarity_mask=None):
    idx, w = get_interpolation(events, event_flow(flow, events, res), 1, res, scaling, round_idx)
    if not round_idx:
        polarity_mask = np.concatenate([polarity_mask] * 4, axis=1)
    return interpolate(idx, w, res, polarity_mask)


def compute_pol_iwe(flow, events, res, pos_mask, neg_mask, scaling=128, round_idx=True):
    return np.concatenate([deblur_events(flow, events, res, scaling, round_idx, m) for m in (pos_mask, neg_mask)], axis=1)


def warping_images(flow, events, pol_mask, res, reverse=False):
    """[2 (tref = 1, 0), B, 4 (count+, count-, stamp sum+, stamp sum-), H * W]: the eight images the loss is made of."""
    B = events.shape[0]
    fe = event_flow(flow, events, res)
    pm = np.concatenate([pol_mask] * 4, axis=1)
    ts = np.concatenate([events[:, :, 0:1]] * 4, axis=1)
    out = []
    for tref, stamp in ((1, ts), (0, (F(1) - ts).astype(F))):
        idx, w = get_interpolation(events, fe, tref, res, max(res))
        wt = (w * stamp).astype(F)
        planes = [interpolate(idx, ww, res, pm[:, :, q:q + 1], reverse) for ww in (w, wt) for q in (0, 1)]
        out.append(np.concatenate(planes, axis=1).reshape(B, 4, -1))
    return np.stack(out)


def warping_loss(flow, events, pol_mask, res, weight):
    """The loss of one flow from the float32 images, the squares, roots and sums in float64 (the device kernel's recipe)."""
    img = warping_images(flow, events, pol_mask, res)
    ratio = (img[:, :, 2:4] / (img[:, :, 0:2] + F(1e-9)).astype(F)).astype(F)
    total = (ratio.astype(np.float64) ** 2).sum()
    dx = (flow[:, :, :-1, :] - flow[:, :, 1:, :]).astype(np.float64)
    dy = (flow[:, :, :, :-1] - flow[:, :, :, 1:]).astype(np.float64)
    return total + weight * (np.sqrt(dx ** 2 + 1e-6).sum() + np.sqrt(dy ** 2 + 1e-6).sum())


def averaged_iwe(flow, events, pol_mask, res):
    """[B, 2, H, W]: rounded counts, each divided by the number of distinct source pixels feeding that pixel and polarity."""
    H, W = res
    B, N = events.shape[:2]
    if N == 0:
        return np.zeros((B, 2, H, W), F)
    idx, w = get_interpolation(events, event_flow(flow, events, res), 1, res, max(res), True)
    out = np.concatenate([interpolate(idx, w, res, pol_mask[:, :, q:q + 1]) for q in (0, 1)], axis=1).reshape(B, 2, -1)
    src = (events[:, :, 1] * F(W) + events[:, :, 2]).astype(np.int64)
    for b in range(B):
        feeds = {}
        for n in range(N):
            if w[b, n, 0] == 0:
                continue                                             # an unfeasible mapping is ignored
            channel = 1 if events[b, n, 3] < 1 else 0                # `p < 1` is negative
            feeds.setdefault((channel, int(idx[b, n, 0])), set()).add(int(src[b, n]))
        for (channel, pix), sources in feeds.items():
            out[b, channel, pix] = F(out[b, channel, pix] / F(len(sources)))
    return out.reshape(B, 2, H, W)


def near_integer(flows, events, pol_mask, res, tol=1e-3):
    """Unmasked events whose float64 warped coordinate (either tref, any flow) lies within ``tol`` of an integer: there
    float32 and float64 may pick different corners and a comparison under a tolerance means nothing."""
    e = events.astype(np.float64)
    live = pol_mask.sum(axis=2) != 0
    bad = np.zeros(events.shape[:2], bool)
    for flow in flows:
        fe = event_flow(flow, events, res).astype(np.float64)
        for tref in (1.0, 0.0):
            warped = e[:, :, 1:3] + (tref - e[:, :, 0:1]) * fe * float(max(res))
            bad |= (np.abs(warped - np.rint(warped)) < tol).any(axis=2)
    return bad & live


# ------------------------------------------------------------------ torch, any dtype, any device
def t_event_flow(flow, events, res):
    B = flow.shape[0]
    flat = flow.reshape(B, 2, -1)
    at = (events[:, :, 1] * res[1] + events[:, :, 2]).long()
    return torch.stack([flat[:, 1].gather(1, at), flat[:, 0].gather(1, at)], dim=2)


def t_get_interpolation(events, flow_ev, tref, res, scaling, round_idx=False):
    H, W = res
    warped = events[:, :, 1:3] + (tref - events[:, :, 0:1]) * flow_ev * scaling
    if round_idx:
        corner = torch.round(warped)
        weights = torch.ones_like(corner)
    else:
        lo, hi = torch.floor(warped), torch.floor(warped + 1)
        corner = torch.cat([torch.stack([y[:, :, 0], x[:, :, 1]], dim=2) for y, x in ((lo, lo), (lo, hi), (hi, lo), (hi, hi))], dim=1)
        tent = 1 - torch.abs(torch.cat([warped] * 4, dim=1) - corner)
        weights = torch.maximum(torch.zeros_like(tent), tent)            # (a tie passes half the gradient; clamp would pass all)
    inside = (corner[:, :, 0:1] >= 0) & (corner[:, :, 0:1] < H) & (corner[:, :, 1:2] >= 0) & (corner[:, :, 1:2] < W)
    mask = inside.to(warped.dtype)
    corner = corner * mask
    weights = weights[:, :, 0:1] * weights[:, :, 1:2] * mask
    return corner[:, :, 0:1] * W + corner[:, :, 1:2], weights


def t_interpolate(idx, weights, res, polarity_mask=None):
    if polarity_mask is not None:
        weights = weights * polarity_mask
    out = torch.zeros((idx.shape[0], res[0] * res[1], 1), dtype=weights.dtype, device=weights.device)
    return out.scatter_add(1, idx.long(), weights).view(idx.shape[0], 1, res[0], res[1])


def t_event_warping(flows, events, pol_mask, res, weight):
    """The loss over a list of flows; differentiable in the flows."""
    pm = torch.cat([pol_mask] * 4, dim=1)
    ts = torch.cat([events[:, :, 0:1]] * 4, dim=1)
    loss = 0
    for flow in flows:
        fe = t_event_flow(flow, events, res)
        for tref, stamp in ((1, ts), (0, 1 - ts)):
            idx, w = t_get_interpolation(events, fe, tref, res, max(res))
            for q in (0, 1):
                count = t_interpolate(idx, w, res, pm[:, :, q:q + 1])
                total = t_interpolate(idx, w * stamp, res, pm[:, :, q:q + 1])
                loss = loss + ((total / (count + 1e-9)) ** 2).sum()
        dx = flow[:, :, :-1, :] - flow[:, :, 1:, :]
        dy = flow[:, :, :, :-1] - flow[:, :, :, 1:]
        loss = loss + weight * (torch.sqrt(dx ** 2 + 1e-6).sum() + torch.sqrt(dy ** 2 + 1e-6).sum())
    return loss


def t_averaged_iwe(flow, events, pol_mask, res):
    H, W = res
    B, N = events.shape[:2]
    P = H * W
    if N == 0:
        return torch.zeros((B, 2, H, W), dtype=flow.dtype, device=flow.device)
    idx, w = t_get_interpolation(events, t_event_flow(flow, events, res), 1, res, max(res), True)
    out = torch.cat([t_interpolate(idx, w, res, pol_mask[:, :, q:q + 1]) for q in (0, 1)], dim=1).reshape(B * 2 * P)
    src = (events[:, :, 1] * W + events[:, :, 2]).long()
    channel = (events[:, :, 3] < 1).long()
    item = torch.arange(B, device=events.device).view(B, 1).expand(B, N)
    slot = (item * 2 + channel) * P + idx[:, :, 0].long()             # the output element an event feeds
    live = w[:, :, 0] != 0
    pairs = torch.unique(slot[live] * P + src[live])                  # distinct (output element, source pixel)
    feeds = torch.bincount(pairs // P, minlength=B * 2 * P)
    out = torch.where(feeds > 0, out / feeds.clamp_min(1).to(out.dtype), out)
    return out.view(B, 2, H, W)
