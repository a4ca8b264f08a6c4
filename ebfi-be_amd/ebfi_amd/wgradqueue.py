"""A step-wide queue of weight-gradient work that nothing in the backward pass waits for.

Only the data gradients feed the next layer of a backward pass; a layer's weight / bias gradient is needed when the
gradients are packed.  Launched where autograd meets the layer, each of the detail branch's small layers costs a
weight-gradient launch cut into as many splits as fill the chip (one tile per workgroup at 32 x 32), a slab reduction
and, for a folded site, two gathers.  Inside a `scope()` the PURE layers -- the incoming gradient is already that of the
pre-activation, so the kernel has nothing to hand to the data gradient -- are queued instead and run together by
`flush()`: `ebfi_conv2d_backward_weight_f16g_multi` (one launch and one reduction for all layers, each with the split
count of its own launch), then `ebfi_gather_sum_multi` for the fold gathers of every folded site, queued or not.  The
gradients are then assigned to `param.grad` (added where one is present), which is where autograd would have put them:
bit for bit the gradients of the per-layer launches.

Outside a scope nothing changes: `active()` is None and `conv._site_backward` launches per layer.
"""
import contextlib
import ctypes

import torch

from . import _native as N

BYTE_CAP = 1 << 30          # queued operands held back from the allocator: a safety limit, not a tuned figure

_ACTIVE = None


def active():
    return _ACTIVE


def deferrable(params, needs):
    """The queue assigns `.grad` itself: every parameter that wants a gradient must be a leaf."""
    return all((not n) or (p.is_leaf and p.requires_grad) for p, n in zip(params, needs))


def eligible(site, geo, act, x, gout):
    """What ebfi_conv2d_backward_weight_f16g_multi admits (the caller has established the fp16 weight-gradient path)."""
    B, Cin, H, W, M, ks, _, pad = geo
    return (act == 0 and ks == 3 and pad == 1 and site.groups == 1 and W % 4 == 0 and Cin >= 16 and B >= 1 and
            x.data_ptr() % 16 == 0 and gout.data_ptr() % 16 == 0 and
            not (B * H * W >= 65536 and (M <= 4 or Cin <= 4)))          # (the thin layers have kernels of their own)


def _vps(vals):
    return (ctypes.c_void_p * len(vals))(*vals)


def _ints(vals):
    return (ctypes.c_int * len(vals))(*[int(v) for v in vals])


class WgradQueue:
    def __init__(self, byte_cap=BYTE_CAP):
        self.byte_cap = int(byte_cap)
        self.layers = []        # (site, x, gout, geo, x_slot, g_slot, params, needs)
        self.gathers = []       # (src, inv, R, shape, param)
        self.bytes = 0
        self.flushes = 0

    # ------------------------------------------------------------------ enqueue (conv._site_backward)
    def add_layer(self, site, x, gout, geo, x_slot, g_slot, params, needs):
        self.layers.append((site, x, gout, list(geo), x_slot, g_slot, list(params), list(needs)))
        self._held(x.numel() * x.element_size() + gout.numel() * gout.element_size())

    def add_routes(self, site, gw2, gb2, params, needs, count=True):
        """The gradient routing of one site (conv._route_site_grads): views of the folded gradient are assigned now, the gathers
        of a folded site are queued."""
        nw = len(site.w_shapes)
        if site.kind == "id":
            row = 0
            for p, need, shp in zip(params[:nw], needs[:nw], site.w_shapes):
                if need:
                    _assign(p, gw2[row:row + shp[0]].view(shp))
                row += shp[0]
            row = 0
            for p, need, shp in zip(params[nw:], needs[nw:], site.b_shapes):
                if need:
                    _assign(p, gb2[row:row + shp[0]].view(shp))
                row += shp[0]
            return
        for p, need, shp, inv, R in zip(params[:nw], needs[:nw], site.w_shapes, site.w_inv, site.w_R):
            if need:
                self.gathers.append((gw2, inv, int(R), shp, p))
        for p, need, shp, inv, R in zip(params[nw:], needs[nw:], site.b_shapes, site.b_inv, site.b_R):
            if need:
                self.gathers.append((gb2, inv, int(R), shp, p))
        if count:
            self._held(gw2.numel() * 4)

    def _held(self, nbytes):
        self.bytes += int(nbytes)
        if self.bytes > self.byte_cap:
            self.flush()

    # ------------------------------------------------------------------ flush
    def flush(self):
        layers, self.layers = self.layers, []
        if layers:
            self._run_layers(layers)
        gathers, self.gathers = self.gathers, []
        if gathers:
            self._run_gathers(gathers)
        self.bytes = 0
        self.flushes += 1

    def _run_layers(self, layers):
        lib = N.lib()
        dev = layers[0][1].device
        n = len(layers)
        gws, gbs = [], []
        for site, x, gout, geo, xs, gs, params, needs in layers:
            gws.append(torch.empty((site.M, site.K, 3, 3), dtype=x.dtype, device=dev))
            gbs.append(torch.empty(site.M, dtype=x.dtype, device=dev) if site.has_bias else None)
        col = lambda i: _ints([L[3][i] for L in layers])
        Bs, Cins, Hs, Ws, Couts = col(0), col(1), col(2), col(3), col(4)
        need = int(lib.ebfi_conv2d_backward_weight_f16g_multi_workspace(n, Bs, Cins, Hs, Ws, Couts))
        if need == 0:
            raise N.EbfiNativeError("ebfi_conv2d_backward_weight_f16g_multi_workspace refused the queued layers")
        ws = torch.empty(need, dtype=torch.uint8, device=dev)
        slot = lambda v: v.value if isinstance(v, ctypes.c_void_p) else v
        with torch.cuda.device(dev):
            rc = lib.ebfi_conv2d_backward_weight_f16g_multi(
                n, _vps([L[1].data_ptr() for L in layers]), _vps([L[2].data_ptr() for L in layers]),
                _vps([g.data_ptr() for g in gws]), _vps([None if g is None else g.data_ptr() for g in gbs]),
                Bs, Cins, Hs, Ws, Couts, col(5), col(6), col(7), _ints([L[0].groups for L in layers]),
                _vps([slot(L[4]) for L in layers]), _vps([slot(L[5]) for L in layers]), N.ptr(ws), need, N.stream_ptr(dev))
        N.check(rc, "ebfi_conv2d_backward_weight_f16g_multi")
        for (site, x, gout, geo, xs, gs, params, needs), gw2, gb2 in zip(layers, gws, gbs):
            self.add_routes(site, gw2, gb2, params, needs, count=False)

    def _run_gathers(self, gathers):
        lib = N.lib()
        dev = gathers[0][0].device
        outs = [torch.empty(shp, dtype=src.dtype, device=dev) for src, inv, R, shp, p in gathers]
        n = len(gathers)
        with torch.cuda.device(dev):
            rc = lib.ebfi_gather_sum_multi(n, _vps([g[0].data_ptr() for g in gathers]), _vps([g[1].data_ptr() for g in gathers]),
                                           _vps([o.data_ptr() for o in outs]), (ctypes.c_int64 * n)(*[o.numel() for o in outs]),
                                           _ints([g[2] for g in gathers]), N.stream_ptr(dev))
        N.check(rc, "ebfi_gather_sum_multi")
        for (src, inv, R, shp, p), out in zip(gathers, outs):
            _assign(p, out)


def _assign(p, g):
    p.grad = g if p.grad is None else p.grad + g


@contextlib.contextmanager
def scope(enabled=True, byte_cap=BYTE_CAP):
    """Queue the deferrable weight-gradient work of the backward passes inside; the caller flushes (`q.flush()`) after
    `backward()`.  enabled=False: a no-op scope (yields None)."""
    global _ACTIVE
    if not enabled:
        yield None
        return
    prev, _ACTIVE = _ACTIVE, WgradQueue(byte_cap)
    try:
        yield _ACTIVE
    finally:
        q, _ACTIVE = _ACTIVE, prev
        q.layers, q.gathers = [], []        # (an exception between backward and flush: drop the operands)
