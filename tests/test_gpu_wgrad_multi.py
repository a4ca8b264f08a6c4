"""ebfi_conv2d_backward_weight_f16g_multi and ebfi_gather_sum_multi: the batched launches behind ebfi_amd.wgradqueue.

The weight gradients are checked against float64 on the CPU computed from the operands AS THE KERNEL ROUNDS THEM (scaled by
the slot's power of two, rounded to fp16; products of two fp16 numbers are exact in fp32; the bias gradient sums the fp32
gradient unrounded), so that what is left is the fp32
accumulation over the P = B*H*W pixels: |err| <= gamma_P * sum |x^||g^| with gamma_P ~ P * 2^-24 for any order of summation;
the bound asserted is twice that, componentwise, and the same bound holds between two different summation orders (multi
against the one-layer launch).  The gathers must reproduce ebfi_gather_sum bit for bit."""
import ctypes
import math

import pytest
import torch

pytestmark = pytest.mark.gpu

# B, Cin, Cout, H, W
ITEMS = [
    (2, 32, 32, 12, 20),       # ragged Cin, ragged tile rows and columns
    (1, 48, 64, 8, 8),         # ragged Cin
    (2, 64, 128, 5, 36),       # two co blocks; W crosses a 32-pixel tile by one quad; H not a multiple of 4
    (1, 128, 192, 4, 4),       # two ci x three co blocks, a single tile: never more splits than tiles
]
SLOT_STRIDE, SLOT_AMAX = 64, 32


def _pow2_scale(t):
    return 2.0 ** (1 - math.floor(math.log2(t.abs().max().item())))        # |max| * scale in [2, 4)


def _operands(items, seed):
    g = torch.Generator().manual_seed(seed)
    ops = []
    for k, (B, Cin, Cout, H, W) in enumerate(items):
        x = torch.randn(B, Cin, H, W, generator=g) * 10.0 ** (k % 3 - 1)
        go = torch.randn(B, Cout, H, W, generator=g) * 10.0 ** ((k + 1) % 3 - 2)
        x.view(-1)[(7 * k + 3) % x.numel()] = 37.5 * 10.0 ** (k % 3 - 1)         # one planted large element per operand
        go.view(-1)[(11 * k + 5) % go.numel()] = -41.25 * 10.0 ** ((k + 1) % 3 - 2)
        ops.append(dict(geo=(B, Cin, Cout, H, W), x=x, g=go, sx=_pow2_scale(x), sg=_pow2_scale(go)))
    return ops


def _reference(op):
    """float64 weight / bias gradient of the rounded operands and the componentwise bounds."""
    B, Cin, Cout, H, W = op["geo"]
    xh = (op["x"] * op["sx"]).half().double() / op["sx"]
    gh = (op["g"] * op["sg"]).half().double() / op["sg"]
    xp = torch.nn.functional.pad(xh, (1, 1, 1, 1))
    gw, aw = torch.empty(Cout, Cin, 3, 3, dtype=torch.float64), torch.empty(Cout, Cin, 3, 3, dtype=torch.float64)
    for ky in range(3):
        for kx in range(3):
            win = xp[:, :, ky:ky + H, kx:kx + W]
            gw[:, :, ky, kx] = torch.einsum("bcyx,bdyx->cd", gh, win)
            aw[:, :, ky, kx] = torch.einsum("bcyx,bdyx->cd", gh.abs(), win.abs())
    u = 2.0 * (B * H * W) * 2.0 ** -24
    # (the bias gradient is summed from the fp32 gradient itself: the kernel rounds only what goes to the matrix cores)
    g64 = op["g"].double()
    return gw, g64.sum((0, 2, 3)), u * aw, u * g64.abs().sum((0, 2, 3))


def _slots(ops):
    s = torch.zeros(2 * len(ops), SLOT_STRIDE)
    for k, op in enumerate(ops):
        s[2 * k, 0], s[2 * k + 1, 0] = op["sx"], op["sg"]
    return s.reshape(-1).cuda()


def _slot_ptr(slots, i):
    return ctypes.c_void_p(slots.data_ptr() + 4 * SLOT_STRIDE * i)


def _dev(ops):
    return [(op["x"].cuda(), op["g"].cuda()) for op in ops]


def _outputs(ops, bias, fill=None):
    mk = (lambda *s: torch.full(s, fill, device="cuda")) if fill is not None else (lambda *s: torch.empty(s, device="cuda"))
    gws = [mk(op["geo"][2], op["geo"][1], 3, 3) for op in ops]
    gbs = [mk(op["geo"][2]) if bias else None for op in ops]
    return gws, gbs


def _single(ops, dev, slots, bias):
    from ebfi_amd import _native as N
    lib = N.lib()
    gws, gbs = _outputs(ops, bias)
    for k, (op, (x, g)) in enumerate(zip(ops, dev)):
        B, Cin, Cout, H, W = op["geo"]
        need = int(lib.ebfi_conv2d_backward_weight_workspace(B, Cin, H, W, Cout, 3, 1, 1, N.EBFI_F32))
        ws = torch.empty(max(need, 4), dtype=torch.uint8, device="cuda")
        rc = lib.ebfi_conv2d_backward_weight_f16g_ex(N.ptr(x), N.ptr(g), N.ptr(None), N.ptr(gws[k]), N.ptr(gbs[k]), N.ptr(None), 0,
                                                     B, Cin, H, W, Cout, 3, 1, 1, 0, 0.0, _slot_ptr(slots, 2 * k),
                                                     _slot_ptr(slots, 2 * k + 1), N.ptr(ws), need, N.stream_ptr(x.device))
        N.check(rc, "ebfi_conv2d_backward_weight_f16g_ex")
    torch.cuda.synchronize()
    return gws, gbs


def _multi_call(geos, xs, gs, gws, gbs, slots, ksize=None, stride=None, pad=None, groups=None):
    """-> status of ebfi_conv2d_backward_weight_f16g_multi over the items (geos: B, Cin, Cout, H, W)."""
    from ebfi_amd import _native as N
    lib = N.lib()
    n = len(geos)
    ints = lambda v: (ctypes.c_int * n)(*[int(a) for a in v])
    vps = lambda v: (ctypes.c_void_p * n)(*v)
    col = lambda i: ints([g[i] for g in geos])
    Bs, Cins, Couts, Hs, Ws = col(0), col(1), col(2), col(3), col(4)
    need = int(lib.ebfi_conv2d_backward_weight_f16g_multi_workspace(n, Bs, Cins, Hs, Ws, Couts))
    ws = torch.empty(max(need, 4), dtype=torch.uint8, device="cuda")
    rc = lib.ebfi_conv2d_backward_weight_f16g_multi(
        n, vps([x.data_ptr() for x in xs]), vps([g.data_ptr() for g in gs]), vps([g.data_ptr() for g in gws]),
        vps([None if g is None else g.data_ptr() for g in gbs]), Bs, Cins, Hs, Ws, Couts, ints(ksize or [3] * n),
        ints(stride or [1] * n), ints(pad or [1] * n), ints(groups or [1] * n),
        vps([slots.data_ptr() + 4 * SLOT_STRIDE * 2 * k for k in range(n)]),
        vps([slots.data_ptr() + 4 * SLOT_STRIDE * (2 * k + 1) for k in range(n)]), N.ptr(ws), need, N.stream_ptr(xs[0].device))
    torch.cuda.synchronize()
    return rc


def _multi(ops, dev, slots, bias):
    from ebfi_amd import _native as N
    gws, gbs = _outputs(ops, bias)
    rc = _multi_call([op["geo"] for op in ops], [d[0] for d in dev], [d[1] for d in dev], gws, gbs, slots)
    N.check(rc, "ebfi_conv2d_backward_weight_f16g_multi")
    return gws, gbs


@pytest.fixture(scope="module")
def four():
    ops = _operands(ITEMS, 1234)
    return ops, _dev(ops), [_reference(op) for op in ops]


def _within(got, ref, bound, what):
    err = (got.double().cpu() - ref).abs()
    over = err > bound
    print("%s: max |err| / bound = %.3g" % (what, (err / bound.clamp_min(1e-300)).max().item()))
    assert not over.any(), (what, err[over].max().item(), bound[over].min().item())


@pytest.mark.parametrize("bias", [True, False])
def test_multi_matches_float64_and_the_single_layer_launch(four, bias):
    ops, dev, refs = four
    s_multi, s_single = _slots(ops), _slots(ops)
    gws, gbs = _multi(ops, dev, s_multi, bias)
    sws, sbs = _single(ops, dev, s_single, bias)
    for k, (gw_ref, gb_ref, bw, bb) in enumerate(refs):
        _within(gws[k], gw_ref, bw, "item %d grad_weight vs float64" % k)
        _within(gws[k], sws[k].double().cpu(), bw, "item %d grad_weight vs the single-layer launch" % k)
        assert torch.equal(gws[k], sws[k])                   # (every item keeps the single-layer split count: the same bits)
        if bias:
            _within(gbs[k], gb_ref, bb, "item %d grad_bias vs float64" % k)
            _within(gbs[k], sbs[k].double().cpu(), bb, "item %d grad_bias vs the single-layer launch" % k)
            assert torch.equal(gbs[k], sbs[k])
    # the running maxima the launches recorded: the same words after one multi call as after the single calls
    am, asg = s_multi.view(-1, SLOT_STRIDE)[:, SLOT_AMAX].cpu(), s_single.view(-1, SLOT_STRIDE)[:, SLOT_AMAX].cpu()
    assert torch.equal(am, asg), (am, asg)
    assert bool((am > 0).all())                              # (every operand was staged through its slot: the planted elements)
    # two runs: the same bits
    gws2, gbs2 = _multi(ops, dev, _slots(ops), bias)
    for a, b in zip(gws + (gbs if bias else []), gws2 + (gbs2 if bias else [])):
        assert torch.equal(a, b)


@pytest.mark.parametrize("k", range(len(ITEMS)))
def test_a_batch_of_one_is_the_single_layer_launch_bit_for_bit(four, k):
    ops, dev, _ = four
    one, done = [ops[k]], [dev[k]]
    gws, gbs = _multi(one, done, _slots(one), True)
    sws, sbs = _single(one, done, _slots(one), True)
    assert torch.equal(gws[0], sws[0]) and torch.equal(gbs[0], sbs[0])


def test_an_ineligible_item_refuses_the_whole_call_and_launches_nothing(four):
    from ebfi_amd import _native as N
    ops, dev, _ = four
    geos = [op["geo"] for op in ops]
    xs, gs = [d[0] for d in dev], [d[1] for d in dev]
    B, Cin, Cout, H, W = geos[1]
    flat = torch.randn(xs[1].numel() + 4, device="cuda")
    narrow_x, narrow_g = torch.randn(B, Cin, H, 10, device="cuda"), torch.randn(B, Cout, H, 10, device="cuda")
    cases = {
        "stride 2": dict(stride=[1, 2, 1, 1]),
        "groups 2": dict(groups=[1, 1, 2, 1]),
        "W % 4 != 0": dict(geos=[geos[0], (B, Cin, Cout, H, 10)] + geos[2:], xs=[xs[0], narrow_x] + xs[2:], gs=[gs[0], narrow_g] + gs[2:]),
        "unaligned view": dict(xs=[xs[0], flat[1:1 + xs[1].numel()].view_as(xs[1])] + xs[2:]),
    }
    for name, c in cases.items():
        gws, gbs = _outputs(ops, True, fill=-7.0)
        if "geos" in c:
            gws[1] = torch.full((Cout, Cin, 3, 3), -7.0, device="cuda")
        N.prof_reset()
        N.prof_enable(True)
        try:
            rc = _multi_call(c.get("geos", geos), c.get("xs", xs), c.get("gs", gs), gws, gbs, _slots(ops),
                             stride=c.get("stride"), groups=c.get("groups"))
        finally:
            N.prof_enable(False)
        prof = {k: v[0] for k, v in N.prof_collect().items() if v[0] > 0}
        assert rc == N.EBFI_ERR_UNSUPPORTED, (name, rc)
        assert not prof, (name, prof)
        assert all(bool((t == -7.0).all()) for t in gws + gbs), name


def test_seventeen_items_take_two_launches(four):
    from ebfi_amd import _native as N
    small = [(1, 32, 32, 8, 8), (2, 48, 32, 4, 12), (1, 64, 64, 8, 4)]
    items = [small[k % 3] for k in range(17)]
    ops = _operands(items, 99)
    dev = _dev(ops)
    N.prof_reset()
    N.prof_enable(True)
    try:
        gws, gbs = _multi(ops, dev, _slots(ops), True)
    finally:
        N.prof_enable(False)
    prof = {k: v[0] for k, v in N.prof_collect().items() if v[0] > 0}
    assert prof.get("conv_wgrad_f16_tr/f32_multi") == 2 and prof.get("conv_wgrad_reduce_f32") == 2, prof
    sws, sbs = _single(ops, dev, _slots(ops), True)
    for k, op in enumerate(ops):
        _, _, bw, bb = _reference(op)
        _within(gws[k], sws[k].double().cpu(), bw, "item %d of 17 grad_weight" % k)
        _within(gbs[k], sbs[k].double().cpu(), bb, "item %d of 17 grad_bias" % k)


# ------------------------------------------------------------------------------------------------ gathers
def _gather_single(items):
    from ebfi_amd import _native as N
    outs = []
    for src, idx, n_out, R in items:
        out = torch.full((n_out,), float("nan"), device="cuda")
        N.check(N.lib().ebfi_gather_sum(N.ptr(src), N.ptr(idx), N.ptr(out), n_out, R, N.stream_ptr(src.device)), "ebfi_gather_sum")
        outs.append(out)
    return outs


def _gather_multi(items):
    from ebfi_amd import _native as N
    n = len(items)
    outs = [torch.full((it[2],), float("nan"), device="cuda") for it in items]
    vps = lambda v: (ctypes.c_void_p * n)(*v)
    rc = N.lib().ebfi_gather_sum_multi(n, vps([it[0].data_ptr() for it in items]), vps([it[1].data_ptr() for it in items]),
                                       vps([o.data_ptr() for o in outs]), (ctypes.c_int64 * n)(*[it[2] for it in items]),
                                       (ctypes.c_int * n)(*[it[3] for it in items]), N.stream_ptr(outs[0].device))
    N.check(rc, "ebfi_gather_sum_multi")
    return outs


def _same_bits(a, b):
    torch.cuda.synchronize()
    for x, y in zip(a, b):
        assert torch.equal(x.view(torch.int32), y.view(torch.int32))


def _random_gathers(count, seed):
    g = torch.Generator().manual_seed(seed)
    items, sizes = [], [1, 255, 257, 4097]
    for k in range(count):
        n_out, R, n_src = sizes[k % 4], 1 + (k // 4) % 3, 50 + 37 * k
        idx = torch.randint(0, n_src, (n_out, R), generator=g, dtype=torch.int32)
        idx[torch.rand(n_out, R, generator=g) < 0.3] = -1
        items.append((torch.randn(n_src, generator=g).cuda(), idx.cuda(), n_out, R))
    return items


@pytest.mark.parametrize("count", [1, 12, 49])      # one item; every (n_out, R) pair; the 48 of one launch plus one
def test_gather_multi_is_bit_identical(count):
    items = _random_gathers(count, 7 + count)
    _same_bits(_gather_multi(items), _gather_single(items))


def test_gather_multi_on_real_folded_sites():
    from ebfi_amd import fold3d, weightbank
    torch.manual_seed(3)
    c3 = torch.nn.Conv3d(8, 16, 3, padding=1).cuda()
    ct = torch.nn.ConvTranspose3d(16, 8, (3, 4, 4), stride=(1, 2, 2), padding=(1, 1, 1)).cuda()
    bank = weightbank.WeightBank([c3.weight, c3.bias, ct.weight, ct.bias])
    sites = [bank.register(c3.weight, c3.bias, "conv3d", fold3d.fold_conv3d_weight, fold3d._rep2),
             bank.register(ct.weight, ct.bias, "convT3d", fold3d.fold_conv_transpose3d_weight, fold3d._rep8)]
    items = []
    for s in sites:
        gw2, gb2 = torch.randn(s.M, s.K, s.ks, s.ks, device="cuda"), torch.randn(s.M, device="cuda")
        for src, shapes, invs, Rs in ((gw2, s.w_shapes, s.w_inv, s.w_R), (gb2, s.b_shapes, s.b_inv, s.b_R)):
            for shp, inv, R in zip(shapes, invs, Rs):
                items.append((src, inv, math.prod(shp), int(R)))
    assert len(items) == 4 and max(it[3] for it in items) > 1
    _same_bits(_gather_multi(items), _gather_single(items))
