"""ebfi_pack_pairs_bf16 (csrc/conv2d.hip) and the bank that drives it (ebfi_amd.weightbank): one table entry and one gather per
(hi, lo) pair, blocks of 512 entries, a launch over the blocks on the bank's list.

The bank of the tiny model (grouped concatenated sites rcA / rcB, Conv3d and ConvTranspose3d folds with structural zeros) plus
hand-registered corners: 3x3 5 -> 7 and 1x1 20 -> 3 (channel padding entries; 1008 and 96 entries: no multiple of the block or
of the workgroup), a grouped concatenation, one more fold of each kind.  Every image's device bytes must equal the expectation
formed on the host from the folded fp32 weight with torch's bf16 rounding (the `expect` construction of tests/test_host_logic.py),
and the whole buffer must equal what ebfi_pack_table_bf16 writes from `bank.table`.  With NaN / +-Inf weights planted the
comparison is the same, except that where the expectation is a NaN the device value must be a NaN: lo = bf16(Inf - Inf)
is a GENERATED NaN, whose sign IEEE 754 leaves open (the host makes it negative, the GPU positive); against
ebfi_pack_table_bf16 the bytes stay equal there too."""
import pytest
import torch

pytestmark = pytest.mark.gpu

SENTINEL = 0x5A5A


def _expect(W2, groups=1):
    M, K, ks, _ = W2.shape
    Mg = M // groups
    K16, M16 = (K + 15) // 16 * 16, (Mg + 15) // 16 * 16
    W2 = W2 + 0.0          # (the folds form structural zeros as weight * 0, -0.0 under a negative weight; the pack writes +0)
    f = torch.zeros(ks * ks, M, K16)
    f[:, :, :K] = W2.permute(2, 3, 0, 1).reshape(ks * ks, M, K)
    t = torch.zeros(ks * ks, groups * K, M16)
    for gi in range(groups):
        t[:, gi * K:(gi + 1) * K, :Mg] = W2[gi * Mg:(gi + 1) * Mg].flip((2, 3)).permute(2, 3, 1, 0).reshape(ks * ks, K, Mg)
    split = lambda v: torch.cat([v.bfloat16(), (v - v.bfloat16().float()).bfloat16()])       # [hi | lo]
    return {"fwd": split(f.reshape(-1)), "tr": split(t.reshape(-1))}


class _Bank:
    """The tiny model's bank plus the hand-registered corners, and the folded fp32 weight of every site."""

    def __init__(self, book=False, on_demand=False, plant=False):
        from ebfi_amd import f16scale, fold3d, weightbank
        from ebfi_amd.engine import DEFAULT_MODEL_ARGS
        from ebfi_amd.model import EVFIAutoEx
        torch.manual_seed(21)
        self.net = net = EVFIAutoEx(**dict(DEFAULT_MODEL_ARGS, FrameBasech=8, EventBasech=8, InterCH=8, TB=4, step=2,
                                           channels=[4, 4, 8, 8])).cuda()
        P = lambda *shape: torch.nn.Parameter(torch.empty(*shape, device="cuda"))
        self.extra = extra = {"w57": P(7, 5, 3, 3), "w203": P(3, 20, 1, 1), "ga": P(8, 8, 3, 3), "gb": P(8, 8, 3, 3),
                              "c3": P(6, 5, 3, 3, 3), "ct3": P(5, 3, 3, 4, 4)}
        with torch.no_grad():
            for p in list(net.parameters()) + list(extra.values()):
                p.copy_(torch.randn_like(p))
            if plant:
                extra["w57"][1, 2, 0, 1] = float("nan")
                extra["w57"][3, 0, 2, 2] = float("inf")
                extra["ga"][0, 0, 0, 0] = float("-inf")
                extra["c3"][2, 1, 1, 1, 1] = float("nan")
        self.params = params = list(net.parameters()) + list(extra.values())
        self.bank = bank = weightbank.build_for(net, params=params, fwd16="filters" if book else None)
        bank.register(extra["w57"], None, "id")
        bank.register(extra["w203"], None, "id")
        bank.register([extra["ga"], extra["gb"]], None, kind="gcat", groups=2)
        bank.register(extra["c3"], None, "conv3d", fold3d.fold_conv3d_weight)
        bank.register(extra["ct3"], None, "convT3d", fold3d.fold_conv_transpose3d_weight)
        if book:
            bank.attach_scale_book(f16scale.ScaleBook("cuda"))
        bank.pack_on_demand = on_demand

    def folded(self, key):
        from ebfi_amd import fold3d
        net, rc = self.net, self.net.ResidualControl
        ptr, kind = key
        w = {p.data_ptr(): p for p in self.params}[ptr].detach().cpu()
        if kind in ("rcA", "rcB"):
            for i in range(rc.step):
                for j in (0, 1):
                    if rc.Conv3[i][j].conv2d.weight.data_ptr() == ptr:
                        return torch.cat([rc.Conv3[i][j].conv2d.weight, rc.Conv4[i][j].conv2d.weight]).detach().cpu(), \
                            (2 if kind == "rcB" else 1)
        if kind == "gcat":
            return torch.cat([self.extra["ga"], self.extra["gb"]]).detach().cpu(), 2
        if kind == "conv3d":
            return fold3d.fold_conv3d_weight(w), 1
        if kind == "convT3d":
            return fold3d.fold_conv_transpose3d_weight(w), 1
        if kind == "fuse_d2":
            return net.Detail._fuse_weight_on_depth_minor_channels(w), 1
        assert kind == "id", kind
        return w, 1

    def image(self, site, name):
        """(device int16 bits of [hi | lo], expected bf16 values) of one image."""
        off, nbytes = getattr(site, name + "_off") // 2, getattr(site, name + "_bytes") // 2
        W2, groups = self.folded(site.key)
        assert site.groups == groups
        return self.bank.packed[off:off + nbytes].view(torch.int16).cpu(), _expect(W2, groups)[name]

    def images(self):
        return [(s, name) for s in self.bank.sites.values() for name in ("fwd", "tr") if getattr(s, name + "_bytes")]


def _same(bits, want, nan_ok=False):
    want_bits = want.view(torch.int16)
    if not nan_ok:
        return torch.equal(bits, want_bits)
    nan = torch.isnan(want.float())
    return torch.equal(bits[~nan], want_bits[~nan]) and bool(torch.isnan(bits.view(torch.bfloat16).float()[nan]).all())


def _old_pack(bank):
    """What ebfi_pack_table_bf16 writes from the bank's one-entry-per-element table."""
    from ebfi_amd import _native as N
    table = bank.table.cuda()
    assert table.numel() == bank._n_packed
    out = torch.empty(max(table.numel(), 8), dtype=torch.bfloat16, device="cuda")
    N.check(N.lib().ebfi_pack_table_bf16(N.ptr(bank.flat), N.ptr(table), table.numel(), N.ptr(out), N.stream_ptr(out.device)),
            "ebfi_pack_table_bf16")
    return out


@pytest.mark.parametrize("plant", [False, True], ids=["finite", "nan_inf"])
def test_bank_without_a_book_packs_every_image_bit_for_bit(plant):
    b = _Bank(plant=plant)
    bank = b.bank
    bank.refresh()
    bank.packed.view(torch.int16).fill_(SENTINEL)          # (whatever the pack does not write stays visible)
    bank.refresh()
    kinds = {k for _, k in bank.sites}
    assert {"id", "conv3d", "convT3d", "rcA", "rcB", "gcat"} <= kinds
    imgs = b.images()
    assert len(imgs) == len(bank.packed_images()) >= len(bank.sites)
    sizes = {getattr(s, n + "_bytes") // 4 for s, n in imgs}
    assert any(sz % 512 for sz in sizes) and any(sz % 256 for sz in sizes) and 9 * 7 * 16 in sizes and 3 * 32 in sizes
    for site, name in imgs:
        bits, want = b.image(site, name)
        assert _same(bits, want, nan_ok=plant), (site.kind, name, site.M, site.K)
    if plant:
        assert torch.isnan(bank.packed.float()).any() and torch.isinf(bank.packed.float()).any()
    # the whole buffer: every byte written, and as the one-entry-per-element launch writes it
    assert torch.equal(bank.packed[:bank._n_packed].view(torch.int16), _old_pack(bank)[:bank._n_packed].view(torch.int16))
    again = bank.packed.clone()
    bank.refresh()
    assert torch.equal(again.view(torch.int16), bank.packed.view(torch.int16))


def test_on_demand_bank_packs_an_image_when_it_is_first_asked_for():
    from ebfi_amd import weightbank
    b = _Bank(book=True, on_demand=True)
    bank = b.bank
    bank.refresh()
    bank.packed.view(torch.int16).fill_(SENTINEL)
    bank.refresh()
    assert bank.packed_images() == [] and bool((bank.packed.view(torch.int16) == SENTINEL).all())     # nothing asked for yet
    assert bank.packed16 is not None                                                                   # (the fp16 images are)
    key57 = (b.extra["w57"].data_ptr(), "id")
    s57, sg = bank.sites[key57], bank.sites[(b.extra["ga"].data_ptr(), "gcat")]
    # a first request inside a capture must fail, and must not list the image
    g = torch.cuda.CUDAGraph()
    with pytest.raises(weightbank.WeightImageError):
        with torch.cuda.graph(g):
            s57.tr_ptr()
    assert bank.packed_images() == []
    # asking for an image packs it at once -- and only it
    p = s57.fwd_ptr()
    assert p.value == bank.packed.data_ptr() + s57.fwd_off and bank.packed_images() == [(key57, "fwd")]
    bits, want = b.image(s57, "fwd")
    assert _same(bits, want)
    bits_tr, _ = b.image(s57, "tr")
    assert bool((bits_tr == SENTINEL).all())
    sg.tr_ptr()
    bits, want = b.image(sg, "tr")
    assert _same(bits, want)
    written = 2 * (s57.fwd_bytes // 4) + 2 * (sg.tr_bytes // 4)
    assert int((bank.packed.view(torch.int16) != SENTINEL).sum()) <= written
    # new parameter values: ensure_fresh() re-packs the images asked for, and nothing else
    with torch.no_grad():
        b.extra["w57"].mul_(1.7)
        b.extra["ga"].add_(0.3)
    bank.ensure_fresh()
    for site, name in ((s57, "fwd"), (sg, "tr")):
        bits, want = b.image(site, name)
        assert _same(bits, want), name
    assert bool((b.image(s57, "tr")[0] == SENTINEL).all()) and bool((b.image(sg, "fwd")[0] == SENTINEL).all())
    # a captured refresh replays over the images listed when it was captured; a later request appends behind them
    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):
        bank.refresh()
    torch.cuda.current_stream().wait_stream(side)
    g = torch.cuda.CUDAGraph()
    with torch.cuda.graph(g):
        bank.refresh()
        s57.fwd_ptr()                                      # already listed: fine inside a capture
    s57.tr_ptr()
    with torch.no_grad():
        b.extra["w57"].mul_(0.5)
    bank.flat.copy_(torch.cat([q.detach().reshape(-1) for q in b.params]))
    bank.packed.view(torch.int16).fill_(SENTINEL)
    g.replay()
    torch.cuda.synchronize()
    bits, want = b.image(s57, "fwd")
    assert _same(bits, want)
    assert bool((b.image(s57, "tr")[0] == SENTINEL).all())          # listed after the capture: not part of that graph
    bank.refresh()
    bits, want = b.image(s57, "tr")
    assert _same(bits, want)
    # forgetting the requests empties the per-step pack again
    bank.forget_requests()
    bank.packed.view(torch.int16).fill_(SENTINEL)
    bank.refresh()
    assert bank.packed_images() == [] and bool((bank.packed.view(torch.int16) == SENTINEL).all())
