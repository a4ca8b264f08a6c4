"""The fp16 delayed-scaling slot {scale, floor, running |max|} (csrc/c16.hpp, csrc/scale_law.hpp, ebfi_amd/f16scale.py) on the
device against its numpy restatement oracle/scale_ref.py, bit for bit (torch.equal on int32 views throughout):

  a. ebfi_f16_scales_finish over tables of 600 slots, all 64 words of every slot, and its flag-raising rows;
  b. every kernel that records a maximum, on a fresh slot and on slots with a live floor / a maximum / a NaN already there;
  c. the maximum on the first and the last element of the tensor (the tail of a ragged tile) under a live floor;
  d. one layer's training step in closed loop over a gradient whose magnitude rises, drops, overflows and turns NaN.

The conversions saturate, so the recorded maximum is the only overflow signal a step has: a writer that loses one element above
the floor, or a finish launch that sets a wrong scale, gives finite wrong gradients that nothing else notices."""
import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

from ebfi_amd import _native as N  # noqa: E402
from oracle import scale_ref as R  # noqa: E402

S, AMAX, FLOOR = R.SLOT_STRIDE, R.SLOT_AMAX, R.SLOT_FLOOR
QNAN = 0x7fc00000
IMG_SHAPES = [(2, 64, 16, 64), (1, 64, 13, 36)]          # whole tiles; ragged tiles (13 rows, 36 columns)


def _fbits(v):
    return int(np.array([v], dtype=np.float32).view(np.uint32)[0])


def _i32(a):
    """numpy float32 / uint32 array -> torch int32 tensor of the same bits."""
    return torch.from_numpy(np.ascontiguousarray(a).view(np.int32).copy())


def _words(book, i):
    return book.slots[S * i:S * i + S].view(torch.int32).cpu()


def _set_words(book, i, **words):
    v = book.slots.view(torch.int32)
    for name, b in words.items():
        v[S * i + {"scale": 0, "floor": FLOOR, "amax": AMAX}[name]] = int(b)


def _fill_unused(book, i):
    """A bit pattern in the 61 words of slot i that nothing may touch."""
    pat = (torch.arange(S, dtype=torch.int64) * 0x01010101 + 0x12345 + i).to(torch.int32)
    keep = _words(book, i)
    for k in (0, FLOOR, AMAX):
        pat[k] = keep[k]
    book.slots.view(torch.int32)[S * i:S * i + S] = pat.cuda()


def _states(m_bits):
    """The six live states of the issue's table as (|max| bits, floor bits), built on M (on 1.0 for a launch that records
    nothing): floor just below M / at M / above M; a smaller and a larger maximum already there; a NaN already there."""
    base = m_bits if m_bits > 0 else _fbits(1.0)
    f = float(R.from_bits(np.array([base], np.uint32))[0])
    return [(0, base - 1), (0, base), (0, _fbits(2 * f)), (_fbits(f / 2), 0), (_fbits(2 * f), 0), (QNAN, 0)]


def _check_writer(book, idx, launch, known=None, records=True):
    """`launch()` runs the kernel once on the slots `idx` of `book` (scales already set).  Fresh slots first: the recorded bits M
    (== `known` where the host knows the value), scale and floor untouched; then the six live states against scale_ref.record."""
    for i in idx:
        _fill_unused(book, i)
    fresh = [_words(book, i) for i in idx]
    launch()
    torch.cuda.synchronize()
    M = []
    for n, i in enumerate(idx):
        w = _words(book, i)
        M.append(int(w[AMAX]))
        assert (M[n] > 0) == records, (n, M[n])
        if known is not None and known[n] is not None:
            assert M[n] == _fbits(known[n]), (n, hex(M[n]), known[n])
        exp = fresh[n].clone()
        exp[AMAX] = M[n]
        assert torch.equal(w, exp), n
    for st in range(6):
        before = []
        for n, i in enumerate(idx):
            a, f = _states(M[n])[st]
            _set_words(book, i, amax=a, floor=f)
            before.append(_words(book, i).numpy().view(np.float32))
        launch()
        torch.cuda.synchronize()
        for n, i in enumerate(idx):
            exp = R.record(before[n], M[n])
            assert torch.equal(_words(book, i), _i32(exp)), (st, n, hex(M[n]), _words(book, i)[[0, FLOOR, AMAX]].tolist())
    return M


def _new_book(*scales):
    from ebfi_amd import f16scale
    book = f16scale.ScaleBook("cuda")
    idx = [book.slot(("t", k)) for k in range(len(scales))]
    for i, s in zip(idx, scales):
        book.slots[S * i] = s
    return book, idx


def _more_slots(book, *scales):
    idx = [book.slot(("t", len(book.index) + k)) for k in range(len(scales))]
    for i, s in zip(idx, scales):
        book.slots[S * i] = s
    return idx


def _banked(cin, cout, groups=1, w=None):
    from ebfi_amd import f16scale, weightbank
    if w is None:
        w = torch.randn(cout, cin, 3, 3) / (cin * 9) ** 0.5
    w = torch.nn.Parameter(w.cuda())
    b = torch.nn.Parameter((torch.randn(cout) * 0.1).cuda())
    bank = weightbank.WeightBank([w, b])
    site = bank.register(w, b, "id", groups=groups)
    book = f16scale.ScaleBook("cuda")
    bank.attach_scale_book(book)
    return w, b, bank, book, site


def _amax(*ts):
    return max(t.abs().max().item() for t in ts)


# ------------------------------------------------------------------------------------------------------------------ a. finish
def _finish(slots_np, guard_np, n, tail=1):
    """One ebfi_f16_scales_finish launch over the first n slots of a buffer that holds `tail` more (which must stay untouched).
    Returns (rc, slots int32 [n + tail, 64], guard int32 [2])."""
    slots = _i32(slots_np).cuda().view(torch.float32)
    guard = torch.from_numpy(np.array(guard_np, dtype=np.int32)).cuda()
    rc = N.lib().ebfi_f16_scales_finish(N.ptr(slots), n, N.ptr(guard), N.stream_ptr(slots.device))
    torch.cuda.synchronize()
    return rc, slots.view(torch.int32).cpu().reshape(-1, S), guard.cpu()


def _sentinel(rows=1):
    return R.from_bits(np.full((rows, S), 0x5a5a5a5a, np.uint32))


@pytest.mark.parametrize("part", [0, 1])
def test_finish_table_every_word_of_600_slots(part):
    """Every clean |max| of scale_ref.clean_amax_values() -- 769 values, dealt over two launches of n = 600 (three workgroups,
    the last one partial) -- under scales in use from 2^-126 to 2^120, |max| * scale up to exactly 60000, floors 0 / normal /
    subnormal: all 64 words of all 600 slots, the slot behind them, and guard == [0, 7]."""
    slots, guard = R.finish_tables()[part]
    assert slots.shape == (600, S) and list(guard) == [0, 7]
    buf = np.concatenate([slots, _sentinel()])
    exp_slots, exp_guard = R.finish(slots, guard)
    rc, got, got_guard = _finish(buf, guard, 600)
    assert rc == 0
    bad = (got[:600] != _i32(exp_slots)).any(1).nonzero().reshape(-1).tolist()
    assert not bad, [(r, [hex(v & 0xffffffff) for v in R.bits(slots[r, [0, FLOOR, AMAX]]).tolist()],
                      [hex(v & 0xffffffff) for v in got[r, [0, FLOOR, AMAX]].tolist()]) for r in bad[:5]]
    assert torch.equal(got[600:], _i32(_sentinel()))
    assert got_guard.tolist() == [0, 7] == list(exp_guard)
    # a flag an earlier micro-step raised survives a clean launch
    rc, got, got_guard = _finish(buf, [1, 7], 600)
    assert rc == 0 and got_guard.tolist() == [1, 7] and torch.equal(got[:600], _i32(exp_slots))


@pytest.mark.parametrize("name,amax,scale", R.flagged_rows(), ids=[r[0] for r in R.flagged_rows()])
def test_finish_rows_that_raise_the_flag(name, amax, scale):
    """n = 257 with the row at index 256 (the second workgroup's only live thread): flag raised, the slot's words per the law,
    guard[1] and the slot behind untouched."""
    slots = R.from_bits(np.full((257, S), 0x3c3c3c3c, np.uint32)).copy()
    slots[:, 0], slots[:, FLOOR], slots[:, AMAX] = 1.0, 0.0, 0.0
    slots[256, 0], slots[256, FLOOR], slots[256, AMAX] = scale, 0.5, amax
    exp_slots, exp_guard = R.finish(slots, [0, 7])
    assert list(exp_guard) == [1, 7]
    rc, got, guard = _finish(np.concatenate([slots, _sentinel()]), [0, 7], 257)
    assert rc == 0 and guard.tolist() == [1, 7]
    assert torch.equal(got[:257], _i32(exp_slots)), got[256, [0, FLOOR, AMAX]].tolist()
    assert torch.equal(got[257:], _i32(_sentinel()))


def test_finish_of_no_slots_changes_nothing():
    slots, guard = R.finish_tables()[0]
    rc, got, got_guard = _finish(slots[:4], [0, 7], 0, tail=4)
    assert rc == 0 and torch.equal(got, _i32(slots[:4])) and got_guard.tolist() == [0, 7]


# ------------------------------------------------------------------------------------------------- b. writers under a live slot
@pytest.mark.parametrize("masked", [False, True])
@pytest.mark.parametrize("shape", [(3, 16, 8, 4)] + IMG_SHAPES)
def test_to_c16_records_under_a_live_slot(shape, masked):
    from ebfi_amd import c16
    torch.manual_seed(sum(shape))
    x, y = (torch.randn(*shape) * 3).cuda(), torch.randn(*shape).cuda()
    ref = x * torch.where(y > 0, 1.0, 0.01) if masked else x
    book, idx = _new_book(0.25)
    _check_writer(book, idx, lambda: c16.to_c16(x, book.ptr(idx[0]), y if masked else None, 0.01), known=[_amax(ref)])


@pytest.mark.parametrize("shape", IMG_SHAPES)
def test_to_c16_cat2_records_under_a_live_slot(shape):
    from ebfi_amd import c16
    torch.manual_seed(sum(shape))
    B, C, H, W = shape
    a, b = torch.randn(B, C // 2, H, W).cuda(), torch.randn(B, C // 2, H, W).cuda() * 3.0
    book, idx = _new_book(0.5)
    _check_writer(book, idx, lambda: c16.to_c16_cat2(a, b, book.ptr(idx[0])), known=[_amax(a, b)])


@pytest.mark.parametrize("cin,cout", [(64, 64), (64, 72)])
def test_weight_pack_records_under_a_live_slot(cin, cout):
    """ebfi_pack_table_f16 through WeightBank.refresh (72 output channels: image rows padded with table entries of -1)."""
    torch.manual_seed(cout)
    w, b, bank, book, site = _banked(cin, cout)
    bank.refresh()                              # (first use: calibrates the slot; from here on refresh() is the pack launch alone)
    _set_words(book, site.w_slot, amax=0, floor=0)
    _check_writer(book, [site.w_slot], bank.refresh, known=[_amax(w)])


@pytest.mark.parametrize("shape", IMG_SHAPES)
def test_fused_residual_control_stages_record_under_a_live_slot(shape):
    from ebfi_amd import c16
    torch.manual_seed(sum(shape))
    B, C, H, W = shape
    HW = H * W
    a = torch.randn(B, 2 * C, H, W).cuda()
    s0, s1, x = torch.randn(B, C).cuda(), torch.randn(B, C).cuda(), torch.randn(B, C, H, W).cuda()
    gc = torch.randn(B, 2 * C, H, W).cuda() * 1e-2
    book, (so, sg) = _new_book(4.0, 512.0)
    lib, st = N.lib(), N.stream_ptr(a.device)
    a1p = N._vp(a.data_ptr() + 4 * C * HW)
    out, out16 = torch.empty(B, 2 * C, H, W, device="cuda"), c16.empty(B, 2 * C, H, W, "cuda")
    ga16 = c16.empty(B, 2 * C, H, W, "cuda")
    S_ = int(lib.ebfi_scale_residual_cat_backward_slices())
    gx, p0, p1 = torch.empty(B, C, H, W, device="cuda"), torch.empty(S_, B, C, device="cuda"), torch.empty(S_, B, C, device="cuda")

    def fwd():
        N.check(lib.ebfi_scale_residual_cat_forward_c16(N.ptr(a), N.ptr(s0), a1p, N.ptr(s1), N.ptr(x), N.ptr(out), N.ptr(out16), book.ptr(so),
                                                        B, C, H, W, 2 * C * HW, st), "fwd_c16")

    def bwd():
        N.check(lib.ebfi_scale_residual_cat_backward_c16(N.ptr(gc), N.ptr(a), N.ptr(s0), a1p, N.ptr(s1), N.ptr(ga16), book.ptr(sg), N.ptr(gx),
                                                         N.ptr(p0), N.ptr(p1), B, C, H, W, 2 * C * HW, 0.01, st), "bwd_c16")
    _check_writer(book, [so], fwd)
    _check_writer(book, [sg], bwd)


@pytest.mark.parametrize("planar", [0, 1])
@pytest.mark.parametrize("shape", IMG_SHAPES)
def test_forward_conv_side_image_records_under_a_live_slot(shape, planar):
    from ebfi_amd import c16
    torch.manual_seed(sum(shape) + planar)
    B, C, H, W = shape
    w, b, bank, book, site = _banked(C, 64)
    bank.refresh()
    (i,) = _more_slots(book, 2.0)
    x = torch.randn(B, C, H, W).cuda()
    out = torch.empty(B, 64, H, W, device="cuda")
    img = torch.empty(B, 64, H, W, dtype=torch.float16, device="cuda") if planar else c16.empty(B, 64, H, W, "cuda")
    lib, st = N.lib(), N.stream_ptr(x.device)

    def launch():
        N.check(lib.ebfi_conv2d_packed_x3_c16(N.ptr(x), site.fwd_ptr(), site.fwd_bytes, N.ptr(site.bias()), N.ptr(None if planar else out), B, C, H, W, 64,
                                              3, 1, 1, 1, 0.01, N.ptr(None), N.ptr(None), 0, 0.0, N.ptr(img), book.ptr(i), planar, st), "x3_c16")
    _check_writer(book, [i], launch)


@pytest.mark.parametrize("shape", IMG_SHAPES)
def test_residual_control_epilogue_images_record_under_a_live_slot(shape):
    """ebfi_conv2d_packed_x3_rc: the image of the activation output (pre16) and of the round's output (out16), one slot each."""
    from ebfi_amd import c16
    torch.manual_seed(sum(shape))
    B, C, H, W = shape
    w, b, bank, book, site = _banked(C, 2 * C, groups=2)
    bank.refresh()
    sa_, sc_ = _more_slots(book, 8.0, 4.0)
    ya, x = torch.randn(B, 2 * C, H, W).cuda(), torch.randn(B, C, H, W).cuda()
    s_cat = torch.randn(B, 2 * C).cuda()
    c_out = torch.empty(B, 2 * C, H, W, device="cuda")
    c16_out, a16 = c16.empty(B, 2 * C, H, W, "cuda"), c16.empty(B, 2 * C, H, W, "cuda")
    lib, st = N.lib(), N.stream_ptr(x.device)

    def launch():
        N.check(lib.ebfi_conv2d_packed_x3_rc(N.ptr(ya), site.fwd_ptr(), site.fwd_bytes, N.ptr(site.bias()), N.ptr(c_out), B, C, H, W, 2 * C, 2,
                                             0.01, N.ptr(s_cat), N.ptr(x), C, N.ptr(a16), book.ptr(sa_), N.ptr(c16_out), book.ptr(sc_), st), "x3_rc")
    _check_writer(book, [sa_, sc_], launch)


@pytest.mark.parametrize("shape", IMG_SHAPES)
def test_data_gradient_records_under_a_live_slot(shape):
    """ebfi_conv2d_packed_f16 (fp32 gradient in: its slot records max|g| exactly) and ebfi_conv2d_packed_f16_c16 (fp32 in + image
    out: both slots; image in: the input slot is only READ -- its writer recorded -- and stays what it is in every state)."""
    from ebfi_amd import c16
    torch.manual_seed(sum(shape))
    B, C, H, W = shape
    w, b, bank, book, site = _banked(C, 64)
    bank.refresh()
    si, so, sr = _more_slots(book, 1.0, 64.0, 1.0)
    g = torch.randn(B, 64, H, W).cuda()
    out, out16 = torch.empty(B, C, H, W, device="cuda"), c16.empty(B, C, H, W, "cuda")
    lib, st = N.lib(), N.stream_ptr(g.device)

    def plain():
        N.check(lib.ebfi_conv2d_packed_f16(N.ptr(g), site.tr16_ptr(), site.tr16_bytes, N.ptr(None), N.ptr(out), B, 64, H, W, C, 3, 1, 1, 0, 0.0,
                                           N.ptr(None), N.ptr(None), 0, 0.0, book.ptr(si), site.w_slot_ptr(), st), "f16")

    def run(inp, is16, in_slot, o16, o_slot):
        N.check(lib.ebfi_conv2d_packed_f16_c16(N.ptr(inp), is16, site.tr16_ptr(), site.tr16_bytes, N.ptr(None), N.ptr(out), B, 64, H, W, C, 3, 1,
                                               1, 0, 0.0, N.ptr(None), N.ptr(None), 0, 0.0, book.ptr(in_slot), site.w_slot_ptr(), N.ptr(o16),
                                               book.ptr(o_slot) if o16 is not None else N.ptr(None), 0, 0, st), "f16_c16")
    _check_writer(book, [si], plain, known=[_amax(g)])
    _set_words(book, si, amax=0, floor=0)
    _check_writer(book, [si, so], lambda: run(g, 0, si, out16, so), known=[_amax(g), None])
    g16 = c16.to_c16(g, book.ptr(sr))
    _set_words(book, sr, amax=0, floor=0)
    _check_writer(book, [sr], lambda: run(g16, 1, sr, None, so), records=False)


@pytest.mark.parametrize("shape", IMG_SHAPES + [(1, 64, 13, 38)])
def test_weight_gradient_records_under_a_live_slot(shape):
    """ebfi_conv2d_backward_weight_f16g without an activation: both operands are staged as they are, max|x| and max|g| exactly
    (rows of whole quads: the pixel-major kernel; W = 38: the pair-word kernel).  ebfi_conv2d_backward_weight_f16c reads images:
    it leaves both slots alone in every state."""
    from ebfi_amd import c16
    torch.manual_seed(sum(shape))
    B, C, H, W = shape
    x, g = torch.randn(B, C, H, W).cuda() * 0.3, torch.randn(B, 64, H, W).cuda() * 2e-2
    book, (sx, sg, tx, tg) = _new_book(4.0, 64.0, 4.0, 64.0)
    lib, st = N.lib(), N.stream_ptr(x.device)
    need = int(lib.ebfi_conv2d_backward_weight_workspace(B, C, H, W, 64, 3, 1, 1, N.EBFI_F32))
    ws = torch.empty(max(need, 4), dtype=torch.uint8, device="cuda")
    gw, gb = torch.empty(64, C, 3, 3, device="cuda"), torch.empty(64, device="cuda")

    def f16g():
        N.check(lib.ebfi_conv2d_backward_weight_f16g(N.ptr(x), N.ptr(g), N.ptr(None), N.ptr(gw), N.ptr(gb), N.ptr(None), B, C, H, W, 64, 3, 1, 1,
                                                     0, 0.0, book.ptr(sx), book.ptr(sg), N.ptr(ws), need, st), "f16g")
    _check_writer(book, [sx, sg], f16g, known=[_amax(x), _amax(g)])
    if W % 4 == 0:
        x16, g16 = c16.to_c16(x, book.ptr(tx)), c16.to_c16(g, book.ptr(tg))
        _set_words(book, tx, amax=0, floor=0)
        _set_words(book, tg, amax=0, floor=0)

        def f16c():
            N.check(lib.ebfi_conv2d_backward_weight_f16c(N.ptr(x16), N.ptr(g16), 0, N.ptr(gw), N.ptr(gb), B, C, H, W, 64, 1, book.ptr(tx),
                                                         book.ptr(tg), N.ptr(ws), need, st), "f16c")
        _check_writer(book, [tx, tg], f16c, records=False)


@pytest.mark.parametrize("B,C,H,W,unpadded", [(2, 3, 9, 36, 0), (2, 3, 9, 36, 1), (2, 3, 9, 40, 1)])
def test_fac_backward_records_the_kernel_gradient_under_a_live_slot(B, C, H, W, unpadded):
    """grad_kernel16 of ebfi_fac_backward_p16: four pixels per thread (W = 36, padded and unpadded input) and eight (unpadded,
    W % 8 == 0)."""
    torch.manual_seed(W + unpadded)
    K = 5
    inp = torch.randn(B, C, H, W).cuda() if unpadded else torch.randn(B, C, H + 4, W + 4).cuda()
    filt = torch.randn(B, C * K * K, H, W).cuda() * 0.2
    go = torch.randn(B, C, H, W).cuda() * 1e-2
    book, (sf, sg) = _new_book(8.0, 256.0)
    f16 = (filt * 8.0).half()
    gin = torch.empty_like(inp)
    gk16 = torch.empty(B, C * K * K, H, W, dtype=torch.float16, device="cuda")
    lib, st = N.lib(), N.stream_ptr(inp.device)
    N.prof_reset()
    N.prof_enable(True)

    def launch():
        N.check(lib.ebfi_fac_backward_p16(N.ptr(inp), unpadded, N.ptr(f16), book.ptr(sf), N.ptr(go), N.ptr(gin), N.ptr(gk16), book.ptr(sg), 0.01,
                                          B, C, H, W, K, st), "fac_backward_p16")
    try:
        _check_writer(book, [sg], launch)
    finally:
        N.prof_enable(False)
    ran = {k.split("/")[0] for k, v in N.prof_collect().items() if v[0] > 0}
    assert ("fac_bwd_rows_p16x8" in ran) == (unpadded == 1 and W % 8 == 0), ran
    assert torch.equal(_words(book, sf)[[0, FLOOR, AMAX]], torch.tensor([_fbits(8.0), 0, 0], dtype=torch.int32))     # the filter slot is read only


# ------------------------------------------------------------------------------------------------ c. the maximum in the corners
CORNER_SHAPES = IMG_SHAPES + [(2, 64, 13, 36)]           # + the ragged tiles with a second sample behind the first one's tail


def _corners(shape):
    """First element; last element (= last column of the last row of the last channel); last element of sample 0."""
    B, C, H, W = shape
    return sorted({(0, 0, 0, 0), (B - 1, C - 1, H - 1, W - 1), (0, C - 1, H - 1, W - 1)})


def _spiked(x, pos, k):
    y = x.clone()
    y[pos] = 3.0 if k % 2 == 0 else -3.0
    return y


def _expect_three(book, i, launch):
    """Slot i with no maximum yet and a floor of 2: after `launch` it holds exactly 3.0; scale, floor and the rest untouched."""
    _set_words(book, i, amax=0, floor=_fbits(2.0))
    before = _words(book, i)
    launch()
    torch.cuda.synchronize()
    exp = before.clone()
    exp[AMAX] = _fbits(3.0)
    assert torch.equal(_words(book, i), exp), [hex(v) for v in _words(book, i)[[0, FLOOR, AMAX]].tolist()]
    assert torch.equal(exp, _i32(R.record(before.numpy().view(np.float32), _fbits(3.0))))


@pytest.mark.parametrize("shape", [(3, 16, 8, 4)] + CORNER_SHAPES)
def test_to_c16_finds_a_maximum_on_the_first_and_the_last_element(shape):
    from ebfi_amd import c16
    torch.manual_seed(1)
    x = (torch.rand(*shape) * 2 - 1).cuda()
    book, (i,) = _new_book(0.25)
    for k, pos in enumerate(_corners(shape)):
        xb = _spiked(x, pos, k)
        _expect_three(book, i, lambda: c16.to_c16(xb, book.ptr(i)))
    B, C, H, W = shape
    if C >= 32:
        a, b = x[:, :C // 2].contiguous(), x[:, C // 2:].contiguous()
        for k, pos in enumerate(_corners((B, C // 2, H, W))):
            ab, bb = _spiked(a, pos, k), _spiked(b, pos, k + 1)
            _expect_three(book, i, lambda: c16.to_c16_cat2(ab, b, book.ptr(i)))
            _expect_three(book, i, lambda: c16.to_c16_cat2(a, bb, book.ptr(i)))


@pytest.mark.parametrize("cout", [64, 72])
def test_weight_pack_finds_a_maximum_on_the_first_and_the_last_weight(cout):
    torch.manual_seed(2)
    w0 = torch.rand(cout, 64, 3, 3) * 2 - 1
    for k, pos in enumerate(_corners(tuple(w0.shape))):
        w, b, bank, book, site = _banked(64, cout, w=_spiked(w0, pos, k))
        bank.refresh()
        _expect_three(book, site.w_slot, bank.refresh)


@pytest.mark.parametrize("shape", CORNER_SHAPES + [(1, 64, 13, 38), (2, 64, 13, 38)])
def test_backward_convs_find_a_maximum_on_the_first_and_the_last_element(shape):
    """x and g of the fp16 weight gradient (both kernels), g of the fp16 data gradient (rows of whole quads: the fp16 data
    gradient does not take W = 38, those layers keep the split-precision form, which has no slot)."""
    torch.manual_seed(3)
    B, C, H, W = shape
    x, g = (torch.rand(B, C, H, W) * 2 - 1).cuda(), (torch.rand(B, 64, H, W) * 2 - 1).cuda()
    w, b, bank, book, site = _banked(C, 64)
    bank.refresh()
    sx, sg, sd = _more_slots(book, 1.0, 1.0, 1.0)
    lib, st = N.lib(), N.stream_ptr(x.device)
    need = int(lib.ebfi_conv2d_backward_weight_workspace(B, C, H, W, 64, 3, 1, 1, N.EBFI_F32))
    ws = torch.empty(max(need, 4), dtype=torch.uint8, device="cuda")
    gw, gb, gx = torch.empty(64, C, 3, 3, device="cuda"), torch.empty(64, device="cuda"), torch.empty(B, C, H, W, device="cuda")

    def wgrad(xt, gt):
        N.check(lib.ebfi_conv2d_backward_weight_f16g(N.ptr(xt), N.ptr(gt), N.ptr(None), N.ptr(gw), N.ptr(gb), N.ptr(None), B, C, H, W, 64, 3, 1, 1,
                                                     0, 0.0, book.ptr(sx), book.ptr(sg), N.ptr(ws), need, st), "f16g")

    def dgrad(gt):
        N.check(lib.ebfi_conv2d_packed_f16(N.ptr(gt), site.tr16_ptr(), site.tr16_bytes, N.ptr(None), N.ptr(gx), B, 64, H, W, C, 3, 1, 1, 0, 0.0,
                                           N.ptr(None), N.ptr(None), 0, 0.0, book.ptr(sd), site.w_slot_ptr(), st), "f16")
    for k, pos in enumerate(_corners(shape)):
        xb, gb_ = _spiked(x, pos, k), _spiked(g, pos, k + 1)
        _set_words(book, sg, amax=0, floor=_fbits(2.0))
        _expect_three(book, sx, lambda: wgrad(xb, g))
        assert _words(book, sg)[AMAX] == 0                       # (g stayed below its floor of 2)
        _set_words(book, sx, amax=0, floor=_fbits(2.0))
        _expect_three(book, sg, lambda: wgrad(x, gb_))
        assert _words(book, sx)[AMAX] == 0
        if W % 4 == 0:
            _expect_three(book, sd, lambda: dgrad(gb_))


# ------------------------------------------------------------------------------------------------- d. closed loop on one layer
def test_one_layer_closed_loop_follows_the_slot_law():
    """begin_step, conv backward, finish, guarded Adam (lr = 0) on a 64 -> 64 layer without activation, the incoming gradient
    scaled by k_t.  After every step the g and x slots (all 64 words), the guard and the skip count equal the model built from
    scale_ref (next_scale for the first use, record per operand, finish); gradients are held to the fp32 CPU convolution (1e-3)
    whenever both operands sat in [1, 4) under the scale in use, and are finite on every other step that is not flagged.

    The 2^-12 phase lasts until the step at which the model re-measures the g slot: the floor 7/8 * 0.5 must halve 11 times
    (ceil(log2(0.875 / 2^-11))), the twelfth 2^-12 step is recorded.  Flagged steps, by the law: the first 2^20 step and the NaN
    step -- and the 64 step, which stands 2^18 above the scale that the re-measured 2^-12 gradient had just been given (|max| *
    scale = 3.75 * 2^18 > 60000); max|g| is set to 3.75 so that the first 2^20 step (2^14 above the 64 step's scale: 61440)
    is past 60000 whatever the seed."""
    from ebfi_amd import conv, weightbank
    from ebfi_amd.dp import FlatAdam, FlatGradBucket
    torch.manual_seed(3)
    w, b, bank, book, site = _banked(64, 64)
    bank.refresh()
    net = torch.nn.ParameterList([w, b])
    opt, bucket = FlatAdam(list(net.parameters()), lr=0.0), FlatGradBucket(net)
    bank2 = weightbank.WeightBank(opt.params, flat=opt.flat.data)
    w2, b2 = opt.params
    bank2.register(w2, b2, "id")
    bank2.attach_scale_book(book)
    x = torch.randn(1, 64, 16, 64).cuda()
    g = torch.randn(1, 64, 16, 64).clamp(-3.5, 3.5)
    g[0, 5, 3, 7] = 3.75
    g = g.cuda()
    # fp32 CPU reference, once: the backward is linear in the incoming gradient
    xr, wr, br = x.cpu().requires_grad_(), w2.detach().cpu().requires_grad_(), b2.detach().cpu().requires_grad_()
    torch.nn.functional.conv2d(xr, wr, br, padding=1).backward(g.cpu())
    rel = lambda a, r: ((a.cpu() - r).abs().max() / r.abs().max()).item()

    model = {"g": np.zeros(S, np.float32), "x": np.zeros(S, np.float32)}
    for v in model.values():
        v[0] = 1.0
    skipped, flagged, done, n12 = 0, [], 0, 0
    phases = [1, 1, 1.1, 0.9, 0.8, 0.5, 0.5, "drop", 64, 2.0 ** 20, 2.0 ** 20, 0, 1, "nan", 1]
    names = []
    conv.set_compute_dtype("bf16x3")
    try:
        for phase in phases:
            while True:
                k = 2.0 ** -12 if phase == "drop" else 1 if phase == "nan" else phase
                gk = g * k
                if phase == "nan":
                    gk[0, 37, 5, 11] = float("nan")
                # ---- device
                bucket.zero()
                bank2.refresh()
                with bank2.active(), book.active():
                    book.begin_step()
                    xd = x.clone().requires_grad_()
                    conv.conv_bias_act(xd, w2, b2, 1, 1, 0, 0.0).backward(gk)
                    gx, gw, gb = xd.grad.clone(), w2.grad.clone(), b2.grad.clone()
                    book.finish()
                opt.step(bucket.gather(), guard=book.guard)
                torch.cuda.synchronize()
                # ---- model
                m_bits = {"g": int(gk.abs().max().reshape(1).view(torch.int32).item()), "x": int(x.abs().max().reshape(1).view(torch.int32).item())}
                in_range, remeasured = True, False
                for name in ("g", "x"):
                    if done == 0:
                        model[name][0] = R.next_scale(R.from_bits(np.array([m_bits[name]], np.uint32)))[0]
                    after = R.record(model[name], m_bits[name])
                    if name == "g":
                        remeasured = R.bits(after[AMAX:AMAX + 1])[0] != 0
                    model[name] = after
                    prod = float(R.from_bits(np.array([m_bits[name]], np.uint32))[0]) * float(after[0])
                    in_range = in_range and 1.0 <= prod < 4.0
                both, guard = R.finish(np.stack([model["g"], model["x"]]), [0, skipped])
                model["g"], model["x"] = both[0].copy(), both[1].copy()
                flag = int(guard[0])
                skipped += flag
                done += 1
                names.append(phase)
                if flag:
                    flagged.append((phase, done))
                # ---- compare
                key = (w2.data_ptr(), "id")
                for name in ("g", "x"):
                    got = _words(book, book.index[(key, name)])
                    assert torch.equal(got, _i32(model[name])), (done, phase, name, got[[0, FLOOR, AMAX]].tolist(),
                                                                 R.bits(model[name][[0, FLOOR, AMAX]]).tolist())
                assert book.guard.tolist() == [flag, skipped], (done, phase, book.guard.tolist(), flag, skipped)
                assert book.skipped_steps() == skipped
                assert float(opt.inner.state[opt.flat]["step"]) == done - skipped          # a skipped step does not count
                if in_range and not flag:
                    assert rel(gx, xr.grad * k) < 1e-3 and rel(gw, wr.grad * k) < 1e-3 and rel(gb, br.grad * k) < 1e-3, (done, phase)
                elif not flag:
                    assert torch.isfinite(gx).all() and torch.isfinite(gw).all() and torch.isfinite(gb).all(), (done, phase)
                if phase != "drop":
                    break
                n12 += 1
                if remeasured:
                    break
                assert n12 < 40
    finally:
        conv.set_compute_dtype("fp32")
    assert n12 == 12                                  # 11 idle steps, then the step that is measured again
    first_big = names.index(2.0 ** 20) + 1
    assert flagged == [(64, first_big - 1), (2.0 ** 20, first_big), ("nan", done - 1)], flagged
    assert skipped == 3
