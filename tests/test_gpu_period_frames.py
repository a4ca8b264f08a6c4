"""ebfi_amd.frameio.period_to_planar (csrc/frameio.hip, ebfi_period_frames_u8): the sharp planes and the exposure mean of one
training period from its stored uint8 frames, against the CPU expressions of the reference's reader, bit for bit.

    sharp == torch.from_numpy(a).permute(0, 3, 1, 2).float() / 255                       (h5dataset.py:296-310)
    blur  == torch.from_numpy(a[:e].mean(0)).permute(2, 0, 1).float() / 255              (h5dataset.py:311)

with the window, the channel reversal and the flips applied to both.  The mean rounds three times (float64 quotient, float32,
float32 / 255): the first test feeds every possible byte sum for every exposure 1..16, on the scalar and on the vector path.
The shapes are those of test_gpu_frameio.py -- every size at which the entry point takes another path."""
import ctypes

import numpy as np
import pytest
import torch

from ebfi_amd import _native as N
from ebfi_amd import frameio

# (H0, W0, window): window None = the whole frame
CASES = {
    "ragged_5x7": (5, 7, None),                   # tail-only width: the scalar path
    "odd_origin_crop": (26, 34, (5, 5, 16, 24)),  # rows start at odd bytes: 16-byte stores, byte loads
    "aligned_8x32": (8, 32, None),                # the vector path on both sides
    "aligned_window": (8, 32, (1, 4, 6, 24)),     # a window that keeps dword loads (j % 4 == 0)
    "unaligned_window": (8, 32, (0, 2, 8, 28)),   # w % 4 == 0, j % 4 != 0: byte loads
    "many_blocks": (40, 132, (3, 0, 36, 128)),    # 36 * 32 = 1152 threads: more than one block
}
FLIPS = [(False, False), (True, False), (False, True), (True, True)]
N_AND_E = [(n, e) for n in (1, 3, 16) for e in sorted({1, min(2, n), n})]


def _frames(n, H, W, seed):
    a = np.random.RandomState(seed).randint(0, 256, size=(n, H, W, 3)).astype(np.uint8)
    a.reshape(-1)[:256] = np.arange(256, dtype=np.uint8)
    return a


def _view(ref, window, rev, fh, fv):
    """Window, channel order and flips on a [..., 3, H, W] CPU reference (pure indexing: no arithmetic)."""
    if window is not None:
        i, j, h, w = window
        ref = ref[..., i:i + h, j:j + w]
    if rev:
        ref = ref[..., [2, 1, 0], :, :]
    if fh:
        ref = ref.flip(-1)
    if fv:
        ref = ref.flip(-2)
    return ref.contiguous()


def _cpu_sharp(a):
    return torch.from_numpy(a).permute(0, 3, 1, 2).float() / 255


def _cpu_blur(a, e):
    return torch.from_numpy(a[:e].mean(0)).permute(2, 0, 1).float() / 255


def _same_bits(a, b):
    return a.shape == b.shape and a.dtype == b.dtype and np.array_equal(a.cpu().numpy().view(np.uint32), b.cpu().numpy().view(np.uint32))


def _staircase(W, seed=0):
    """[16, 1, W, 3]: frame k holds clip(s - 255 k, 0, 255) at element s, so the sum over the first e frames is min(s, 255 e):
    every possible sum of e bytes.  Elements past 4080 (the padding of a width) hold random bytes."""
    s = np.arange(W * 3, dtype=np.int64)
    a = np.stack([np.clip(s - 255 * k, 0, 255) for k in range(16)]).astype(np.uint8)
    pad = s > 4080
    a[:, pad] = np.random.RandomState(seed).randint(0, 256, size=(16, int(pad.sum()))).astype(np.uint8)
    return a.reshape(16, 1, W, 3)


@pytest.mark.gpu
@pytest.mark.parametrize("W", [1361, 1364], ids=["scalar_1361", "vector_1364"])
def test_the_mean_rounds_like_the_host_expression_at_every_byte_sum(W):
    a = _staircase(W)
    dev = torch.from_numpy(a).cuda()
    sharp_ref = _cpu_sharp(a)
    for e in range(1, 17):
        sums = a[:e].astype(np.int64).sum(0).reshape(-1)
        assert set(range(255 * e + 1)) <= set(sums.tolist())                # the inputs are exhaustive for this exposure
        sharp, blur = frameio.period_to_planar(dev, e)
        ref = _cpu_blur(a, e)
        bad = int((blur.cpu().numpy().view(np.uint32) != ref.numpy().view(np.uint32)).sum())
        assert bad == 0, (e, bad)
        assert _same_bits(sharp, sharp_ref), e
    # ... and they discriminate: the fused division sum / (255 e) is another function on exactly these inputs
    e = 3
    s = torch.from_numpy(a[:e].astype(np.int64).sum(0).reshape(-1)[:766].astype(np.float32))
    assert s.tolist() == list(range(766))
    fused = s / torch.tensor(255.0 * e)
    host = (s.double() / e).float() / 255
    assert fused.dtype == host.dtype == torch.float32 and int((fused != host).sum()) == 167


@pytest.mark.gpu
@pytest.mark.parametrize("case", sorted(CASES))
def test_period_to_planar_is_the_cpu_expression(case):
    H, W, window = CASES[case]
    a16 = _frames(16, H, W, seed=len(case))
    dev16 = torch.from_numpy(a16).cuda()
    sharp16 = _cpu_sharp(a16)
    for n, e in N_AND_E:
        blur_ref = _cpu_blur(a16[:n], e)
        for rev in (False, True):
            for fh, fv in FLIPS:
                sharp, blur = frameio.period_to_planar(dev16[:n], e, window=window, reverse_channels=rev, flip_h=fh, flip_v=fv)
                assert _same_bits(sharp, _view(sharp16[:n], window, rev, fh, fv)), (case, n, e, rev, fh, fv)
                assert _same_bits(blur, _view(blur_ref, window, rev, fh, fv)), (case, n, e, rev, fh, fv)
                # the sharp side is the existing kernel's output, bit for bit
                assert _same_bits(sharp, frameio.frames_to_planar(dev16[:n], window=window, reverse_channels=rev, flip_h=fh,
                                                                  flip_v=fv))


@pytest.mark.gpu
@pytest.mark.parametrize("case", ["aligned_8x32", "odd_origin_crop", "ragged_5x7"])
def test_period_to_planar_reads_a_view_at_a_one_byte_offset(case):
    """The source starts one byte into its allocation: no 4-byte load may be used, whatever the shape says."""
    H, W, window = CASES[case]
    a = _frames(3, H, W, seed=7)
    buf = torch.zeros(a.size + 1, dtype=torch.uint8, device="cuda")
    buf[1:].copy_(torch.from_numpy(a).reshape(-1))
    view = buf[1:].view(3, H, W, 3)
    assert view.data_ptr() % 4 == 1
    for rev, (fh, fv) in ((False, (False, False)), (True, (True, True))):
        sharp, blur = frameio.period_to_planar(view, 2, window=window, reverse_channels=rev, flip_h=fh, flip_v=fv)
        assert _same_bits(sharp, _view(_cpu_sharp(a), window, rev, fh, fv)), (case, rev, fh, fv)
        assert _same_bits(blur, _view(_cpu_blur(a, 2), window, rev, fh, fv)), (case, rev, fh, fv)


@pytest.mark.gpu
@pytest.mark.parametrize("case", ["aligned_window", "odd_origin_crop", "ragged_5x7"])
def test_period_to_planar_reads_a_slice_of_a_larger_clip(case):
    """The period is frames i0 .. i0 + n of an uploaded clip whose frames are taller and wider than the view handed in: the
    frame stride is neither h * w * 3 of the window nor H0 * W0 * 3 of the view."""
    H, W, window = CASES[case]
    clip = _frames(7, H + 2, W + 3, seed=11)
    dev = torch.from_numpy(clip).cuda()
    for i0, n, e in ((0, 3, 2), (2, 4, 4), (4, 3, 1)):
        view = dev[i0:i0 + n, 1:1 + H, 3:]
        host = np.ascontiguousarray(clip[i0:i0 + n, 1:1 + H, 3:])
        assert view.stride(0) != H * W * 3 and tuple(view.shape) == (n, H, W, 3)
        sharp, blur = frameio.period_to_planar(view, e, window=window, reverse_channels=True, flip_h=True)
        assert _same_bits(sharp, _view(_cpu_sharp(host), window, True, True, False)), (case, i0)
        assert _same_bits(blur, _view(_cpu_blur(host, e), window, True, True, False)), (case, i0)
    every_second = dev[::2][:3]                                           # a frame stride of two frames
    sharp, blur = frameio.period_to_planar(every_second, 3, window=None)
    host = np.ascontiguousarray(clip[::2][:3])
    assert _same_bits(sharp, _cpu_sharp(host)) and _same_bits(blur, _cpu_blur(host, 3))


@pytest.mark.gpu
@pytest.mark.parametrize("case", ["aligned_8x32", "odd_origin_crop", "ragged_5x7"])
def test_period_to_planar_fills_slices_of_larger_tensors(case):
    """sharp_out / blur_out are slots of batch tensors; one pair starts a single float into its allocation (4-byte aligned
    only: the 16-byte stores must not be used, whatever the width says).  Nothing outside the slot is written."""
    H, W, window = CASES[case]
    n, e = 3, 2
    a = _frames(n, H, W, seed=5)
    dev = torch.from_numpy(a).cuda()
    h, w = (H, W) if window is None else window[2:]
    sharp_ref, blur_ref = _view(_cpu_sharp(a), window, True, False, True), _view(_cpu_blur(a, e), window, True, False, True)
    batch_sharp = torch.full((3, 1, 1, n, 3, h, w), -7.0, device="cuda")
    batch_blur = torch.full((3, 1, 1, 3, h, w), -7.0, device="cuda")
    s, b = frameio.period_to_planar(dev, e, window=window, reverse_channels=True, flip_v=True, sharp_out=batch_sharp[1, 0, 0],
                                    blur_out=batch_blur[1, 0, 0])
    assert s.data_ptr() == batch_sharp[1].data_ptr() and b.data_ptr() == batch_blur[1].data_ptr()
    assert _same_bits(batch_sharp[1, 0, 0], sharp_ref) and _same_bits(batch_blur[1, 0, 0], blur_ref)
    assert (batch_sharp[[0, 2]] == -7).all() and (batch_blur[[0, 2]] == -7).all()
    # one float into an allocation: sharp, then blur, then both
    for off_s, off_b in ((1, 0), (0, 1), (1, 1)):
        sbuf = torch.full((n * 3 * h * w + 2,), -7.0, device="cuda")
        bbuf = torch.full((3 * h * w + 2,), -7.0, device="cuda")
        s_out = sbuf[off_s:off_s + n * 3 * h * w].view(n, 3, h, w)
        b_out = bbuf[off_b:off_b + 3 * h * w].view(3, h, w)
        assert s_out.data_ptr() % 16 == 4 * off_s and b_out.data_ptr() % 16 == 4 * off_b
        frameio.period_to_planar(dev, e, window=window, reverse_channels=True, flip_v=True, sharp_out=s_out, blur_out=b_out)
        assert _same_bits(s_out, sharp_ref) and _same_bits(b_out, blur_ref), (case, off_s, off_b)
        for buf, off, size in ((sbuf, off_s, n * 3 * h * w), (bbuf, off_b, 3 * h * w)):
            assert (buf[:off] == -7).all() and (buf[off + size:] == -7).all()
    with pytest.raises(ValueError, match="sharp_out"):
        frameio.period_to_planar(dev, e, window=window, sharp_out=torch.empty(n, 3, h, w + 1, device="cuda"))
    with pytest.raises(ValueError, match="blur_out"):
        frameio.period_to_planar(dev, e, window=window, blur_out=torch.empty(3, w, h, device="cuda").transpose(1, 2))


@pytest.mark.gpu
def test_period_frames_refuses_bad_arguments():
    lib = N.lib()
    s3 = (ctypes.c_int64 * 3)(48, 12, 3)
    p = ctypes.c_void_p(16)
    ok = (4, 4, 0, 0, 4, 4, 0, 0, 0)
    assert lib.ebfi_period_frames_u8(p, s3, 2, 0, *ok, p, p, None) == -1 and b"n_blur" in lib.ebfi_last_error()
    assert lib.ebfi_period_frames_u8(p, s3, 2, 3, *ok, p, p, None) == -1 and b"n_blur" in lib.ebfi_last_error()
    assert lib.ebfi_period_frames_u8(p, s3, 0, 0, *ok, p, p, None) == -1
    assert lib.ebfi_period_frames_u8(p, s3, 2, 1, *ok, None, p, None) == -1 and b"null" in lib.ebfi_last_error()
    assert lib.ebfi_period_frames_u8(p, s3, 2, 1, *ok, p, None, None) == -1 and b"null" in lib.ebfi_last_error()
    assert lib.ebfi_period_frames_u8(None, s3, 2, 1, *ok, p, p, None) == -1 and b"null" in lib.ebfi_last_error()
    for win in ((0, 0, 5, 4), (1, 0, 4, 4), (0, 2, 4, 3), (-1, 0, 2, 2), (0, 0, 0, 4)):
        assert lib.ebfi_period_frames_u8(p, s3, 2, 1, 4, 4, *win, 0, 0, 0, p, p, None) == -1 and b"window" in lib.ebfi_last_error()
    assert lib.ebfi_period_frames_u8(p, (ctypes.c_int64 * 3)(48, 12, 2), 2, 1, *ok, p, p, None) == -1
    # the wrapper: errors of the library become exceptions, and nothing is written
    frames = torch.zeros(2, 4, 4, 3, dtype=torch.uint8, device="cuda")
    for e in (0, 3):
        with pytest.raises(N.EbfiNativeError, match="n_blur"):
            frameio.period_to_planar(frames, e)
    with pytest.raises(N.EbfiNativeError, match="window"):
        frameio.period_to_planar(frames, 1, window=(2, 0, 4, 4))
    with pytest.raises(ValueError):
        frameio.period_to_planar(frames.float(), 1)
