"""ebfi_amd.frameio (csrc/frameio.hip): the uint8 -> planar float upload kernel and the planar float -> uint8 download kernel
against the CPU expressions they replace, bit for bit.

    frames_to_planar == torch.from_numpy(a).permute(0, 3, 1, 2).float() / 255          (h5dataset_realdata.py:189)
    planar_to_u8     == (x.clamp(0, 1) * 255).cpu().numpy().transpose(0, 2, 3, 1).astype('uint8')      (infer_ours.py:135)

Shapes: every size at which the entry points take another path -- a width that is no multiple of four pixels (scalar), a
window at an odd origin (16-byte stores, byte loads), an aligned full frame (16-byte stores, dword loads), views whose storage
starts one byte / one float into an allocation (the alignment checks must see the real pointer), more than one block."""
import numpy as np
import pytest
import torch

from ebfi_amd import _native as N
from ebfi_amd import frameio

# (n, H0, W0, window): window None = the whole frame
UPLOAD_CASES = {
    "all_bytes_16x16": (1, 16, 16, None),            # every byte value, 16-byte stores + dword loads
    "ragged_5x7": (3, 5, 7, None),                   # tail-only width: the scalar path
    "odd_origin_crop": (2, 26, 34, (5, 5, 16, 24)),  # the fixture's centre crop: rows start at odd bytes, 16-byte stores
    "aligned_8x32": (2, 8, 32, None),                # the vector path on both sides
    "aligned_window": (2, 8, 32, (1, 4, 6, 24)),     # a window that keeps dword loads (j % 4 == 0)
    "unaligned_window": (2, 8, 32, (0, 2, 8, 28)),   # w % 4 == 0, j % 4 != 0: byte loads
    "many_blocks": (3, 40, 132, (3, 0, 36, 128)),    # 3 * 36 * 32 = 3456 threads: more than one block
}
FLIPS = [(False, False), (True, False), (False, True), (True, True)]


def _frames(n, H, W, seed):
    a = np.random.RandomState(seed).randint(0, 256, size=(n, H, W, 3)).astype(np.uint8)
    a.reshape(-1)[:256] = np.arange(256, dtype=np.uint8)           # every byte value, whatever the draw
    return a


def _cpu_planar(a, window, rev, fh, fv):
    ref = torch.from_numpy(a).permute(0, 3, 1, 2).float() / 255
    if window is not None:
        i, j, h, w = window
        ref = ref[..., i:i + h, j:j + w]
    if rev:
        ref = ref[:, [2, 1, 0]]
    if fh:
        ref = ref.flip(-1)
    if fv:
        ref = ref.flip(-2)
    return ref.contiguous()


def _same_bits(a, b):
    return a.shape == b.shape and a.dtype == b.dtype and np.array_equal(a.cpu().numpy().view(np.uint32), b.cpu().numpy().view(np.uint32))


@pytest.mark.gpu
@pytest.mark.parametrize("case", sorted(UPLOAD_CASES))
def test_frames_to_planar_is_the_cpu_expression(case):
    n, H, W, window = UPLOAD_CASES[case]
    a = _frames(n, H, W, seed=len(case))
    if case == "all_bytes_16x16":
        a = (np.arange(768) % 256).astype(np.uint8).reshape(1, 16, 16, 3)
    dev = torch.from_numpy(a).cuda()
    for rev in (False, True):
        for fh, fv in FLIPS:
            got = frameio.frames_to_planar(dev, window=window, reverse_channels=rev, flip_h=fh, flip_v=fv)
            assert _same_bits(got, _cpu_planar(a, window, rev, fh, fv)), (case, rev, fh, fv)


@pytest.mark.gpu
@pytest.mark.parametrize("case", ["aligned_8x32", "odd_origin_crop", "ragged_5x7"])
def test_frames_to_planar_reads_a_view_at_a_one_byte_offset(case):
    """The source starts one byte into its allocation: no 4-byte load may be used, whatever the shape says."""
    n, H, W, window = UPLOAD_CASES[case]
    a = _frames(n, H, W, seed=7)
    buf = torch.zeros(a.size + 1, dtype=torch.uint8, device="cuda")
    buf[1:].copy_(torch.from_numpy(a).reshape(-1))
    view = buf[1:].view(n, H, W, 3)
    assert view.data_ptr() % 4 == 1
    for rev, (fh, fv) in ((False, (False, False)), (True, (True, True))):
        got = frameio.frames_to_planar(view, window=window, reverse_channels=rev, flip_h=fh, flip_v=fv)
        assert _same_bits(got, _cpu_planar(a, window, rev, fh, fv)), (case, rev, fh, fv)
    # ... and a strided source: every second frame of a batch, rows of a wider image
    wide = _frames(2 * n, H, W + 3, seed=8)
    got = frameio.frames_to_planar(torch.from_numpy(wide).cuda()[::2, :, 3:], window=window)
    assert _same_bits(got, _cpu_planar(np.ascontiguousarray(wide[::2, :, 3:]), window, False, False, False))


def _numpy_u8(x):
    return (x.clamp(0, 1) * 255).cpu().numpy().transpose(0, 2, 3, 1).astype("uint8")


def _rounding_probe():
    """k / 255 and its two float neighbours for every k: 768 values as [1, 3, 16, 16]."""
    k = (np.arange(256, dtype=np.float32) / np.float32(255)).astype(np.float32)
    v = np.stack([np.nextafter(k, np.float32(-1)), k, np.nextafter(k, np.float32(2))]).astype(np.float32)
    return torch.from_numpy(v.reshape(1, 3, 16, 16))


def _values(n, H, W, seed):
    g = torch.Generator().manual_seed(seed)
    x = torch.rand((n, 3, H, W), generator=g) * 2 - 0.5                     # [-0.5, 1.5): below 0, inside, above 1
    flat = x.view(-1)
    special = torch.tensor([0.0, 1.0, -0.0, -1e-30, 1e-45, 1.0 - 2 ** -24, 1.0 + 2 ** -23, 254.999 / 255, 0.5, -3.0, 7.0, 1 / 255])
    flat[:special.numel()] = special
    return x


@pytest.mark.gpu
def test_planar_to_u8_rounds_like_numpy_at_every_level():
    x = _rounding_probe()
    ref = _numpy_u8(x)
    assert sorted(set(ref.reshape(-1).tolist())) == list(range(256))
    got = frameio.planar_to_u8(x.cuda())
    assert got.dtype == torch.uint8 and np.array_equal(got.cpu().numpy(), ref)
    edge = torch.tensor([0.0, 1.0, -0.0, -5.0, 5.0, 1.0 - 2 ** -24] * 8).view(1, 3, 4, 4)
    assert np.array_equal(frameio.planar_to_u8(edge.cuda()).cpu().numpy(), _numpy_u8(edge))
    assert frameio.planar_to_u8(torch.zeros(1, 3, 4, 4, device="cuda")).sum().item() == 0
    assert (frameio.planar_to_u8(torch.ones(1, 3, 4, 4, device="cuda")) == 255).all()


@pytest.mark.gpu
@pytest.mark.parametrize("shape", [(3, 5, 7), (2, 16, 24), (2, 8, 32), (3, 36, 128)])
def test_planar_to_u8_is_the_numpy_expression(shape):
    n, H, W = shape
    x = _values(n, H, W, seed=H).cuda()
    ref = _numpy_u8(x)
    assert np.array_equal(frameio.planar_to_u8(x).cpu().numpy(), ref)
    # a view that starts one float into its allocation: never 16-byte aligned
    buf = torch.zeros(x.numel() + 1, device="cuda")
    buf[1:].copy_(x.reshape(-1))
    view = buf[1:].view(n, 3, H, W)
    assert view.data_ptr() % 16 == 4
    assert np.array_equal(frameio.planar_to_u8(view).cpu().numpy(), ref)
    # an output that starts one byte into its allocation
    obuf = torch.zeros(n * H * W * 3 + 1, dtype=torch.uint8, device="cuda")
    out = obuf[1:].view(n, H, W, 3)
    assert frameio.planar_to_u8(x, out=out) is out and np.array_equal(out.cpu().numpy(), ref) and obuf[0].item() == 0
    # windows of a larger tensor: row starts off the 16-byte grid, and on it
    big = _values(n, H + 10, W + 12, seed=W).cuda()
    for win in (big[..., 5:5 + H, 5:5 + W], big[..., 2:2 + H, 4:4 + W], big[:, :, 1:1 + H, :W]):
        assert np.array_equal(frameio.planar_to_u8(win).cpu().numpy(), _numpy_u8(win))


@pytest.mark.gpu
def test_planar_to_u8_maps_nan_to_zero_and_infinities_to_the_ends():
    """NaN -> 0 is this kernel's own definition (numpy leaves the cast of NaN undefined, so it is not compared with numpy)."""
    for shape in ((1, 3, 4, 8), (1, 3, 3, 5)):                      # vector and scalar path
        x = torch.full(shape, 0.5, device="cuda")
        x[0, 0, 0, 0], x[0, 1, 1, 2], x[0, 2, 2, 3] = float("nan"), float("inf"), float("-inf")
        got = frameio.planar_to_u8(x)
        assert got[0, 0, 0, 0].item() == 0 and got[0, 1, 2, 1].item() == 255 and got[0, 2, 3, 2].item() == 0
        keep = torch.ones(shape, dtype=torch.bool)
        keep[0, 0, 0, 0] = keep[0, 1, 1, 2] = keep[0, 2, 2, 3] = False
        assert (got.permute(0, 3, 1, 2).cpu()[keep] == 127).all()


def test_frameio_refuses_cpu_tensors_and_bad_arguments():
    with pytest.raises(NotImplementedError):
        frameio.frames_to_planar(torch.zeros(1, 4, 4, 3, dtype=torch.uint8))
    with pytest.raises(NotImplementedError):
        frameio.planar_to_u8(torch.zeros(1, 3, 4, 4))
    lib = N.lib()
    import ctypes
    s3 = (ctypes.c_int64 * 3)(48, 12, 3)
    p = ctypes.c_void_p(16)
    assert lib.ebfi_frames_u8_to_planar(None, s3, 1, 4, 4, 0, 0, 4, 4, 0, 0, 0, p, None) == -1 and b"null" in lib.ebfi_last_error()
    for win in ((0, 0, 5, 4), (1, 0, 4, 4), (0, 2, 4, 3), (-1, 0, 2, 2), (0, 0, 0, 4)):
        assert lib.ebfi_frames_u8_to_planar(p, s3, 1, 4, 4, *win, 0, 0, 0, p, None) == -1 and b"window" in lib.ebfi_last_error()
    assert lib.ebfi_frames_u8_to_planar(p, s3, -1, 4, 4, 0, 0, 4, 4, 0, 0, 0, p, None) == -1
    assert lib.ebfi_frames_u8_to_planar(p, (ctypes.c_int64 * 3)(48, 12, 2), 1, 4, 4, 0, 0, 4, 4, 0, 0, 0, p, None) == -1
    assert lib.ebfi_frames_u8_to_planar(p, s3, 0, 4, 4, 0, 0, 4, 4, 0, 0, 0, p, None) == 0          # n == 0: nothing to do
    assert lib.ebfi_planar_to_u8(p, s3, 1, 4, 4, None, None) == -1 and b"null" in lib.ebfi_last_error()
    assert lib.ebfi_planar_to_u8(p, s3, 1, 0, 4, p, None) == -1 and b"sizes" in lib.ebfi_last_error()
    assert lib.ebfi_planar_to_u8(p, (ctypes.c_int64 * 3)(48, -16, 4), 1, 4, 4, p, None) == -1
    assert lib.ebfi_planar_to_u8(p, s3, 0, 4, 4, p, None) == 0
