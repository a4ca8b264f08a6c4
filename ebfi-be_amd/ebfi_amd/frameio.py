"""The two ends of an inference run on recorded clips, on the device (csrc/frameio.hip).

``frames_to_planar``: stored frames, interleaved uint8 [n, H0, W0, 3] -> float32 [n, 3, h, w], bit-identical to
``torch.from_numpy(frames).permute(0, 3, 1, 2).float() / 255`` on the CPU (dataloader/h5dataset_realdata.py:189), with the
dataset's crop window, the two flips and -- for clips stored BGR -- the channel reversal folded into the one read: a frame
crosses the bus at one byte per sample.

``planar_to_u8``: float32 [n, 3, H, W] -> interleaved uint8 [n, H, W, 3], bit-identical to
``(x.clamp(0, 1) * 255).cpu().numpy().transpose(0, 2, 3, 1).astype('uint8')`` (infer_ours.py:135) for every input that is not
NaN; NaN gives 0, where numpy's cast is undefined.  A load's restored frames come back at one byte per sample, already in the
layout an image writer takes.

``period_to_planar``: the training reader's form of the first (ClipDataset(frames="device")): the n stored frames of a period
-> (sharp [n, 3, h, w], blur [3, h, w]) in one pass, sharp as ``frames_to_planar`` writes it and blur bit-identical to
``torch.from_numpy(frames[:e].mean(0)).permute(2, 0, 1).float() / 255`` (dataloader/h5dataset.py:311).

Inputs must be GPU tensors; there is no CPU path.
"""
import ctypes

import torch

from . import _native as N


def _i64x3(vals):
    return (ctypes.c_int64 * 3)(*[int(v) for v in vals])


@torch.no_grad()
def frames_to_planar(frames, window=None, reverse_channels=False, flip_h=False, flip_v=False):
    """frames: uint8 [n, H0, W0, 3] on the GPU, any strides with adjacent channels (a view with a storage offset is read in
    place).  window: (i, j, h, w) of the frame to read -- `crop_window`'s tuple -- or None for the whole frame."""
    N.require_gpu(frames)
    if frames.dtype != torch.uint8 or frames.dim() != 4 or frames.shape[-1] != 3:
        raise ValueError("frames_to_planar: expected uint8 [n, H, W, 3], got %s %r" % (frames.dtype, tuple(frames.shape)))
    if frames.stride(3) != 1:
        frames = frames.contiguous()
    n, H0, W0 = (int(v) for v in frames.shape[:3])
    i, j, h, w = (0, 0, H0, W0) if window is None else (int(v) for v in window)
    out = torch.empty((n, 3, max(h, 0), max(w, 0)), dtype=torch.float32, device=frames.device)
    with torch.cuda.device_of(frames):
        rc = N.lib().ebfi_frames_u8_to_planar(N.ptr(frames), _i64x3(frames.stride()[:3]), n, H0, W0, i, j, h, w,
                                              int(bool(reverse_channels)), int(bool(flip_h)), int(bool(flip_v)), N.ptr(out),
                                              N.stream_ptr(frames.device))
    N.check(rc, "ebfi_frames_u8_to_planar")
    return out


def _planar_out(name, out, shape, device):
    if out is None:
        return torch.empty(shape, dtype=torch.float32, device=device)
    if out.dtype != torch.float32 or tuple(out.shape) != tuple(shape) or not out.is_contiguous() or out.device != device:
        raise ValueError("period_to_planar: %s must be a contiguous float32 tensor of shape %r on %s" % (name, tuple(shape), device))
    return out


@torch.no_grad()
def period_to_planar(frames, num_blur, window=None, reverse_channels=False, flip_h=False, flip_v=False, sharp_out=None,
                     blur_out=None):
    """frames: the n stored frames of one period, uint8 [n, H0, W0, 3] on the GPU, as `frames_to_planar` takes them.  Returns
    (sharp float32 [n, 3, h, w], blur float32 [3, h, w]): sharp is `frames_to_planar` of the same arguments, blur the mean of
    the first `num_blur` frames.  sharp_out / blur_out: contiguous destinations to fill (slices of a batch tensor), allocated
    otherwise."""
    N.require_gpu(frames, sharp_out, blur_out)
    if frames.dtype != torch.uint8 or frames.dim() != 4 or frames.shape[-1] != 3:
        raise ValueError("period_to_planar: expected uint8 [n, H, W, 3], got %s %r" % (frames.dtype, tuple(frames.shape)))
    if frames.stride(3) != 1:
        frames = frames.contiguous()
    n, H0, W0 = (int(v) for v in frames.shape[:3])
    i, j, h, w = (0, 0, H0, W0) if window is None else (int(v) for v in window)
    sharp = _planar_out("sharp_out", sharp_out, (n, 3, max(h, 0), max(w, 0)), frames.device)
    blur = _planar_out("blur_out", blur_out, (3, max(h, 0), max(w, 0)), frames.device)
    with torch.cuda.device_of(frames):
        rc = N.lib().ebfi_period_frames_u8(N.ptr(frames), _i64x3(frames.stride()[:3]), n, int(num_blur), H0, W0, i, j, h, w,
                                           int(bool(reverse_channels)), int(bool(flip_h)), int(bool(flip_v)), N.ptr(sharp),
                                           N.ptr(blur), N.stream_ptr(frames.device))
    N.check(rc, "ebfi_period_frames_u8")
    return sharp, blur


@torch.no_grad()
def planar_to_u8(x, out=None):
    """x: float32 [n, 3, H, W] on the GPU, any strides with adjacent columns.  out: a contiguous uint8 [n, H, W, 3] tensor to
    fill (a serving loop hands the same buffer in for every load); allocated otherwise."""
    N.require_gpu(x, out)
    if x.dtype != torch.float32 or x.dim() != 4 or x.shape[1] != 3:
        raise ValueError("planar_to_u8: expected float32 [n, 3, H, W], got %s %r" % (x.dtype, tuple(x.shape)))
    if x.stride(3) != 1:
        x = x.contiguous()
    n, _, H, W = (int(v) for v in x.shape)
    if out is None:
        out = torch.empty((n, H, W, 3), dtype=torch.uint8, device=x.device)
    elif out.dtype != torch.uint8 or tuple(out.shape) != (n, H, W, 3) or not out.is_contiguous() or out.device != x.device:
        raise ValueError("planar_to_u8: out must be a contiguous uint8 tensor of shape %r on %s" % ((n, H, W, 3), x.device))
    with torch.cuda.device_of(x):
        rc = N.lib().ebfi_planar_to_u8(N.ptr(x), _i64x3(x.stride()[:3]), n, H, W, N.ptr(out), N.stream_ptr(x.device))
    N.check(rc, "ebfi_planar_to_u8")
    return out
