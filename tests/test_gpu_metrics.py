"""ebfi_image_metrics on the MI355X (ebfi_amd.metrics.frame_metrics) against the float64 restatement of test_metrics_host:
shapes from a single interior pixel to 720p, one and three channels, strided views, the narrow (unaligned) load path, the SSIM
data range, non-finite frames and bit-reproducibility."""
import numpy as np
import pytest
import torch

from test_metrics_host import ref_metrics

pytestmark = pytest.mark.gpu


def _pair(N, C, H, W, seed, wide=False):
    g = torch.Generator().manual_seed(seed)
    target = torch.rand(N, C, H, W, generator=g)
    pred = (target + 0.08 * torch.randn(N, C, H, W, generator=g)).clamp(0, 1)
    if wide:                                               # pred beyond [0, 1], as an unclipped network output is
        pred = torch.rand(N, C, H, W, generator=g) * 1.5 - 0.2
    return pred, target


def _check(got, pred, target, data_range=2.0):
    want = ref_metrics(pred.cpu().numpy(), target.cpu().numpy(), data_range)
    psnr, ssim, mse = (t.cpu().double().numpy() for t in got)
    assert np.abs(psnr - want[0]).max() <= 1e-3, (psnr, want[0])
    assert np.abs(ssim - want[1]).max() <= 1e-4, (ssim, want[1])
    assert (np.abs(mse - want[2]) / want[2]).max() <= 1e-5, (mse, want[2])


@pytest.mark.parametrize("H,W", [(7, 7), (24, 32), (37, 53), (256, 256)])
@pytest.mark.parametrize("N", [1, 5, 16])
@pytest.mark.parametrize("C", [3, 1])
def test_kernel_vs_restatement(H, W, N, C):
    from ebfi_amd.metrics import frame_metrics
    if H == 256 and N == 16 and C == 1:
        N = 5                                              # (keeps the host restatement quick; N = 16 is covered at C = 3)
    pred, target = _pair(N, C, H, W, seed=H * 1000 + W + N + C)
    _check(frame_metrics(pred.cuda(), target.cuda()), pred, target)


@pytest.mark.parametrize("C", [3, 1])
def test_wide_prediction_range(C):
    from ebfi_amd.metrics import frame_metrics
    pred, target = _pair(5, C, 37, 53, seed=7, wide=True)
    _check(frame_metrics(pred.cuda(), target.cuda()), pred, target)


def test_720p_frames():
    from ebfi_amd.metrics import frame_metrics
    pred, target = _pair(4, 3, 720, 1280, seed=9)
    _check(frame_metrics(pred.cuda(), target.cuda()), pred, target)


def test_strided_views_without_copies():
    from ebfi_amd.metrics import frame_metrics
    g = torch.Generator().manual_seed(5)
    seq = torch.rand(2, 5, 3, 40, 72, generator=g)        # [B, T, 3, H, W], the inference output layout
    sharp = torch.rand(2, 5, 3, 40, 72, generator=g)
    pred, target = seq.cuda()[1], sharp.cuda()[1]          # a slice of the batch: storage offset, contiguous frames
    assert pred.storage_offset() > 0
    _check(frame_metrics(pred, target), seq[1], sharp[1])
    wide = torch.rand(5, 6, 40, 72, generator=g)           # channel stride 2 H W
    p2, t2 = wide.cuda()[:, ::2], wide.cuda()[:, 1::2]
    assert not p2.is_contiguous()
    _check(frame_metrics(p2, t2), wide[:, ::2], wide[:, 1::2])


def test_unaligned_rows_take_the_narrow_path():
    from ebfi_amd.metrics import frame_metrics
    pred, target = _pair(3, 3, 33, 70, seed=13)
    ref = frame_metrics(pred.cuda(), target.cuda())
    buf_p = torch.zeros(pred.numel() + 1, device="cuda")
    buf_t = torch.zeros(pred.numel() + 1, device="cuda")
    buf_p[1:] = pred.cuda().flatten()
    buf_t[1:] = target.cuda().flatten()
    p1, t1 = buf_p[1:].view(pred.shape), buf_t[1:].view(pred.shape)    # row pointers 4 bytes past 16-byte alignment
    assert p1.data_ptr() % 16 == 4
    got = frame_metrics(p1, t1)
    _check(got, pred, target)
    for a, b in zip(got, ref):
        assert torch.allclose(a, b, rtol=1e-6, atol=0), (a, b)
    # a row stride that is not a multiple of 4 floats: narrow path too
    padded = torch.zeros(3, 3, 33, 71, device="cuda")
    padded[..., :70] = pred.cuda()
    _check(frame_metrics(padded[..., :70], target.cuda()), pred, target)


def test_ssim_data_range_one():
    from ebfi_amd.metrics import frame_metrics
    pred, target = _pair(5, 3, 24, 32, seed=17)
    got = frame_metrics(pred.cuda(), target.cuda(), ssim_data_range=1.0)
    _check(got, pred, target, data_range=1.0)
    assert not torch.allclose(got[1], frame_metrics(pred.cuda(), target.cuda())[1])


def test_nan_frame_only():
    from ebfi_amd.metrics import frame_metrics
    pred, target = _pair(4, 3, 30, 40, seed=19)
    clean = frame_metrics(pred.cuda(), target.cuda())
    bad = pred.clone()
    bad[2, 1, 10, 33] = float("nan")
    got = frame_metrics(bad.cuda(), target.cuda())
    keep = [0, 1, 3]
    for a, b in zip(got, clean):
        assert torch.isnan(a[2])
        assert torch.equal(a[keep], b[keep])
    tgt = target.clone()
    tgt[0, 0, 0, 0] = float("nan")                          # in the target, at the corner (outside every SSIM window's centre)
    got = frame_metrics(pred.cuda(), tgt.cuda())
    for a, b in zip(got, clean):
        assert torch.isnan(a[0]) and torch.equal(a[1:], b[1:])


def test_identical_images_give_infinite_psnr():
    from ebfi_amd.metrics import frame_metrics
    _, target = _pair(2, 3, 20, 20, seed=23)
    psnr, ssim, mse = frame_metrics(target.cuda(), target.cuda())
    assert torch.all(torch.isposinf(psnr)) and torch.all(mse == 0)
    assert torch.allclose(ssim, torch.ones_like(ssim), atol=1e-6)


def test_bit_reproducible():
    from ebfi_amd.metrics import frame_metrics
    pred, target = _pair(16, 3, 256, 256, seed=29)
    pred, target = pred.cuda(), target.cuda()
    a = frame_metrics(pred, target)
    b = frame_metrics(pred, target)
    for x, y in zip(a, b):
        assert torch.equal(x, y)


def test_reference_call_contract():
    """loss.psnr_loss / ssim_loss: a 1 x C x H x W pair in, a Python float out, as loss/restore.py:43-92."""
    from loss import psnr_loss, ssim_loss
    pred, target = _pair(1, 3, 24, 32, seed=31)
    want = ref_metrics(pred.numpy(), target.numpy())
    p = psnr_loss()(pred.cuda(), target.cuda())
    s = ssim_loss()(pred.cuda(), target.cuda())
    assert isinstance(p, float) and isinstance(s, float)
    assert abs(p - want[0][0]) <= 1e-3 and abs(s - want[1][0]) <= 1e-4
