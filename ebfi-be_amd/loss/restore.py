"""Drop-in for the evaluation metrics of `loss.restore` (loss/restore.py:13-92): the reference's call contract -- a 1 x C x H x W
pair in, a Python float out -- computed by ebfi_amd.metrics on the device instead of scikit-image on the host."""
from ebfi_amd.metrics import LPIPS_UNAVAILABLE, frame_metrics


class ssim_loss:
    def __init__(self, data_range=2.0):
        self.data_range = data_range           # (2.0: the reference's float32 call without data_range)

    def __call__(self, pred, tgt):
        assert pred.size() == tgt.size()
        return float(frame_metrics(_nchw(pred), _nchw(tgt), ssim_data_range=self.data_range)[1][0])


class psnr_loss:
    def __call__(self, pred, tgt):
        assert pred.size() == tgt.size()
        return float(frame_metrics(_nchw(pred), _nchw(tgt))[0][0])


class perceptual_loss:
    def __init__(self, *args, **kwargs):
        raise NotImplementedError(LPIPS_UNAVAILABLE)


def _nchw(t):
    # the reference squeezes its 1 x C x H x W input: one frame, C channels (or one plane)
    if t.dim() == 4 and t.shape[0] == 1:
        return t.float()
    if t.dim() == 3:
        return t.float().unsqueeze(0)
    if t.dim() == 2:
        return t.float()[None, None]
    raise ValueError("expected a 1 x C x H x W tensor, got %s" % (tuple(t.shape),))
