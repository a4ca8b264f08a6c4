"""Drop-in for the evaluation metrics of `loss.restore` (loss/restore.py:13-92): the reference's call contract -- a 1 x C x H x W
pair in, a Python float out -- computed by ebfi_amd.metrics on the device instead of scikit-image on the host.  CharbonnierLoss (loss/restore.py:95-105, the
validation score of the trainer) is the device implementation of ebfi_amd.loss."""
import torch

from ebfi_amd.loss import CharbonnierLoss  # noqa: F401
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
    """LPIPS (v0.1) on the device, from the two weight files named here: lin_path, the reference's
    loss/PerceptualSimilarity/models/weights/v0.1/alex.pth, and backbone_path, torchvision's AlexNet state dict
    (alexnet-owt-7be5be79.pth); with net='vgg', v0.1/vgg.pth and torchvision's VGG-16 state dict (vgg16-397923af.pth).
    Without them it raises: no weight cache is searched.  net='squeeze' is refused.
    With net='vgg', grad mode on and a pred that requires grad, the call is a training loss: the value goes through
    VggLPIPS.loss and differentiates into pred (the per-channel average of other channel counts too).  net='alex' -- the
    reference's default, and what its trainer builds -- does the same when the object was made with train=True, which loads
    AlexLPIPSLoss (the data-gradient weights are packed only then); without it net='alex' is a score, with or without grad mode."""

    def __init__(self, weight=1.0, net='alex', use_gpu=True, gpu_ids=[0], lin_path=None, backbone_path=None, train=False):
        if lin_path is None or backbone_path is None:
            raise NotImplementedError(LPIPS_UNAVAILABLE)
        from ebfi_amd.lpips import load_lpips
        extra = {"train": True} if train else {}
        self.model = load_lpips(net, lin_path, backbone_path, device="cuda:%d" % gpu_ids[0], **extra)
        self.weight = weight
        self.train_alex = net == 'alex' and bool(train)

    def __call__(self, pred, target, normalize=True):
        """pred, target: N x C x H x W; C == 1 and C == 3 in one call, any other C as the mean of per-channel calls, each channel
        read as three (the reference's loop).  Returns weight * mean over N, a 0-dim device tensor."""
        assert pred.size() == target.size()
        c = pred.shape[1]
        model = self.model
        if (getattr(model, "NET", None) == "vgg" or self.train_alex) and torch.is_grad_enabled() and pred.requires_grad:
            model = model.loss                  # the training loss: the same value with a graph into pred
        if c in (1, 3):
            dist = model(pred, target, normalize=normalize)
        else:
            dist = sum(model(pred[:, i:i + 1], target[:, i:i + 1], normalize=normalize) for i in range(c)) / c
        return self.weight * dist.mean()


def _nchw(t):
    # the reference squeezes its 1 x C x H x W input: one frame, C channels (or one plane)
    if t.dim() == 4 and t.shape[0] == 1:
        return t.float()
    if t.dim() == 3:
        return t.float().unsqueeze(0)
    if t.dim() == 2:
        return t.float()[None, None]
    raise ValueError("expected a 1 x C x H x W tensor, got %s" % (tuple(t.shape),))
