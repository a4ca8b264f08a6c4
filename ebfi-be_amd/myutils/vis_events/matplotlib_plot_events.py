"""Import-path shim: `from myutils.vis_events.matplotlib_plot_events import event_visualisation` as the reference spells it
(infer_ours.py:18, the model file's star import), on top of the native event-count image (ebfi_amd.eventvis,
csrc/eventvis.hip).

What is here: `plot_event_cnt` (myutils/vis_events/matplotlib_plot_events.py:127-251) and `plot_frame` (:74-79) with the
reference's signatures and defaults -- the two methods its inference loop calls.  plot_event_cnt returns the same H x W x 3
uint8 array as the reference's, bit for bit; the array is computed on the MI355X and there is no CPU path.  Saving: the
reference draws the array into a matplotlib figure of the array's pixel size and saves that; here the array itself is written
with PIL (like infer_ours.py's write_png), so the contract is the array, not matplotlib's resampling and encoder.

What is not: the 'gray' scheme of plot_event_cnt (in the reference it only runs with use_opencv=True and nothing calls it;
NotImplementedError here), and the class's other plotting methods -- plot_event_stack, plot_event_img, the 3-D plots, the image
grids and the animation helpers -- which need matplotlib / open3d and belong to no inference or training path.

Importing this module needs neither matplotlib, cv2 nor open3d; PIL is imported only when something is saved.
"""
import numpy as np
import torch

from ebfi_amd import eventvis

__all__ = ["event_visualisation"]


def _save(array, path):
    assert path is not None
    from PIL import Image
    Image.fromarray(array).save(path)


class event_visualisation():
    def plot_frame(self, frame, is_save, path=None, cmap='gray'):
        """frame: np.ndarray uint8, HxW or HxWx3; written as it is when is_save (cmap is kept for the signature: the
        reference's callers pass RGB frames, on which matplotlib ignores it)."""
        if is_save:
            _save(np.ascontiguousarray(frame), path)

    def plot_event_cnt(self, event_cnt, is_save, path=None, color_scheme="green_red", use_opencv=False,
                       is_black_background=True, is_norm=True):
        """event_cnt: HxWx2 (np.ndarray on the reference's path, or a tensor; 0 for positive, 1 for negative).  A GPU tensor
        is read where it lies; a host array cannot be drawn -- NotImplementedError, like every op of the package.
        Returns the HxWx3 uint8 ndarray of the reference.

        'green_red': green for positive, red for negative
        'blue_red': blue for positive, red for negative
        """
        assert color_scheme in ['green_red', 'gray', 'blue_red'], f'Not support {color_scheme}'
        if color_scheme == 'gray':
            raise NotImplementedError("plot_event_cnt: the 'gray' scheme is not built (the reference's only runs with "
                                      "use_opencv=True and nothing calls it)")
        if not torch.is_tensor(event_cnt):
            event_cnt = torch.from_numpy(np.asarray(event_cnt))
        if event_cnt.dim() != 3 or event_cnt.shape[2] != 2:
            raise ValueError("plot_event_cnt: expected HxWx2, got %r" % (tuple(event_cnt.shape),))
        ev = event_cnt.permute(2, 0, 1).unsqueeze(0)           # [1, 2, H, W] view
        if ev.is_cuda and ev.dtype != torch.float32:
            ev = ev.float()
        image = eventvis.event_count_images(ev, color_scheme=color_scheme, black_background=is_black_background,
                                            is_norm=is_norm, use_opencv=use_opencv)[0].cpu().numpy()
        if is_save:
            _save(image, path)
        return image
