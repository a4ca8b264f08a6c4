"""The frame-upsampling step of dataset generation on the device: the Vid2E adaptive upsampler around two Super-SloMo U-Nets
(generate_dataset/upsampling/utils/{upsampler,model,dataset,utils,const}.py of the reference).

Per pair of consecutive frames (I0, I1): the flow network gives F_0_1 and F_1_0; N = ceil(max |flow|) as an int; for k in
1 .. N-1 the frame at t = k / N is synthesised by the interpolation network from the 20-channel tensor built around two
back-warps, and blended from two more.  Each pair yields I0 and its intermediates (never the last frame of a sequence), written
as gray PNGs with every frame's time in timestamps.txt -- the `mono/*` and `timestamps.txt` that generate_dataset/syn_gopro.py
reads when `--imgs_dirname mono` is given.

Where the work runs.  3x3 convolutions: the split-precision kernels on weight images packed once per network
(ebfi_conv2d_pack_bf16x3 -> ebfi_conv2d_forward_bf16x3); 7x7 and 5x5: the exact fp32 kernel (ebfi_conv2d_forward); pool,
up-sampling, flow maximum, the 20-channel assembly with its warps, and the blend with its warps, byte law and gray:
csrc/upsample.hip.  Batch is 1, so a channel slice of a [C, H, W] buffer is contiguous: a skip tensor and the convolution output
it is concatenated with are written straight into the two halves of one preallocated buffer and no concatenation runs.  The host
reads one scalar per pair (the flow maximum, which decides how many frames there are) and one block of gray bytes.

What differs from the reference: video files are refused (no skvideo here) with an error naming the directory; a missing
checkpoint is an error naming the path and is never downloaded; there is no CPU path.  The law itself is written out in
include/ebfi_hip.h and restated in float64 by tests/upsample_ref.py.
"""
import math
import os
import shutil
from pathlib import Path

import numpy as np
import torch

from . import _native as N

MEAN = (0.429, 0.431, 0.397)                  # const.py, RGB order; std is 1
FPS_FILENAME = "fps.txt"
IMGS_DIRNAME = "imgs"
TIMESTAMPS_FILENAME = "timestamps.txt"
DEFAULT_CHECKPOINT = "./upsampling/checkpoint/SuperSloMo.ckpt"      # the reference's relative path
VIDEO_FORMATS = frozenset(
    ".webm .mp4 .m4p .m4v .avi .avchd .ogg .mov .ogv .vob .f4v .mkv .svi .m2v .mpg .mp2 .mpeg .mpe .mpv .amv .wmv .flv .mts "
    ".m2ts .ts .qt .3gp .3g2 .f4p .f4a .f4b".split())
IMG_FORMATS = frozenset(".png .jpg .jpeg .bmp .pbm .pgm .ppm .pnm .webp .tiff .tif".split())

ACT_LEAKY, SLOPE = 1, 0.1
MAX_FRAMES_PER_PAIR = 4096                    # a flow maximum beyond this is a broken checkpoint, not motion


def unet_layers(in_channels, out_channels):
    """[(state-dict prefix, Cin, Cout, k)] of UNet(in, out) in execution order."""
    layers = [("conv1", in_channels, 32, 7), ("conv2", 32, 32, 7)]
    for i, (ci, co, k) in enumerate([(32, 64, 5), (64, 128, 3), (128, 256, 3), (256, 512, 3), (512, 512, 3)], 1):
        layers += [("down%d.conv1" % i, ci, co, k), ("down%d.conv2" % i, co, co, k)]
    for i, (ci, co) in enumerate([(512, 512), (512, 256), (256, 128), (128, 64), (64, 32)], 1):
        layers += [("up%d.conv1" % i, ci, co, 3), ("up%d.conv2" % i, 2 * co, co, 3)]
    return layers + [("conv3", 32, out_channels, 3)]


# ------------------------------------------------------------------------------------------------------------ the U-Net
class SloMoNet:
    """UNet(in_channels, out_channels) of Super-SloMo, forward only, batch 1.  Holds the float32 weights, the packed images of the
    3x3 layers and the activation buffers of every resolution it has run at."""

    def __init__(self, in_channels, out_channels, device):
        self.device = torch.device(device)
        if self.device.type != "cuda":
            raise NotImplementedError("SloMoNet runs on an MI355X through libebfi_hip.so only; got device %s" % (device,))
        self.in_channels, self.out_channels = int(in_channels), int(out_channels)
        self.layers = unet_layers(self.in_channels, self.out_channels)
        self._w, self._b, self._packed = {}, {}, {}
        self._buffers = {}

    def state_dict_keys(self):
        return [p + s for p, _, _, _ in self.layers for s in (".weight", ".bias")]

    def load_state_dict(self, sd):
        """sd: the reference's key names (conv1.weight, down1.conv1.weight, ...).  3x3 weights are packed here, once."""
        missing = [k for k in self.state_dict_keys() if k not in sd]
        if missing:
            raise KeyError("SloMoNet.load_state_dict: missing %s" % ", ".join(missing))
        lib = N.lib()
        with torch.cuda.device(self.device):
            st = N.stream_ptr(self.device)
            for name, ci, co, k in self.layers:
                w = sd[name + ".weight"].detach().to(self.device, torch.float32).contiguous()
                b = sd[name + ".bias"].detach().to(self.device, torch.float32).contiguous()
                if tuple(w.shape) != (co, ci, k, k) or tuple(b.shape) != (co,):
                    raise ValueError("SloMoNet.load_state_dict: %s is %r / %r, expected %r / %r"
                                     % (name, tuple(w.shape), tuple(b.shape), (co, ci, k, k), (co,)))
                self._w[name], self._b[name] = w, b
                if k == 3:
                    nbytes = int(lib.ebfi_conv2d_packed_bytes(ci, co, 3, 0))
                    img = torch.empty(nbytes, dtype=torch.uint8, device=self.device)
                    N.check(lib.ebfi_conv2d_pack_bf16x3(N.ptr(w), ci, co, 3, 0, N.ptr(img), nbytes, st), "ebfi_conv2d_pack_bf16x3")
                    self._packed[name] = (img, nbytes)
        return self

    def _conv(self, name, x, out, H, W):
        _, ci, co, k = next(l for l in self.layers if l[0] == name)
        lib, st = N.lib(), N.stream_ptr(self.device)
        if k == 3:
            img, nbytes = self._packed[name]
            rc = lib.ebfi_conv2d_forward_bf16x3(N.ptr(x), N.ptr(None), N.ptr(self._b[name]), N.ptr(out), 1, ci, H, W, co, 3, 1, 1,
                                                ACT_LEAKY, SLOPE, N.ptr(img), nbytes, st)
        else:
            rc = lib.ebfi_conv2d_forward(N.ptr(x), N.ptr(self._w[name]), N.ptr(self._b[name]), N.ptr(out), 1, ci, H, W, co, k, 1,
                                         k // 2, ACT_LEAKY, SLOPE, N.EBFI_F32, st)
        N.check(rc, "convolution %s (%d -> %d, %dx%d, map %d x %d)" % (name, ci, co, k, k, H, W))

    def _bufs(self, H, W):
        b = self._buffers.get((H, W))
        if b is None:
            new = lambda c, l: torch.empty((c, H >> l, W >> l), dtype=torch.float32, device=self.device)
            b = {"x0": new(32, 0), "out": new(self.out_channels, 0)}
            widths = [32, 64, 128, 256, 512, 512]             # channels of the encoder at level 0 .. 5
            for l in range(1, 6):
                b["pool%d" % l] = new(widths[l - 1], l)         # pooled input of down<l>
                b["mid%d" % l] = new(widths[l], l)              # down<l>.conv1
            b["bottom"] = new(512, 5)                           # down5.conv2
            for l in range(5):                                  # level l: [up-path half | skip half], then up<5-l>.conv2
                b["cat%d" % l] = new(2 * widths[l], l)
                b["up%d" % l] = new(widths[l + 1] if l < 4 else 512, l)     # the bilinear x2 of the level below
                b["dec%d" % l] = new(widths[l], l)
            self._buffers[(H, W)] = b
        return b

    @torch.no_grad()
    def forward(self, x):
        """x: float32 [Cin, H, W] on the device, H and W multiples of 32 -> [Cout, H, W], a buffer this object owns (valid until
        the next forward at that size)."""
        N.require_gpu(x)
        if x.dim() == 4 and x.shape[0] == 1:
            x = x[0]
        if x.dim() != 3 or x.shape[0] != self.in_channels or x.dtype != torch.float32:
            raise ValueError("SloMoNet.forward: expected float32 [%d, H, W], got %s %r" % (self.in_channels, x.dtype, tuple(x.shape)))
        H, W = int(x.shape[1]), int(x.shape[2])
        if H % 32 or W % 32 or H < 32 or W < 32:
            raise ValueError("SloMoNet.forward: H = %d, W = %d must be multiples of 32 (five 2x2 pools)" % (H, W))
        if not self._w:
            raise RuntimeError("SloMoNet.forward: load_state_dict first")
        x = x.contiguous()
        b = self._bufs(H, W)
        lib = N.lib()
        widths = [32, 64, 128, 256, 512, 512]
        with torch.cuda.device(self.device):
            st = N.stream_ptr(self.device)
            self._conv("conv1", x, b["x0"], H, W)
            self._conv("conv2", b["x0"], b["cat0"][32:], H, W)                  # s1, the skip of up5
            for l in range(1, 6):
                h, w, c = H >> l, W >> l, widths[l]
                src = b["cat%d" % (l - 1)][widths[l - 1]:]
                N.check(lib.ebfi_avgpool2_forward(N.ptr(src), N.ptr(b["pool%d" % l]), widths[l - 1], 2 * h, 2 * w, st),
                        "ebfi_avgpool2_forward")
                self._conv("down%d.conv1" % l, b["pool%d" % l], b["mid%d" % l], h, w)
                dst = b["cat%d" % l][c:] if l < 5 else b["bottom"]
                self._conv("down%d.conv2" % l, b["mid%d" % l], dst, h, w)
            cur = b["bottom"]
            for i in range(1, 6):
                l = 5 - i                                                       # the level up<i> writes at
                h, w, c = H >> l, W >> l, widths[l]
                N.check(lib.ebfi_bilinear_up2_forward(N.ptr(cur), N.ptr(b["up%d" % l]), int(cur.shape[0]), h // 2, w // 2, st),
                        "ebfi_bilinear_up2_forward")
                self._conv("up%d.conv1" % i, b["up%d" % l], b["cat%d" % l][:c], h, w)
                self._conv("up%d.conv2" % i, b["cat%d" % l], b["dec%d" % l], h, w)
                cur = b["dec%d" % l]
            self._conv("conv3", cur, b["out"], H, W)
        return b["out"]

    __call__ = forward


# ------------------------------------------------------------------------------------------------------------ sequences
def crop_box(w_orig, h_orig):
    """(left, upper, right, lower) of the centre crop to multiples of 32."""
    w, h = w_orig // 32 * 32, h_orig // 32 * 32
    left, upper = (w_orig - w) // 2, (h_orig - h) // 2
    return left, upper, left + w, upper + h


def is_img_file(path):
    return Path(path).suffix.lower() in IMG_FORMATS


def is_video_file(path):
    return Path(path).suffix.lower() in VIDEO_FORMATS


class ImageSequence:
    """The sorted image files of a directory at `fps`; pair idx has the times idx / fps and (idx + 1) / fps."""

    def __init__(self, imgs_dirpath, fps):
        if not os.path.isdir(imgs_dirpath):
            raise NotADirectoryError("ImageSequence: %s is not a directory" % imgs_dirpath)
        self.fps = float(fps)
        if not self.fps > 0:
            raise ValueError("ImageSequence: fps = %r must be positive" % (fps,))
        self.imgs_dirpath = imgs_dirpath
        self.file_names = sorted(f for f in os.listdir(imgs_dirpath) if is_img_file(f))
        if not self.file_names:
            raise FileNotFoundError("ImageSequence: no image file under %s" % imgs_dirpath)

    def __len__(self):
        return len(self.file_names) - 1

    def path(self, idx):
        return os.path.join(self.imgs_dirpath, self.file_names[idx])

    def times(self, idx):
        return idx / self.fps, (idx + 1) / self.fps

    @staticmethod
    def load_rgb_u8(path):
        """uint8 [h, w, 3] RGB, centre-cropped to multiples of 32."""
        from PIL import Image
        with Image.open(path) as im:
            im = im.convert("RGB")
            im = im.crop(crop_box(*im.size))
            return np.asarray(im).copy()


def sequence_or_none(dirpath):
    """The sequence a directory holds: fps.txt + imgs/ is an ImageSequence; a directory without fps.txt and without a video file
    is none.  A video (with or without fps.txt) cannot be read here and is an error naming the directory."""
    fps_file = os.path.join(dirpath, FPS_FILENAME)
    videos = sorted(f for f in os.listdir(dirpath) if is_video_file(f) and os.path.isfile(os.path.join(dirpath, f)))
    if os.path.isfile(fps_file):
        with open(fps_file) as f:
            fps = float(f.readline().strip())
        if not fps > 0:
            raise ValueError("%s: expected fps to be larger than 0, got %r" % (fps_file, fps))
        imgs_dir = os.path.join(dirpath, IMGS_DIRNAME)
        if os.path.isdir(imgs_dir):
            return ImageSequence(imgs_dir, fps)
        if not videos:
            raise FileNotFoundError("%s has %s but neither %s/ nor a video file" % (dirpath, FPS_FILENAME, IMGS_DIRNAME))
    if videos:
        raise NotImplementedError("%s holds the video %s and no %s + %s/: video files are not read here (no skvideo); extract the "
                                  "frames into %s/ and write the frame rate to %s"
                                  % (dirpath, videos[0], FPS_FILENAME, IMGS_DIRNAME, os.path.join(dirpath, IMGS_DIRNAME),
                                     os.path.join(dirpath, FPS_FILENAME)))
    return None


def find_sequences(src_dir):
    """[(directory, sequence)] in os.walk order, as the reference visits them."""
    found = []
    for dirpath, _, _ in os.walk(src_dir):
        seq = sequence_or_none(dirpath)
        if seq is not None:
            found.append((dirpath, seq))
    return found


def normalise_table():
    """float32 [3, 256]: byte v of channel c -> float32(v / 255) - mean[c], each step rounded in float32 (ToTensor, Normalize)."""
    v = np.arange(256, dtype=np.float32) / np.float32(255)
    return np.stack([v - np.float32(m) for m in MEAN]).astype(np.float32)


def timestamps_text(timestamps):
    return "".join(str(t) + "\n" for t in timestamps)


def frame_count(flow_max):
    """N of a pair from the maximum flow magnitude: ceil as an int."""
    if not math.isfinite(flow_max):
        raise ValueError("the flow network returned a non-finite flow (maximum magnitude %r)" % (flow_max,))
    n = int(math.ceil(flow_max))
    if n > MAX_FRAMES_PER_PAIR:
        raise ValueError("maximum flow magnitude %g asks for %d frames between two inputs (limit %d): wrong checkpoint?"
                         % (flow_max, n, MAX_FRAMES_PER_PAIR))
    return n


def pair_timestamps(t0, t1, n):
    """Times of I0 and of the n - 1 intermediates, as the reference forms them (Python doubles)."""
    return [t0] + [t0 + (float(k) / n) * (t1 - t0) for k in range(1, n)]


def load_checkpoint(path):
    """The reference's file: torch.load of {'state_dictFC': ..., 'state_dictAT': ...}.  Never downloaded."""
    if not os.path.isfile(path):
        raise FileNotFoundError("Super-SloMo checkpoint %s does not exist (it is not downloaded: put the file there or pass "
                                "--checkpoint)" % os.path.abspath(path))
    ckpt = torch.load(path, map_location="cpu")
    for key in ("state_dictFC", "state_dictAT"):
        if key not in ckpt:
            raise KeyError("%s: no %r in the checkpoint" % (path, key))
    return ckpt


# ------------------------------------------------------------------------------------------------------------ the upsampler
class Upsampler:
    """Same contract as the reference's: Upsampler(input_dir, output_dir, device).upsample() walks input_dir and writes, per
    sequence, <output_dir>/<relative path>/<imgs_dirname>/%08d.png and timestamps.txt."""

    _timestamps_filename = TIMESTAMPS_FILENAME

    def __init__(self, input_dir, output_dir, device="cuda:0", checkpoint=DEFAULT_CHECKPOINT, imgs_dirname=IMGS_DIRNAME):
        if not os.path.isdir(input_dir):
            raise NotADirectoryError("The input directory must exist: %s" % input_dir)
        if os.path.exists(output_dir):
            raise FileExistsError("The output directory must not exist: %s" % output_dir)
        ckpt = load_checkpoint(checkpoint)
        self.device = torch.device(device)
        if self.device.type != "cuda" or not torch.cuda.is_available():
            raise NotImplementedError("upsampling runs on an MI355X through libebfi_hip.so only; device %s is not one (there is no "
                                      "CPU path)" % (device,))
        self.src_dir, self.dest_dir, self.imgs_dirname = input_dir, output_dir, imgs_dirname
        self._load_nets(ckpt["state_dictFC"], ckpt["state_dictAT"])
        self._prepare_output_dir(input_dir, output_dir)

    @classmethod
    def from_state_dicts(cls, device, state_dict_fc, state_dict_at):
        """The device side alone (normalise, upsample_pair), without directories or a checkpoint file."""
        self = object.__new__(cls)
        self.device = torch.device(device)
        self.src_dir = self.dest_dir = None
        self.imgs_dirname = IMGS_DIRNAME
        self._load_nets(state_dict_fc, state_dict_at)
        return self

    def _load_nets(self, state_dict_fc, state_dict_at):
        self.flowComp = SloMoNet(6, 4, self.device).load_state_dict(state_dict_fc)
        self.ArbTimeFlowIntrp = SloMoNet(20, 5, self.device).load_state_dict(state_dict_at)
        self.mean = torch.tensor(MEAN, dtype=torch.float32, device=self.device).view(3, 1, 1)
        self.table = torch.from_numpy(normalise_table()).to(self.device)
        self._pair_bufs = {}

    @staticmethod
    def _prepare_output_dir(src_dir, dest_dir):
        shutil.copytree(src_dir, dest_dir, ignore=lambda d, files: [f for f in files if os.path.isfile(os.path.join(d, f))])

    def upsample(self):
        for count, (src_dir, sequence) in enumerate(find_sequences(self.src_dir), 1):
            print("Processing sequence number {}".format(count))
            rel = os.path.relpath(src_dir, self.src_dir)
            self.upsample_sequence(sequence, os.path.join(self.dest_dir, rel, self.imgs_dirname),
                                   os.path.join(self.dest_dir, rel, self._timestamps_filename))

    def do_upsample(self, imgs_dir, fps=25):
        sequence = ImageSequence(imgs_dir, fps)
        rel = os.path.relpath(imgs_dir, self.src_dir)
        dest_imgs_dir = os.path.join(self.dest_dir, rel, self.imgs_dirname)
        dest_timestamps = os.path.join(self.dest_dir, rel, self._timestamps_filename)
        self.upsample_sequence(sequence, dest_imgs_dir, dest_timestamps)
        return dest_imgs_dir, dest_timestamps

    # -- device side of one pair
    def normalise(self, rgb_u8, out=None):
        """uint8 [h, w, 3] RGB (host, cropped) -> float32 [3, h, w] on the device, staged through pinned memory.  The values
        float32(v / 255) - mean come from a 256-entry table per channel made on the host (normalise_table): a device division
        by a constant may be a multiplication by its reciprocal, which is not the same float."""
        stage = torch.empty(rgb_u8.shape, dtype=torch.uint8, pin_memory=True)
        stage.numpy()[...] = rgb_u8
        idx = stage.to(self.device, non_blocking=True).permute(2, 0, 1).to(torch.int64)
        x = torch.gather(self.table, 1, idx.reshape(3, -1)).view(idx.shape)
        if out is None:
            return x.contiguous()
        out.copy_(x)
        return out

    def _bufs(self, H, W):
        b = self._pair_bufs.get((H, W))
        if b is None:
            dev = self.device
            b = {"x6": torch.empty((6, H, W), dtype=torch.float32, device=dev),
                 "x20": torch.empty((20, H, W), dtype=torch.float32, device=dev),
                 "max": torch.empty(1, dtype=torch.float32, device=dev)}
            self._pair_bufs[(H, W)] = b
        return b

    @torch.no_grad()
    def upsample_pair(self, I0, I1, t0, t1, want_float=False):
        """I0, I1: normalised float32 [3, H, W] on the device.  -> (N, timestamps, gray uint8 [max(N, 1), H, W] on the device:
        I0 and the intermediates, float frames [max(N, 1), 3, H, W] (`+ mean`, before the byte law) or None)."""
        H, W = int(I0.shape[1]), int(I0.shape[2])
        b = self._bufs(H, W)
        lib = N.lib()
        with torch.cuda.device(self.device):
            st = N.stream_ptr(self.device)
            x6 = b["x6"]
            if I0.data_ptr() != x6[:3].data_ptr():
                x6[:3].copy_(I0)
            if I1.data_ptr() != x6[3:].data_ptr():
                x6[3:].copy_(I1)
            I0, I1 = x6[:3], x6[3:]
            flow = self.flowComp(x6)
            N.check(lib.ebfi_flow_max_magnitude(N.ptr(flow), H, W, N.ptr(b["max"]), st), "ebfi_flow_max_magnitude")
            n = frame_count(float(b["max"].item()))          # the one synchronisation of the pair: it sizes everything below
            count = max(n, 1)
            gray = torch.empty((count, H, W), dtype=torch.uint8, device=self.device)
            frames = torch.empty((count, 3, H, W), dtype=torch.float32, device=self.device) if want_float else None
            N.check(lib.ebfi_slomo_frame_u8(N.ptr(I0), N.ptr(gray[0]), H, W, st), "ebfi_slomo_frame_u8")
            if want_float:
                frames[0] = I0 + self.mean
            for k in range(1, n):
                t = float(k) / n
                N.check(lib.ebfi_slomo_assemble(N.ptr(I0), N.ptr(I1), N.ptr(flow), t, N.ptr(b["x20"]), H, W, st), "ebfi_slomo_assemble")
                intrp = self.ArbTimeFlowIntrp(b["x20"])
                N.check(lib.ebfi_slomo_blend(N.ptr(intrp), N.ptr(b["x20"]), t, N.ptr(frames[k] if want_float else None),
                                             N.ptr(gray[k]), H, W, st), "ebfi_slomo_blend")
        return n, pair_timestamps(t0, t1, n), gray, frames

    def upsample_sequence(self, sequence, dest_imgs_dir, dest_timestamps_filepath):
        from PIL import Image
        os.makedirs(dest_imgs_dir, exist_ok=True)
        timestamps_list = []
        idx = 0
        nxt = None
        for pair in range(len(sequence)):
            first = sequence.load_rgb_u8(sequence.path(pair)) if nxt is None else nxt
            nxt = sequence.load_rgb_u8(sequence.path(pair + 1))
            if nxt.shape != first.shape:
                raise ValueError("%s: frame of shape %r in a sequence of %r" % (sequence.path(pair + 1), nxt.shape, first.shape))
            H, W = first.shape[:2]
            if H < 32 or W < 32:
                raise ValueError("%s: %d x %d pixels; frames need at least 32 x 32" % (sequence.path(pair), W, H))
            x6 = self._bufs(H, W)["x6"]
            if pair == 0:
                self.normalise(first, x6[:3])
            else:
                x6[:3].copy_(x6[3:])
            self.normalise(nxt, x6[3:])
            t0, t1 = sequence.times(pair)
            _, timestamps, gray, _ = self.upsample_pair(x6[:3], x6[3:], t0, t1)
            host = torch.empty(gray.shape, dtype=torch.uint8, pin_memory=True)
            host.copy_(gray)
            timestamps_list += timestamps
            for frame in host.numpy():
                Image.fromarray(frame).save(os.path.join(dest_imgs_dir, "%08d.png" % idx))
                idx += 1
        with open(dest_timestamps_filepath, "w") as f:
            f.write(timestamps_text(timestamps_list))
