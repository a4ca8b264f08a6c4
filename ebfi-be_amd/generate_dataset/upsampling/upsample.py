"""The frame-upsampling step: a tree of frame sequences -> adaptively upsampled gray frames and their times.

Same path and flags as the reference's generate_dataset/upsampling/upsample.py (`--input_dir`, `--output_dir`, `--device`), plus
`--checkpoint` and `--imgs_dirname`.  Every directory under --input_dir that holds `fps.txt` and `imgs/` is one sequence; for
each, <output_dir>/<same relative path>/<imgs_dirname>/%08d.png and timestamps.txt are written (ebfi_amd.upsample).  With
`--imgs_dirname mono` the output is what generate_dataset/syn_gopro.py reads beside a sequence's `rgb/`.

--output_dir must not exist.  The Super-SloMo checkpoint (the reference's SuperSloMo.ckpt: torch.load of a dict with
state_dictFC and state_dictAT) is read from --checkpoint and never downloaded.  Video files are not read: a directory that holds
only a video is an error.
"""
import argparse
import os
import sys

PKG = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
if PKG not in sys.path:
    sys.path.insert(0, PKG)

FLAGS = (          # (name, required, default, help): the reference's three, then --checkpoint and --imgs_dirname
    ("--input_dir", True, None, "Path to input directory: sequences are directories with fps.txt and imgs/."),
    ("--output_dir", True, None, "Path to non-existing output directory. This script will generate the directory."),
    ("--device", False, "cuda:0", "Device to be used (cuda:X)"),
    ("--checkpoint", False, "./upsampling/checkpoint/SuperSloMo.ckpt", "Super-SloMo checkpoint file (never downloaded)"),
    ("--imgs_dirname", False, "imgs", "name of the directory the frames are written to (mono: what syn_gopro.py reads)"),
)


def get_flags(argv=None):
    parser = argparse.ArgumentParser(description=__doc__.split("\n")[0])
    for name, required, default, text in FLAGS:
        parser.add_argument(name, type=str, required=required, default=default, help=text)
    return parser.parse_args(argv)


def main(argv=None):
    flags = get_flags(argv)
    from ebfi_amd.upsample import Upsampler
    upsampler = Upsampler(input_dir=flags.input_dir, output_dir=flags.output_dir, device=flags.device,
                          checkpoint=flags.checkpoint, imgs_dirname=flags.imgs_dirname)
    upsampler.upsample()
    return 0


if __name__ == "__main__":
    sys.exit(main())
