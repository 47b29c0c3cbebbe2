#!/usr/bin/env python
"""Motion-appearance alignment of the exported mask channels; takes the flags of the reference's
tools/SemanticConstraintsAndMAA/maa.py unchanged, plus --data_dir, --dino_ckpt and --batch-frames, e.g.

    python tools/maa.py --pretrain_dir <exp dir> --dataset davis --num-channels 4 --dino_ckpt dino_deitsmall8_pretrain.pth
    OBJECT_CHANNEL=$?

Prints the frame MAA of every channel (rcf_amd.maa.main).  When more than one channel was evaluated the best channel
is the exit code, as in the reference; with --object-channel the script ends normally."""
import os
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

from rcf_amd import maa  # noqa: E402


def cli(argv, **kw):
    _, best = maa.main(argv, **kw)
    if best is not None:
        sys.exit(best)


if __name__ == "__main__":
    cli(sys.argv[1:])
