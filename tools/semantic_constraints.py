#!/usr/bin/env python
"""Semantic-constraint refinement of the exported masks of the object channel (the targets of stage 2.2); takes the flags of
the reference's tools/SemanticConstraintsAndMAA/semantic_constraints.py unchanged, plus --data_dir, --dino_ckpt, --batch-frames
and --step, e.g.

    python tools/semantic_constraints.py --pretrain_dir <exp dir> --dataset davis --object-channel $OBJECT_CHANNEL \
        --dino_ckpt dino_deitsmall8_pretrain.pth

Writes {pretrain_dir}/{export dir}_torchcrf_ncut_torchcrf/{channel}/pred_seg_*.png (rcf_amd.semantic.main) and refuses to
overwrite a file that is already there."""
import os
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

from rcf_amd import semantic  # noqa: E402


def cli(argv, **kw):
    written = semantic.main(argv, **kw)
    print(f"wrote {len(written)} masks")


if __name__ == "__main__":
    cli(sys.argv[1:])
