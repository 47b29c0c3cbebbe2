#!/usr/bin/env python
"""Evaluation and `pred_seg_*.png` export of a checkpoint: the reference's `main.py CONFIG --test`, e.g.

    python tools/export_masks.py configs/rcf/rcf_export_trainval_ema.yaml --test --test-override-pretrained CKPT \
        --opts checkpoints_dir ... object_channel N
    python tools/export_masks.py configs/rcf/rcf_eval.yaml --test --test-override-pretrained CKPT --test-override-object-channel N

plus --batch-size, --workers (decode and writer threads, at most 16) and --sync (write inline).  One process, one GPU; prints the
reference's mIoU lines (rcf_amd.export_driver)."""
import os
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

from rcf_amd import export_driver  # noqa: E402

if __name__ == "__main__":
    export_driver.main(sys.argv[1:])
