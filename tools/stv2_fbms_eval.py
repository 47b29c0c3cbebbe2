#!/usr/bin/env python
"""SegTrackv2 / FBMS59 mIoU of exported pred_seg_*.png masks; takes the flags of the reference's
tools/STv2-FBMS59-evaluation/eval_tool.py, e.g.

    python tools/stv2_fbms_eval.py --dataset FBMS59 --step 0 --pred_dir <exp dir>/saved_eval_export/0

plus --data_dir (default data: the folder with data_SegTrackv2 / data_fbms59), --batch-frames (frames per device call) and
--host (Pillow on the host, no device call).  Prints the reference tool's lines (rcf_amd.stv2_fbms.main)."""
import os
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

from rcf_amd import stv2_fbms  # noqa: E402

if __name__ == "__main__":
    stv2_fbms.main(sys.argv[1:])
