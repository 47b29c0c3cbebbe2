#!/usr/bin/env python
"""CRF post-processing of exported masks (the step before evaluation); takes the flags of the reference's
tools/pydenseCRF/crf.py unchanged -- --seq may name several sequences, one process takes them all -- plus --batch-frames and
--workers, e.g.

    python tools/crf_postprocess.py --input data/data_davis/JPEGImages/480p --output output \
        --annotation-dir saved/saved_rcf_stage2.2/saved_eval_export --step 4320

Writes {annotation-dir}_crf/pred_seg_*.png (rcf_amd.postprocess.main; for a channel directory such as .../export/0 the suffix
goes to its parent: .../export_crf/0) and overwrites what is there, as the reference does."""
import os
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

from rcf_amd import postprocess  # noqa: E402


def cli(argv, **kw):
    written = postprocess.main(argv, **kw)
    print(f"wrote {len(written)} masks")


if __name__ == "__main__":
    cli(sys.argv[1:])
