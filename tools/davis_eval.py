#!/usr/bin/env python
"""DAVIS J & F evaluation of exported pred_seg_*.png masks; takes the flags of the reference's
tools/davis2016-evaluation/evaluation_method.py unchanged, e.g.

    python tools/davis_eval.py --task unsupervised --year 2016 --step 0 --davis_path data/DAVIS \
        --results_path <exp dir>/saved_eval_export

Writes global_results-{set}.csv and per-sequence_results-{set}.csv into --results_path (rcf_amd.davis.main)."""
import os
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

from rcf_amd import davis  # noqa: E402

if __name__ == "__main__":
    davis.main(sys.argv[1:])
