#!/usr/bin/env python3
"""Fixture for the SegTrackv2 / FBMS59 evaluation (rcf_amd.stv2_fbms): the REFERENCE's own tool decides the lines.

Builds rcf_amd.synth.stv2_fbms_tree in a temporary directory and runs the reference's
tools/STv2-FBMS59-evaluation/eval_tool.py there, with that directory as the working directory (the tool reads
data/data_SegTrackv2/trainval.txt and data/data_fbms59/val_all.txt relative to it), once per dataset, in a fresh
interpreter.  Stored in stv2_fbms_eval.json: the tree's seed and step, the Pillow version that resized, and the lines the
tool printed.  A recorded result; no reference text.

Run in the build container only:  python tests/golden/make_golden_stv2_fbms.py
"""
import json
import os
import subprocess
import sys
import tempfile

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(os.path.dirname(HERE))
REF_TOOL = "/root/reference/tools/STv2-FBMS59-evaluation/eval_tool.py"
sys.path.insert(0, ROOT)

from rcf_amd import synth  # noqa: E402

SEED, STEP = 59, 3


def main():
    import PIL
    out = {"seed": SEED, "step": STEP, "pillow": PIL.__version__, "lines": {}}
    with tempfile.TemporaryDirectory() as tmp:
        _, pred_dirs = synth.stv2_fbms_tree(tmp, seed=SEED, step=STEP)
        for ds, pred_dir in pred_dirs.items():
            r = subprocess.run([sys.executable, "-W", "ignore", REF_TOOL, "--dataset", ds, "--step", str(STEP), "--pred_dir",
                                pred_dir], cwd=tmp, check=True, capture_output=True, text=True)
            out["lines"][ds] = r.stdout.splitlines()
            print(ds)
            print(r.stdout)
    with open(os.path.join(HERE, "stv2_fbms_eval.json"), "w") as f:
        json.dump(out, f, indent=1, sort_keys=True)
        f.write("\n")


if __name__ == "__main__":
    main()
