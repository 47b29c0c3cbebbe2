#!/usr/bin/env python3
"""Fixtures for the DAVIS J & F evaluation (rcf_amd.davis): the REFERENCE's own tool decides the numbers.

The reference's `davis2017` package (tools/davis2016-evaluation) is imported from /root/reference and run on seeded
synthetic inputs (rcf_amd.synth.davis_inputs / davis_tree).  It needs two modules that are not installed here, so this
script registers numpy stand-ins for them before the import:
  - cv2.dilate(src, kernel): binary dilation with a 0/1 kernel, anchor at the kernel's centre, default border (pixels
    outside the image add nothing): dst(y, x) = max over kernel[i, j] != 0 of src(y + i - ay, x + j - ax);
  - skimage.morphology.disk(r): X^2 + Y^2 <= r^2 on arange(-r, r + 1), as uint8.
These stand-ins restate the libraries' documented behaviour; parity with the real cv2 and skimage is therefore not
pinned by these fixtures (the same status as rcf_amd.export's save_image stand-in).  numpy 2 dropped `np.bool`, which
the reference uses; it is aliased to `bool` when missing.

The CSV texts come from the reference's evaluation_method.py itself (run with runpy; it needs pandas, which only the
build machine has).  Stored: seeds, shapes, the per-frame J / F values (float.hex), statistics, metrics_res dicts and
the two CSV texts.  No reference text.

Run in the build container only:  python tests/golden/make_golden_davis.py
"""
import io
import json
import os
import runpy
import sys
import tempfile
import types
from contextlib import redirect_stdout

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(os.path.dirname(HERE))
REF_TOOL = "/root/reference/tools/davis2016-evaluation"
sys.path.insert(0, ROOT)

from rcf_amd import synth  # noqa: E402

# (name, seed, kind, N, H, W, bound_th, void)
CASES = [
    ("blobs_480x854", 11, "blobs", 3, 480, 854, 0.008, False),
    ("blobs_480x854_void", 12, "blobs", 2, 480, 854, 0.008, True),
    ("blobs_480x854_th0", 13, "blobs", 1, 480, 854, 0, False),
    ("blobs_480x854_th0.004", 14, "blobs", 1, 480, 854, 0.004, False),
    ("blobs_480x854_th0.05", 15, "blobs", 1, 480, 854, 0.05, False),
    ("blobs_480x854_th3px", 16, "blobs", 1, 480, 854, 3, False),
    ("blobs_100x300_th64px", 17, "blobs", 2, 100, 300, 64, False),
    ("empty_pred", 21, "empty_pred", 1, 120, 214, 0.008, False),
    ("empty_gt", 22, "empty_gt", 1, 120, 214, 0.008, False),
    ("both_empty", 23, "both_empty", 1, 120, 214, 0.008, False),
    ("all_ones", 24, "all_ones", 1, 120, 214, 0.008, False),
    ("all_ones_void", 25, "all_ones", 1, 120, 214, 0.008, True),
    ("pixels_37x61", 26, "pixels", 3, 37, 61, 0.008, False),
    ("pixels_64x128", 27, "pixels", 2, 64, 128, 2, False),
    ("lines_70x130", 28, "lines", 3, 70, 130, 0.008, False),
    ("checker_48x70", 29, "checker", 1, 48, 70, 0.008, False),
    ("checker_48x70_void", 30, "checker", 1, 48, 70, 1, True),
    ("shape_1x1", 31, "blobs", 2, 1, 1, 0.008, False),
    ("shape_1x1_ones", 32, "all_ones", 1, 1, 1, 0.008, False),
    ("shape_1x97", 33, "blobs", 2, 1, 97, 0.008, False),
    ("shape_83x1", 34, "blobs", 2, 83, 1, 0.008, False),
    ("shape_37x61", 35, "blobs", 3, 37, 61, 0.008, True),
    ("shape_481x855", 36, "blobs", 2, 481, 855, 0.008, False),
]

# db_statistics inputs: (name, seed, length, nan fraction)
STATS = [("s10", 41, 10, 0.0), ("s7_nan", 42, 7, 0.3), ("s50_nan", 43, 50, 0.2), ("s300", 44, 300, 0.0),
         ("s300_nan", 45, 300, 0.1), ("s3", 46, 3, 0.0), ("all_nan", 47, 5, 1.0)]


def stats_values(seed, n, nan_frac):
    g = np.random.Generator(np.random.PCG64(seed))
    v = g.integers(0, 1001, size=n) / 1000.0
    v[g.random(n) < nan_frac] = np.nan
    return v


def _install_standins():
    def dilate(src, kernel):
        src, k = np.asarray(src), np.asarray(kernel)
        H, W = src.shape
        kh, kw = k.shape
        ay, ax = kh // 2, kw // 2
        dst = np.zeros_like(src)
        for i in range(kh):
            for j in np.nonzero(k[i])[0]:
                dy, dx = i - ay, j - ax                       # dst(y, x) |= src(y + dy, x + dx)
                ys, yd = (slice(dy, H), slice(0, H - dy)) if dy >= 0 else (slice(0, H + dy), slice(-dy, H))
                xs, xd = (slice(dx, W), slice(0, W - dx)) if dx >= 0 else (slice(0, W + dx), slice(-dx, W))
                np.maximum(dst[yd, xd], src[ys, xs], out=dst[yd, xd])
        return dst

    def disk(radius, dtype=np.uint8):
        L = np.arange(-radius, radius + 1)
        X, Y = np.meshgrid(L, L)
        return np.array((X ** 2 + Y ** 2) <= radius ** 2, dtype=dtype)

    sys.modules["cv2"] = types.SimpleNamespace(dilate=dilate)
    sk = types.ModuleType("skimage")
    sk.morphology = types.SimpleNamespace(disk=disk)
    sys.modules["skimage"] = sk
    sys.modules["skimage.morphology"] = sk.morphology
    if not hasattr(np, "bool"):
        np.bool = bool


def _hex(x):
    return float(x).hex()


def _metrics_json(m):
    out = {}
    for k, d in m.items():
        out[k] = {"M": [_hex(v) for v in d["M"]], "R": [_hex(v) for v in d["R"]], "D": [_hex(v) for v in d["D"]],
                  "M_per_object": {s: _hex(v) for s, v in d["M_per_object"].items()},
                  "seq_len": {s: int(v) for s, v in d["seq_len"].items()}}
    return out


def main():
    _install_standins()
    sys.path.insert(0, REF_TOOL)
    from davis2017 import metrics, utils
    from davis2017.evaluation import DAVISEvaluation
    out = {"cases": [], "stats": [], "tree": {}}
    for name, seed, kind, N, H, W, th, void in CASES:
        pred, gt, vd = synth.davis_inputs(seed, N=N, H=H, W=W, kind=kind, void=void)
        J = [metrics.db_eval_iou(gt[n], pred[n], None if vd is None else vd[n]) for n in range(N)]
        F = [metrics.f_measure(pred[n], gt[n], None if vd is None else vd[n], bound_th=th) for n in range(N)]
        out["cases"].append({"name": name, "seed": seed, "kind": kind, "N": N, "H": H, "W": W, "bound_th": th,
                             "void": void, "J": [_hex(v) for v in J], "F": [_hex(v) for v in F]})
        print(f"{name:24s} J {np.round(np.array(J, float), 4)} F {np.round(np.array(F, float), 4)}")
    for name, seed, n, frac in STATS:
        M, R, D = utils.db_statistics(stats_values(seed, n, frac))
        out["stats"].append({"name": name, "seed": seed, "n": n, "nan_frac": frac, "MRD": [_hex(M), _hex(R), _hex(D)]})
    with tempfile.TemporaryDirectory() as tmp:
        davis_path, res_path = synth.davis_tree(tmp)
        with redirect_stdout(io.StringIO()):
            for task in ("unsupervised", "semi-supervised"):
                ev = DAVISEvaluation(davis_root=davis_path, task=task, gt_set="val", year="2016", step=0)
                out["tree"][task] = _metrics_json(ev.evaluate(res_path))
            argv = sys.argv
            sys.argv = ["evaluation_method.py", "--davis_path", davis_path, "--set", "val", "--task", "unsupervised",
                        "--results_path", res_path, "--year", "2016", "--step", "0"]
            try:
                runpy.run_path(os.path.join(REF_TOOL, "evaluation_method.py"), run_name="__main__")
            finally:
                sys.argv = argv
        for fn in ("global_results-val.csv", "per-sequence_results-val.csv"):
            with open(os.path.join(res_path, fn)) as f:
                out["tree"][fn] = f.read()
    print(out["tree"]["global_results-val.csv"] + out["tree"]["per-sequence_results-val.csv"])
    with open(os.path.join(HERE, "davis.json"), "w") as f:
        json.dump(out, f, indent=1, sort_keys=True)
        f.write("\n")


if __name__ == "__main__":
    main()
