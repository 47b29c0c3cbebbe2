#!/usr/bin/env python
"""ms per 480x854 frame of the DAVIS boundary / region counts: the device kernel (rcf_davis_counts_u8, device events
around repeated launches on resident u8 masks), rcf_amd.davis.boundary_counts from host numpy masks (copies included),
and the plain numpy restatement of davis2017/metrics.py on the host (tests/test_davis_gpu.py numpy_counts).

    python tools/time_davis.py [--frames 100] [--reps 20] [--bound_th 0.008]"""
import argparse
import json
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))

import numpy as np  # noqa: E402
import torch  # noqa: E402

from rcf_amd import _lib, davis, synth  # noqa: E402
from rcf_amd.ops import _p, _stream  # noqa: E402
from test_davis_gpu import numpy_counts  # noqa: E402


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--frames", type=int, default=100)
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--bound_th", type=float, default=0.008)
    ap.add_argument("--host_frames", type=int, default=3)
    a = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("time_davis.py measures the device: no GPU here")
    N, H, W = a.frames, 480, 854
    r = davis.radius_for(H, W, a.bound_th)
    pred, gt, vd = synth.davis_inputs(5, N=N, H=H, W=W, kind="blobs")
    p, g = torch.from_numpy(pred).cuda(), torch.from_numpy(gt).cuda()
    counts = torch.zeros((N, 6), dtype=torch.int64, device="cuda")
    res = {"H": H, "W": W, "radius": r, "frames_per_call": N}
    for label, n in (("device_kernel_ms_per_frame_batch", N), ("device_kernel_ms_per_frame_single", 1)):
        call = lambda: _lib.call("rcf_davis_counts_u8", _p(p), _p(g), None, n, H, W, r, _p(counts), _stream())
        for _ in range(5):
            call()
        torch.cuda.synchronize()
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        for _ in range(a.reps):
            call()
        e1.record()
        torch.cuda.synchronize()
        res[label] = e0.elapsed_time(e1) / (a.reps * n)
    davis.boundary_counts(pred, gt)
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    for _ in range(3):
        davis.boundary_counts(pred, gt)
    res["boundary_counts_from_numpy_ms_per_frame"] = (time.perf_counter() - t0) * 1e3 / (3 * N)
    t0 = time.perf_counter()
    for n in range(a.host_frames):
        numpy_counts(pred[n], gt[n], None, r)
    res["host_numpy_ms_per_frame"] = (time.perf_counter() - t0) * 1e3 / a.host_frames
    res["device_name"] = torch.cuda.get_device_name(0)
    print(json.dumps(res))


if __name__ == "__main__":
    main()
