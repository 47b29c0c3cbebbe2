#!/usr/bin/env python
"""ms per frame of the SegTrackv2 / FBMS59 evaluation's resize + IoU counts at 480x854 -> 360x640 and 240x427 -> 480x854 (RGB
masks, channel 0): the device kernel alone (rcf_pil_resample_u8 in its counts form, device events around repeated launches on
resident inputs), rcf_amd.pilresize.resize_iou_counts from host numpy arrays (copies and the read-back included), and
Pillow + numpy on the host as the reference tool does it.  Checks on the way that the three agree.

    python tools/time_stv2_fbms.py [--frames 16] [--reps 2000] [--out profiles/stv2_fbms_time.txt]"""
import argparse
import json
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

import numpy as np  # noqa: E402
import torch  # noqa: E402

from rcf_amd import pilresize, stv2_fbms  # noqa: E402

SHAPES = ((480, 854, 360, 640), (240, 427, 480, 854))


def inputs(N, h, w, H, W, seed):
    g = np.random.Generator(np.random.PCG64(seed))
    yy, xx = np.mgrid[:h, :w]
    frames = np.empty((N, h, w, 3), dtype=np.uint8)
    for n in range(N):                       # soft masks around the threshold, as the exported ones are
        d = np.hypot((yy - g.uniform(0.3, 0.7) * h) / (0.25 * h), (xx - g.uniform(0.3, 0.7) * w) / (0.25 * w))
        frames[n] = np.clip(89.5 + 40.0 * (1.0 - d) + g.normal(0, 2.0, size=(h, w)), 0, 255).astype(np.uint8)[..., None]
    gt = (g.integers(0, 2, size=(N, H // 8 + 1, W // 8 + 1)).repeat(8, 1).repeat(8, 2)[:, :H, :W]).astype(np.uint8)
    return frames, gt


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--frames", type=int, default=16)
    ap.add_argument("--reps", type=int, default=2000)
    ap.add_argument("--host_frames", type=int, default=8)
    ap.add_argument("--out", type=str, default=None, help="also append the result lines to this file")
    a = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("time_stv2_fbms.py measures the device: no GPU here")
    from PIL import Image
    pred_min = stv2_fbms.pred_min_for()
    lines = []
    for h, w, H, W in SHAPES:
        N = a.frames
        frames, gt = inputs(N, h, w, H, W, seed=h)
        res = {"src": [h, w], "dst": [H, W], "frames_per_call": N, "tile_rows": pilresize.tile_rows(
            h, H, pilresize.coeff_tables(h, H)[0].shape[1])}
        src, g = torch.from_numpy(frames).cuda(), torch.from_numpy(gt).cuda()
        counts = torch.zeros((N, 2), dtype=torch.int64, device="cuda")
        dst = torch.empty((N, H, W), dtype=torch.uint8, device="cuda")
        forms = (("device_kernel_counts_ms_per_frame", src, None, g, counts),
                 ("device_kernel_resize_ms_per_frame", src, dst, None, None),
                 ("device_kernel_counts_single_frame_ms", src[:1], None, g[:1], counts[:1]))
        for label, s, d, gg, cc in forms:
            call = lambda: pilresize._launch(s, (H, W), "bicubic", d, gg, pred_min, cc)
            for _ in range(5):
                call()
            torch.cuda.synchronize()
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record()
            for _ in range(a.reps):
                call()
            e1.record()
            torch.cuda.synchronize()
            res[label] = round(e0.elapsed_time(e1) / (a.reps * s.shape[0]), 5)
        dev_counts = pilresize.resize_iou_counts(frames, gt, pred_min)
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        for _ in range(3):
            pilresize.resize_iou_counts(frames, gt, pred_min)
        res["resize_iou_counts_from_numpy_ms_per_frame"] = round((time.perf_counter() - t0) * 1e3 / (3 * N), 4)
        nh = min(a.host_frames, N)
        t0 = time.perf_counter()
        host_counts = [stv2_fbms.pillow_counts(Image.fromarray(frames[n]), gt[n], pred_min) for n in range(nh)]
        res["host_pillow_numpy_ms_per_frame"] = round((time.perf_counter() - t0) * 1e3 / nh, 4)
        res["counts_agree"] = bool(np.array_equal(np.stack(host_counts), dev_counts[:nh]))
        res["device_name"] = torch.cuda.get_device_name(0)
        lines.append(json.dumps(res))
        print(lines[-1], flush=True)
    if a.out:
        with open(a.out, "a") as f:
            f.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
