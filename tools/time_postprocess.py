#!/usr/bin/env python
"""ms per 480x854 frame of the CRF post-processing (tools/pydenseCRF/crf.py's `refine`: T = 50, symmetric normalisation), 8
seeded natural-like frames per call (synth.smooth_rgb, synth.soft_blob_mask), one process, host clock around work that ends in a
device synchronise, medians and spread of repeated runs after warm-up:
 (a) offline.refine_batch: the unary in float64 numpy on the host, frame by frame, 3.3 MB of fp32 per frame uploaded, the CRF,
     the MAP copied back as fp32;
 (b) offline.refine_batch_u8 on the same bytes: 0.4 MB per frame uploaded, the unary from the table on the device
     (rcf_crf_unary_lut_u8), the CRF, the u8 result copied back;
 (c) the parts: the host unary alone, its upload alone, the device unary pass alone on resident masks (`--inner` calls per timed
     window: a call is tens of microseconds), and the CRF alone on a resident unary.
The routes alternate inside every repetition, so a drift of the clock hits all of them.  Fails without a GPU.

    python tools/time_postprocess.py [--reps 20]"""
import argparse
import json
import os
import statistics
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

import numpy as np  # noqa: E402
import torch  # noqa: E402

from rcf_amd import offline, postprocess, synth  # noqa: E402
from rcf_amd.crf import crf_soft_batched  # noqa: E402

FRAMES = 8
H, W = postprocess.IMG_SIZE


def wall_ms(fn):
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    fn()
    torch.cuda.synchronize()
    return (time.perf_counter() - t0) * 1e3


def alternate(fns, reps, warmup=3):
    """{name: [ms per call] * reps}; every repetition runs each fn once, in turn"""
    for _ in range(warmup):
        for fn in fns.values():
            fn()
    runs = {k: [] for k in fns}
    for _ in range(reps):
        for k, fn in fns.items():
            runs[k].append(wall_ms(fn))
    return runs


def summary(runs, per):
    return {k: {"median_ms_per_frame": statistics.median(v) / per[k], "min": min(v) / per[k], "max": max(v) / per[k],
                "spread_pct": 100.0 * (max(v) - min(v)) / statistics.median(v)} for k, v in runs.items()}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=20, help="repetitions of every route (at least 20)")
    ap.add_argument("--inner", type=int, default=50, help="calls of the device unary pass per timed window")
    a = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("time_postprocess.py measures the device: no GPU here")
    reps = max(20, a.reps)
    dev = "cuda:0"
    kw = postprocess.REFINE_KW
    images = np.stack([synth.smooth_rgb(H, W, 7000 + i) for i in range(FRAMES)])
    masks = np.stack([(synth.soft_blob_mask(H, W, 7000 + i) * (255, 190, 140, 230)[i % 4]).astype(np.uint8) for i in range(FRAMES)])
    a_out = offline.refine_batch(masks, images, **kw)
    b_out = offline.refine_batch_u8(masks, images, **kw).cpu().numpy()
    res = {"H": H, "W": W, "frames_per_call": FRAMES, "iters": kw["iters"], "reps": reps,
           "outputs_of_the_two_routes_equal": bool(np.array_equal((a_out * 255.).astype(np.uint8), b_out))}
    per = {"a_refine_batch_host_unary": FRAMES, "b_refine_batch_u8_device_unary": FRAMES}
    res["routes"] = summary(alternate({"a_refine_batch_host_unary": lambda: offline.refine_batch(masks, images, **kw),
                                       "b_refine_batch_u8_device_unary": lambda: offline.refine_batch_u8(masks, images, **kw).cpu()},
                                      reps), per)
    r = res["routes"]
    res["a_over_b"] = r["a_refine_batch_host_unary"]["median_ms_per_frame"] / r["b_refine_batch_u8_device_unary"]["median_ms_per_frame"]
    # (c) the parts
    m_dev, rgb_dev = torch.from_numpy(masks).to(dev), torch.from_numpy(images).to(dev)
    unary_host = torch.from_numpy(np.stack([offline._unary_from_u8(m, kw["gk"]) for m in masks]))
    unary_dev = offline.unary_from_u8_device(m_dev)
    res["unaries_bit_identical"] = bool(torch.equal(unary_dev.cpu().view(torch.int32), unary_host.view(torch.int32)))
    crf = lambda: crf_soft_batched(rgb_dev, unary_dev, W, H, 0.0, 0.0, kw["compat"], kw["sxy"], kw["srgb"], kw["iters"], symmetric=True)
    parts = {
        "host_unary_numpy_float64": lambda: np.stack([offline._unary_from_u8(m, kw["gk"]) for m in masks]),
        "upload_fp32_unary": lambda: unary_host.to(dev),
        "upload_u8_masks": lambda: torch.from_numpy(masks).to(dev),
        "device_unary_pass": lambda: [offline.unary_from_u8_device(m_dev) for _ in range(a.inner)],
        "crf_alone_symmetric": crf,
    }
    per = {k: FRAMES for k in parts}
    per["device_unary_pass"] = FRAMES * a.inner
    res["parts"] = summary(alternate(parts, reps), per)
    p = res["parts"]
    res["host_unary_plus_upload_over_crf"] = ((p["host_unary_numpy_float64"]["median_ms_per_frame"] + p["upload_fp32_unary"]["median_ms_per_frame"]) /
                                              p["crf_alone_symmetric"]["median_ms_per_frame"])
    npix = H * W
    res["device_unary_pass_bytes_per_frame"] = {"mask_read_twice": 2 * npix, "unary_written": 8 * npix}
    res["device_unary_pass_GB_per_s"] = 10 * npix / (p["device_unary_pass"]["median_ms_per_frame"] * 1e-3) / 1e9
    res["device_name"] = torch.cuda.get_device_name(0)
    print(json.dumps(res))


if __name__ == "__main__":
    main()
