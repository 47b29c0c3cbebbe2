#!/usr/bin/env python
"""ms per 480x856 frame of the MAA channel scoring (n = 6420 tokens, M channels), one process, device events after warm-up:
 (a) the per-channel route: NCutEvalHead.forward once per channel (a ViT forward, a Gram, a threshold and a mat-vec each);
 (b) NCutEvalHead.forward_multi at 1 and 4 frames per call (one ViT forward and one Gram per frame, all channels in one pass);
 (c) the new kernel alone (rcf_ncut_values_f32 on a resident raw Gram) against the work it replaces on the same Gram: one
     rcf_affinity_threshold_f32 + M rcf_ncut_value_grad_f32;
 (d) the new kernel's bytes / time (the Gram once + the masks) beside the chip's measured copy rate.

    python tools/time_maa.py [--channels 4] [--reps 20]"""
import argparse
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

import torch  # noqa: E402

from rcf_amd import _lib, ncut, ops, synth, vit  # noqa: E402
from rcf_amd.ops import _p, _stream  # noqa: E402

COPY_RATE_TBS = 6.29            # the chip's measured copy rate (tools/hbm_ceiling.py)


def timed(fn, reps, warmup=3):
    for _ in range(warmup):
        fn()
    torch.cuda.synchronize()
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    for _ in range(reps):
        fn()
    e1.record()
    torch.cuda.synchronize()
    return e0.elapsed_time(e1) / reps


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--channels", type=int, default=4)
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--kernel_reps", type=int, default=100)
    a = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("time_maa.py measures the device: no GPU here")
    dev, M, H, W = "cuda", a.channels, 480, 854
    m = vit.vit_small(patch_size=8)
    shapes = {k: tuple(v.shape) for k, v in m.state_dict().items()}
    m.load_state_dict({k: torch.from_numpy(v) for k, v in synth.fill_vit_state_dict(shapes, seed=21).items()})
    head = ncut.NCutEvalHead(args=None, model=m).to(dev).eval()
    g = torch.Generator().manual_seed(3)
    imgs = torch.rand(4, H, W, 3, generator=g).to(dev)
    masks = torch.rand(4, M, H, W, generator=g).to(dev)
    res = {"H": H, "W": 856, "tokens": 6420, "channels": M}
    # (a) / (b): end to end, per frame
    res["a_per_channel_route_ms_per_frame"] = timed(lambda: [head(imgs[:1], masks[:1, c], standardize=True) for c in range(M)], a.reps)
    res["b_forward_multi_ms_per_frame_batch1"] = timed(lambda: head.forward_multi(imgs[:1], masks[:1], standardize=True), a.reps)
    res["b_forward_multi_ms_per_frame_batch4"] = timed(lambda: head.forward_multi(imgs, masks, standardize=True), max(1, a.reps // 4)) / 4
    res["a_over_b_batch1"] = res["a_per_channel_route_ms_per_frame"] / res["b_forward_multi_ms_per_frame_batch1"]
    res["a_over_b_batch4"] = res["a_per_channel_route_ms_per_frame"] / res["b_forward_multi_ms_per_frame_batch4"]
    # (c): the kernels alone, on clustered features (a bimodal Gram) of the real size
    hf, wf, tau, eps = 60, 107, 0.2, 1e-5
    n = hf * wf
    npad = (n + 3) // 4 * 4
    feats = torch.from_numpy(synth.maa_features(101, hf, wf, 1.2)).to(dev)
    x = torch.from_numpy(synth.maa_masks(211, hf, wf, M)).to(dev).reshape(1, M, n).contiguous()
    fn = ops.l2_normalize_rows(feats[0, 1:].contiguous())
    G = torch.empty((1, n, npad), dtype=torch.float32, device=dev)
    ops.gemm_nt(fn, fn, out=G[0, :, :n])
    out = torch.empty((1, M, 4), dtype=torch.float64, device=dev)
    nbytes = _lib.load().rcf_ncut_values_workspace_bytes(1, n, M)
    ws = torch.empty(nbytes, dtype=torch.uint8, device=dev)
    new = lambda: _lib.call("rcf_ncut_values_f32", _p(G), npad, n, 1, tau, eps, _p(x), M, _p(out), _p(ws), nbytes, _stream())
    A = G[0].clone()
    u, s = torch.empty(n, dtype=torch.float64, device=dev), torch.empty(n, dtype=torch.float64, device=dev)
    val = torch.empty(1, dtype=torch.float32, device=dev)

    def old():
        # the threshold pass is idempotent on an affinity (1 > tau, eps < tau), so repeating it on A moves the same bytes
        _lib.call("rcf_affinity_threshold_f32", _p(A), npad, n, tau, eps, _stream())
        for c in range(M):
            _lib.call("rcf_ncut_value_grad_f32", _p(A), npad, n, _p(x[0, c]), _p(u), _p(s), 1 if c == 0 else 0, None, _p(val), _stream())

    # alternate the two routes, so that a drift of the clock hits both
    t_new, t_old = [], []
    for _ in range(3):
        t_new.append(timed(new, a.kernel_reps))
        t_old.append(timed(old, max(1, a.kernel_reps // 4)))
    res["c_new_kernel_ms"] = min(t_new)
    res["c_new_kernel_ms_runs"] = t_new
    res["c_threshold_plus_M_matvec_ms"] = min(t_old)
    res["c_threshold_plus_M_matvec_ms_runs"] = t_old
    res["c_speedup"] = min(t_old) / min(t_new)
    # (d)
    moved = n * npad * 4 + M * n * 4 + nbytes
    res["d_new_kernel_bytes"] = moved
    res["d_new_kernel_TB_per_s"] = moved / (min(t_new) * 1e-3) / 1e12
    res["d_share_of_copy_rate"] = res["d_new_kernel_TB_per_s"] / COPY_RATE_TBS
    res["d_note"] = "a 165 MB Gram fits the 256 MiB Infinity Cache: repeated launches on a resident Gram can exceed the HBM copy rate"
    res["device_name"] = torch.cuda.get_device_name(0)
    print(json.dumps(res))


if __name__ == "__main__":
    main()
