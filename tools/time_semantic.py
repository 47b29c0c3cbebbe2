#!/usr/bin/env python
"""ms per 480x854 frame of the semantic-constraint refinement (n = 6420 tokens, 10 Adam steps, two 50-iteration CRFs), 4 frames
per call, one process, host clock around work that ends in a device synchronise, medians of repeated runs after warm-up:
 (a) the per-frame route as it stood before the batched one: NCutHead.forward + offline.double_crf_merge, one frame at a time,
     the result scaled to u8 and copied to the host (umi_th None as for davis / stv2, and 10000 as for fbms59);
 (b) the batched route: NCutHead.forward_batch + offline.double_crf_merge_u8 on the 4 frames, one copy to the host;
 (c) the parts, on the same 4 frames: the ViT forward (with the resizes), the NCut refinement alone on resident features --
     ncut.ncut_refine per frame against ncut.ncut_refine_batch, the latter also split into Gram + pack and the Adam steps --
     and the two CRFs + merge per frame against batched.
The two routes alternate inside every repetition, so a drift of the clock hits both.

    python tools/time_semantic.py [--reps 7]"""
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

from rcf_amd import crf, ncut, offline, ops, semantic, synth, vit  # noqa: E402

FRAMES = 4


def wall_ms(fn):
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    fn()
    torch.cuda.synchronize()
    return (time.perf_counter() - t0) * 1e3


def alternate(fns, reps, warmup=2):
    """{name: [ms per call] * reps}; every repetition runs each fn once, in turn"""
    for _ in range(warmup):
        for fn in fns.values():
            fn()
    runs = {k: [] for k in fns}
    for _ in range(reps):
        for k, fn in fns.items():
            runs[k].append(wall_ms(fn))
    return runs


def summary(runs, per=FRAMES):
    return {k: {"median_ms_per_frame": statistics.median(v) / per, "min": min(v) / per, "max": max(v) / per,
                "spread_pct": 100.0 * (max(v) - min(v)) / statistics.median(v)} for k, v in runs.items()}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=7)
    a = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("time_semantic.py measures the device: no GPU here")
    dev = "cuda"
    m = vit.vit_small(patch_size=8)
    shapes = {k: tuple(v.shape) for k, v in m.state_dict().items()}
    m.load_state_dict({k: torch.from_numpy(v) for k, v in synth.fill_vit_state_dict(shapes, seed=21).items()})
    head = ncut.NCutHead(args=None, model=m, **semantic.NCUT_KW).to(dev).eval()
    single = crf.CRFHead(args=None, crf_scale=semantic.CRF_SCALE_SINGLE, **semantic.CRF_KW)
    double = crf.CRFHead(args=None, crf_scale=semantic.CRF_SCALE, **semantic.CRF_KW)
    g = np.random.default_rng(3)
    frames = [synth._maa_frame(g, t % 3, t) for t in range(FRAMES)]              # flat coloured regions with mild noise
    imgs = torch.from_numpy(np.stack([f[0].astype(np.float32) / 255. for f in frames])).to(dev)
    masks = torch.from_numpy(np.stack([np.where(np.roll(f[1], (40, 60), axis=(0, 1)), 0.9, 0.1).astype(np.float32) for f in frames])).to(dev)

    def per_frame(umi_th):
        out = []
        for i in range(FRAMES):
            refined = head(imgs[i:i + 1], masks[i:i + 1], standardize=True)
            merged = offline.double_crf_merge(single, double, imgs[i:i + 1], masks[i:i + 1], refined, umi_th=umi_th)
            out.append((merged[0] * 255.).to(torch.uint8).cpu())
        return out

    def batched(umi_th):
        refined = head.forward_batch(imgs, masks, standardize=True)
        return offline.double_crf_merge_u8(single, double, imgs, masks, refined, umi_th=umi_th).cpu()

    same = all(torch.equal(p, b) for p, b in zip(per_frame(10000), batched(10000)))
    res = {"H": 480, "W": 854, "tokens": 6420, "frames_per_call": FRAMES, "reps": a.reps, "outputs_of_the_two_routes_equal": bool(same)}
    res["routes"] = summary(alternate({"a_per_frame_umi_none": lambda: per_frame(None), "b_batched_umi_none": lambda: batched(None),
                                       "a_per_frame_umi_10000": lambda: per_frame(10000), "b_batched_umi_10000": lambda: batched(10000)}, a.reps))
    r = res["routes"]
    for k in ("umi_none", "umi_10000"):
        res[f"a_over_b_{k}"] = r[f"a_per_frame_{k}"]["median_ms_per_frame"] / r[f"b_batched_{k}"]["median_ms_per_frame"]
    # (c) the parts.  Features that tell regions apart (the seeded ViT's are nearly identical; the kernels' time does not
    # depend on the bits, but the comparison should run on a real-looking affinity)
    hf, wf = head.h_featuremap, head.w_featuremap
    n = hf * wf
    feats = torch.cat([torch.from_numpy(synth.maa_features(101 + i, hf, wf, 1.2)) for i in range(FRAMES)]).to(dev)
    small = torch.from_numpy(np.stack([synth.maa_masks(211 + i, hf, wf, 1)[0] for i in range(FRAMES)])).to(dev)
    kw = dict(tau=head.tau, eps=head.eps, **semantic.NCUT_KW)
    fnorm = ops.l2_normalize_rows(feats[:, 1:].reshape(FRAMES * n, -1).contiguous()).view(FRAMES, n, -1)
    npad = (n + 3) // 4 * 4
    G = torch.empty((n, npad), dtype=torch.float32, device=dev)
    bits = torch.empty((FRAMES, n, ncut.pack_words(n)), dtype=torch.int32, device=dev)
    deg = torch.empty((FRAMES, n), dtype=torch.int32, device=dev)

    def gram_pack():
        for b in range(FRAMES):
            ops.gemm_nt(fnorm[b], fnorm[b], out=G[:, :n])
            ncut.affinity_pack(G, n, head.tau, bits[b:b + 1], deg[b:b + 1])

    def pack_only():
        for b in range(FRAMES):
            ncut.affinity_pack(G, n, head.tau, bits[b:b + 1], deg[b:b + 1])

    gram_pack()
    x0 = small.reshape(FRAMES, n).contiguous()
    refined = head.forward_batch(imgs, masks, standardize=True)

    def crfs_per_frame():
        for i in range(FRAMES):
            offline.double_crf_merge(single, double, imgs[i:i + 1], masks[i:i + 1], refined[i:i + 1], umi_th=10000)

    parts = {
        "vit_forward_with_resizes_batch4": lambda: head.get_feats(head._inputs(imgs, masks, True)[0]),
        "refine_per_frame_ncut_refine": lambda: [ncut.ncut_refine(feats[b:b + 1], small[b], **kw) for b in range(FRAMES)],
        "refine_batched_ncut_refine_batch": lambda: ncut.ncut_refine_batch(feats, small, **kw),
        "refine_batched_gram_and_pack": gram_pack,
        "refine_batched_pack_only": pack_only,
        "refine_batched_adam_steps_20_launches": lambda: ncut.refine_packed(bits, deg, x0.clone(), head.eps, 10, 0.45, 1e-6),
        "crfs_and_merge_per_frame_umi_10000": crfs_per_frame,
        "crfs_and_merge_batched_umi_10000": lambda: offline.double_crf_merge_u8(single, double, imgs, masks, refined, umi_th=10000),
    }
    res["parts"] = summary(alternate(parts, a.reps))
    p = res["parts"]
    res["refine_per_frame_over_batched"] = (p["refine_per_frame_ncut_refine"]["median_ms_per_frame"] /
                                            p["refine_batched_ncut_refine_batch"]["median_ms_per_frame"])
    res["bytes_per_frame"] = {"gram_read_by_the_pack": n * n * 4, "bits_and_popcounts_written": n * ncut.pack_words(n) * 4 + n * 4,
                              "threshold_pass_replaced_read_plus_write": 2 * n * n * 4}
    res["device_name"] = torch.cuda.get_device_name(0)
    print(json.dumps(res))


if __name__ == "__main__":
    main()
