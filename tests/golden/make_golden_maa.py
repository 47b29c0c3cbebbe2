#!/usr/bin/env python3
"""Golden values for the MAA channel selection (rcf_amd.maa, ncut.soft_ncut_values), captured from the REFERENCE:
`soft_ncut_value` of tools/SemanticConstraintsAndMAA/maa.py and its three `val_seqs` lists, both extracted with `ast`
(the script itself imports matplotlib / tqdm and runs on import).  Run in the build container only (CPU):
    python tests/golden/make_golden_maa.py
    python tests/golden/make_golden_maa.py --scan-mask-seeds CASE      (how the mask seeds of CASES were picked: see there)
Writes tests/golden/maa.json: for every case the seeds and shapes and, per mask, the reference's fp32 value (float.hex), the
same expression in float64, their relative deviation and the number of Gram entries within 1e-5 of tau; for the synthetic
tree (synth.maa_tree + synth.PatchFeatures on the CPU) the per-frame, per-channel values, the frame MAAs and the best
channel.  No reference text goes into the file.
"""
import ast
import json
import os
import sys
import tempfile

import numpy as np
import torch
import torch.nn.functional as F

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(os.path.dirname(HERE))
REF = "/root/reference"
sys.path.insert(0, ROOT)

TAU, EPS = 0.2, 1e-5
TREE_TOL = 1e-4                      # tests/test_maa_gpu.py: the bar on anything computed from device-side image preprocessing
# (name, feature seed, mask seed, hf, wf, M, noise, all-zero masks)
CASES = [("n6420_noise1.2", 101, 211, 60, 107, 4, 1.2, False), ("n6420_noise2.0", 102, 202, 60, 107, 4, 2.0, False),
         ("n6527_padded", 103, 203, 61, 107, 3, 1.2, False), ("n63_m1", 104, 204, 7, 9, 1, 1.2, False),
         ("n63_m3", 105, 205, 7, 9, 3, 1.2, False), ("n63_m8", 106, 206, 7, 9, 8, 1.2, False),
         ("n63_zero_mask", 107, 207, 7, 9, 1, 1.2, True)]


def gram_float64(feats):
    f = F.normalize(feats[0, 1:, :].double(), p=2)
    return f @ f.T


def ncut_float64(G, mask, tau, eps):
    """the expression of maa.py:19-36 with every operand in float64, on the float64 Gram matrix G -> (ncut, cut, assocA, assocB)"""
    A = torch.where(G > tau, 1.0, eps).double()
    x = mask.reshape(-1).double()
    u = A @ x
    cut, aA, aB = (1 - x) @ u, u.sum(), (A @ (1 - x)).sum()
    return float(cut / aA + cut / aB), float(cut), float(aA), float(aB)


def rel_dev(a, b):
    if np.isnan(a) and np.isnan(b):
        return 0.0
    return abs(a - b) / abs(b)


def scan_mask_seeds(name, ref_ncut, synth, tries=200):
    """The reference's own fp32 error at n = 6420 is of the order of the 1e-6 this generator asserts (its NCut goes through
    sequential fp32 sums of 6420 terms), and whether a given mask stays below depends on the mask.  This prints the first
    mask seed from the case's own on for which EVERY mask of the case does: the seed then goes into CASES.  The choice
    looks at the reference alone (fp32 against float64); nothing of the code under test is involved."""
    _, fseed, mseed, hf, wf, M, noise, _ = next(c for c in CASES if c[0] == name)
    with torch.no_grad():
        feats = torch.from_numpy(synth.maa_features(fseed, hf, wf, noise))
        G = gram_float64(feats)
        for seed in range(mseed, mseed + tries):
            masks = torch.from_numpy(synth.maa_masks(seed, hf, wf, M))
            devs = []
            for m in range(M):
                devs.append(rel_dev(float(ref_ncut(feats, masks[m], TAU, EPS)), ncut_float64(G, masks[m], TAU, EPS)[0]))
                if devs[-1] >= 1e-6:
                    break
            print(name, "mask seed", seed, " ".join(f"{d:.2e}" for d in devs), flush=True)
            if len(devs) == M and max(devs) < 1e-6:
                return seed
    raise SystemExit(f"no mask seed in [{mseed}, {mseed + tries}) keeps the reference within 1e-6 on {name}")


def main():
    import rcf_amd                                           # noqa
    from rcf_amd import synth
    src = open(os.path.join(REF, "tools", "SemanticConstraintsAndMAA", "maa.py")).read()
    tree = ast.parse(src)
    fns = [n for n in tree.body if isinstance(n, ast.FunctionDef) and n.name == "soft_ncut_value"]
    ns = {"torch": torch, "F": F}
    exec(compile(ast.Module(body=fns, type_ignores=[]), "maa.py", "exec"), ns)
    ref_ncut = ns["soft_ncut_value"]
    lists = sorted((n for n in ast.walk(tree) if isinstance(n, ast.Assign) and len(n.targets) == 1 and
                    isinstance(n.targets[0], ast.Name) and n.targets[0].id == "val_seqs"), key=lambda n: n.lineno)
    assert len(lists) == 3
    val_seqs = dict(zip(("davis", "stv2", "fbms59"), (ast.literal_eval(n.value) for n in lists)))

    torch.manual_seed(0)
    torch.set_num_threads(8)
    if len(sys.argv) > 2 and sys.argv[1] == "--scan-mask-seeds":
        return scan_mask_seeds(sys.argv[2], ref_ncut, synth)
    out = {"tau": TAU, "eps": EPS, "val_seqs": val_seqs, "cases": []}
    with torch.no_grad():
        for name, fseed, mseed, hf, wf, M, noise, zero in CASES:
            feats = torch.from_numpy(synth.maa_features(fseed, hf, wf, noise))
            masks = torch.from_numpy(synth.maa_masks(mseed, hf, wf, M))
            if zero:
                masks = torch.zeros_like(masks)
            G = gram_float64(feats)
            vals, near = [], int(((G - TAU).abs() < 1e-5).sum())
            for m in range(M):
                r32 = float(ref_ncut(feats, masks[m], TAU, EPS))
                r64, cut, aA, aB = ncut_float64(G, masks[m], TAU, EPS)
                dev = rel_dev(r32, r64)
                assert dev < 1e-6, (name, m, r32, r64, dev)        # the reference alone stays inside the test's bars
                vals.append({"ref_f32_hex": float(r32).hex(), "ref_f32": None if np.isnan(r32) else r32,
                             "f64": None if np.isnan(r64) else r64, "cut64": cut, "assocA64": aA, "assocB64": aB,
                             "rel_dev": dev})
                print(name, m, r32, r64, f"{dev:.2e}", flush=True)
            out["cases"].append({"name": name, "feature_seed": fseed, "mask_seed": mseed, "hf": hf, "wf": wf, "M": M,
                                 "noise": noise, "zero_masks": zero, "gram_entries_near_tau": near, "masks": vals})

        # the synthetic tree: the reference's function on PatchFeatures (CPU), its mask path restated with PIL + F.interpolate
        from PIL import Image
        model = synth.PatchFeatures().eval()
        mean = torch.tensor((0.485, 0.456, 0.406))[None, :, None, None]
        std = torch.tensor((0.229, 0.224, 0.225))[None, :, None, None]
        frames, per_frame, near_max = [], [], 0
        with tempfile.TemporaryDirectory() as tmp:
            pretrain_dir, data_dir = synth.maa_tree(tmp)
            images = os.path.join(data_dir, "data_davis", "JPEGImages", "480p")
            for seq, T, _ in synth.MAA_TREE:
                for t in range(T):
                    fid = f"{t:05d}"
                    img = np.asarray(Image.open(os.path.join(images, seq, fid + ".jpg")).convert("RGB")).astype(np.float32) / 255.
                    assert img.shape == (480, 854, 3)
                    x = (torch.from_numpy(img)[None].permute(0, 3, 1, 2) - mean) / std
                    x = F.interpolate(x, (480, 856), mode="bilinear")
                    feats = model.get_last_qkv(x, "k")
                    row = []
                    for ch in range(synth.MAA_TREE_CHANNELS):
                        p = os.path.join(pretrain_dir, "saved_eval_export", str(ch), f"pred_seg_{seq}_{fid}_{0:07}.png")
                        mk = np.asarray(Image.open(p).resize((854, 480))).astype(np.float32) / 255.
                        mk = mk[..., 0] if mk.ndim == 3 else mk
                        small = F.interpolate(torch.from_numpy(mk)[None, None], (60, 107), mode="nearest")[0, 0]
                        row.append(np.float32(ref_ncut(feats, small, TAU, EPS)))
                    near = int(((gram_float64(feats) - TAU).abs() < 1e-5).sum())
                    near_max = max(near_max, near)
                    assert near <= 10, (seq, fid, near)
                    frames.append(f"{seq}/{fid}")
                    per_frame.append(row)
                    print(seq, fid, [float(v) for v in row], "near tau", near, flush=True)
        vals = np.array(per_frame, dtype=np.float32)                       # [frames, channels]
        frame_maas = [float(np.mean(list(-vals[:, c]))) for c in range(vals.shape[1])]
        best = int(np.argmax(np.array(frame_maas)))
        order = np.sort(frame_maas)
        assert order[-1] - order[-2] >= 100 * TREE_TOL * abs(order[-1]), frame_maas
        assert best == synth.MAA_TREE_OBJECT
        first = [i for i, f in enumerate(frames) if f.endswith("/00000")]
        out["tree"] = {"frames": frames, "ncut_f32_hex": [[float(v).hex() for v in r] for r in vals],
                       "ncut": [[float(v) for v in r] for r in vals], "frame_maas": frame_maas, "best_channel": best,
                       "first_frames": first,
                       "frame_maas_first_frames": [float(np.mean(list(-vals[first, c]))) for c in range(vals.shape[1])],
                       "gram_entries_near_tau_max": near_max}
    with open(os.path.join(HERE, "maa.json"), "w") as f:
        json.dump(out, f, indent=1)
    print("tree frame MAAs", frame_maas, "best", best)


if __name__ == "__main__":
    main()
