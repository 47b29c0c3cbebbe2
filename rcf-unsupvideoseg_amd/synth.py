"""Deterministic synthetic inputs and weights.

Everything comes from numpy `Generator(PCG64(seed))`, so the build container and the GPU
box produce identical bytes.  seed = 1000 * config_id + sample_index for data; weights
have their own seed.  No dataset or checkpoint exists in either environment.
"""
import numpy as np
import torch

IMAGENET_MEAN = np.array([0.485, 0.456, 0.406], dtype=np.float32)   # dataset/transforms.py:893
IMAGENET_STD = np.array([0.229, 0.224, 0.225], dtype=np.float32)


def _rng(seed):
    return np.random.Generator(np.random.PCG64(int(seed)))


def smooth_rgb(H, W, seed):
    """u8 [H,W,3]: low-frequency sinusoids + 3 coloured convex blobs + N(0,4) noise."""
    g = _rng(seed)
    yy, xx = np.meshgrid(np.arange(H, dtype=np.float32), np.arange(W, dtype=np.float32), indexing="ij")
    img = np.zeros((H, W, 3), dtype=np.float32)
    for c in range(3):
        acc = np.full((H, W), 128.0, dtype=np.float32)
        for _ in range(4):
            fy, fx = g.uniform(0.5, 3.0, size=2) * 2 * np.pi / np.array([H, W])
            ph, amp = g.uniform(0, 2 * np.pi), g.uniform(10, 40)
            acc += amp * np.sin(fy * yy + fx * xx + ph).astype(np.float32)
        img[..., c] = acc
    for _ in range(3):
        cy, cx = g.uniform(0.2, 0.8) * H, g.uniform(0.2, 0.8) * W
        ry, rx = g.uniform(0.08, 0.25) * H, g.uniform(0.08, 0.25) * W
        col = g.uniform(0, 255, size=3).astype(np.float32)
        inside = ((yy - cy) / ry) ** 2 + ((xx - cx) / rx) ** 2 < 1.0
        img[inside] = 0.25 * img[inside] + 0.75 * col
    img += g.normal(0, 2.0, size=img.shape).astype(np.float32)
    return np.clip(img, 0, 255).astype(np.uint8)


def noise_rgb(H, W, seed):
    """u8 [H,W,3] uniform noise: worst-case permutohedral lattice occupancy."""
    return _rng(seed).integers(0, 256, size=(H, W, 3), dtype=np.uint8)


def voronoi_affine_flow(H, W, seed, nseg=3, max_mag=20.0):
    """f32 [2,H,W] (x,y pixel units): per-Voronoi-cell affine motion, |flow| <= max_mag, + N(0,0.25)."""
    g = _rng(seed)
    yy, xx = np.meshgrid(np.arange(H, dtype=np.float32), np.arange(W, dtype=np.float32), indexing="ij")
    sites = np.stack([g.uniform(0, H, nseg), g.uniform(0, W, nseg)], 1)
    d = np.stack([(yy - sy) ** 2 + (xx - sx) ** 2 for sy, sx in sites], 0)
    seg = np.argmin(d, 0)
    flow = np.zeros((2, H, W), dtype=np.float32)
    for k in range(nseg):
        A = g.normal(0, 0.02, size=(2, 2)).astype(np.float32)
        t = g.uniform(-8, 8, size=2).astype(np.float32)
        u = A[0, 0] * (xx - W / 2) + A[0, 1] * (yy - H / 2) + t[0]
        v = A[1, 0] * (xx - W / 2) + A[1, 1] * (yy - H / 2) + t[1]
        m = seg == k
        flow[0][m], flow[1][m] = u[m], v[m]
    flow += g.normal(0, 0.5, size=flow.shape).astype(np.float32)
    mag = np.sqrt((flow ** 2).sum(0, keepdims=True))
    flow *= np.minimum(1.0, max_mag / np.maximum(mag, 1e-6))
    return flow.astype(np.float32), seg.astype(np.uint8)


def warp_np(img, flow):
    """Backward bilinear warp (border clamp) of f32 [C,H,W] by flow [2,H,W]; numpy only."""
    C, H, W = img.shape
    yy, xx = np.meshgrid(np.arange(H, dtype=np.float32), np.arange(W, dtype=np.float32), indexing="ij")
    x = np.clip(xx + flow[0], 0, W - 1)
    y = np.clip(yy + flow[1], 0, H - 1)
    x0, y0 = np.floor(x).astype(np.int64), np.floor(y).astype(np.int64)
    x1, y1 = np.minimum(x0 + 1, W - 1), np.minimum(y0 + 1, H - 1)
    ax, ay = (x - x0).astype(np.float32), (y - y0).astype(np.float32)
    out = (img[:, y0, x0] * (1 - ax) * (1 - ay) + img[:, y0, x1] * ax * (1 - ay)
           + img[:, y1, x0] * (1 - ax) * ay + img[:, y1, x1] * ax * ay)
    return out.astype(np.float32)


def normalize_rgb(u8):
    """u8 [H,W,3] -> f32 [3,H,W], ImageNet-normalised (dataset/transforms.py:893)."""
    x = u8.astype(np.float32) / 255.0
    return ((x - IMAGENET_MEAN) / IMAGENET_STD).transpose(2, 0, 1).copy()


def make_pair(H, W, seed):
    """One training sample: 2 normalised frames + fw + bw flow (SURVEY Appendix F shapes)."""
    rgb0 = smooth_rgb(H, W, seed)
    fw, _ = voronoi_affine_flow(H, W, seed + 500000)
    f0 = rgb0.astype(np.float32).transpose(2, 0, 1)
    f1 = np.clip(warp_np(f0, fw), 0, 255)                    # frame 1 = frame 0 backward-warped
    bw = -warp_np(fw, fw)                                    # bw flow = -fw warped
    rgb1 = f1.transpose(1, 2, 0).astype(np.uint8)
    return normalize_rgb(rgb0), normalize_rgb(rgb1), fw, bw.astype(np.float32)


def make_batch(B, H, W, config_id=1, first_index=0):
    """Batch dict in the layout `RCFModel.forward` consumes (numpy arrays; caller converts)."""
    s = [make_pair(H, W, 1000 * config_id + first_index + i) for i in range(B)]
    return {
        "imgs": [np.stack([p[0] for p in s]), np.stack([p[1] for p in s])],
        "gt_fw_flows": [np.stack([p[2] for p in s])],
        "gt_bw_flows": [np.stack([p[3] for p in s])],
        "seq_ids": np.arange(B, dtype=np.int64),
        "seq_names": [f"synth{first_index + i}" for i in range(B)],
        "paths": [[f"synth/{first_index + i:05d}.jpg" for i in range(B)] for _ in range(2)],
    }


def dropout_scale(n, channels, p=0.1, seed=0):
    """f32 [n, channels]: one nn.Dropout2d draw written down -- Bernoulli(1 - p) per (sample, channel) plane, kept planes
    scaled by 1 / (1 - p) (models/decode_head.py:84-87, models/fcn_head.py:142-147).  Parity tests hand the SAME draw to the
    reference / oracle (oracle.FixedDropout2d) and to FCNHead.keep_mask."""
    keep = (_rng(910000 + seed).uniform(size=(n, channels)) >= p).astype(np.float32)
    return keep / np.float32(1.0 - p)


def soft_blob_mask(H, W, seed):
    """f32 [H,W] in [0,1]: Gaussian-blurred blob (CRF input of SURVEY §8(d))."""
    g = _rng(seed)
    yy, xx = np.meshgrid(np.arange(H, dtype=np.float32), np.arange(W, dtype=np.float32), indexing="ij")
    cy, cx = g.uniform(0.3, 0.7) * H, g.uniform(0.3, 0.7) * W
    ry, rx = g.uniform(0.15, 0.3) * H, g.uniform(0.15, 0.3) * W
    d = np.sqrt(((yy - cy) / ry) ** 2 + ((xx - cx) / rx) ** 2)
    return (1.0 / (1.0 + np.exp((d - 1.0) * 6.0))).astype(np.float32)


def make_pl_masks(B, H, W, config_id=1, first_index=0):
    """batch['pl_masks'] of stage 2.2 (dataset/data.py:137-151): one soft mask in [0,1] per frame, 2 x [B,H,W]"""
    return [np.stack([soft_blob_mask(H, W, 1000 * config_id + first_index + i + 7000 * (f + 1)) for i in range(B)])
            for f in range(2)]


def loader_sample(seed, H=480, W=854):
    """What dataset/data.py:73-151 hands to the transform for one training sample, decoded: frames u8 [2,H,W,3] (smooth
    content; the right quarter is uniform noise so that every hue sector / saturation extreme occurs), forward / backward
    flow fp32 [H,W,2] (the `.npy` layout, :122-128) and pseudo-label masks u8 [2,H,W] (:137-150)."""
    frames = np.stack([smooth_rgb(H, W, seed + 31 * i) for i in range(2)])
    for i in range(2):
        frames[i, :, W - W // 4:] = noise_rgb(H, W // 4, seed + 77 + i)
    fw, _ = voronoi_affine_flow(H, W, seed + 500000)
    bw, _ = voronoi_affine_flow(H, W, seed + 600000)
    pl = np.stack([np.round(soft_blob_mask(H, W, seed + 7000 * (i + 1)) * 255.0).astype(np.uint8) for i in range(2)])
    return dict(frames=frames, fw=np.ascontiguousarray(fw.transpose(1, 2, 0)), bw=np.ascontiguousarray(bw.transpose(1, 2, 0)), pl=pl)


def eval_inputs(seed, N=6, C=4, h=30, w=54, H=120, W=214):
    """Inputs of the evaluation-metric fixtures (tests/golden/make_golden_eval.py): smooth soft masks [N,C,h,w] (softmax
    of low-frequency logits), annotations [N,H,W] u8 in {0, 128 (ignore), 255}, sequence names (two frames each)."""
    g = _rng(seed)
    yy, xx = np.meshgrid(np.arange(h, dtype=np.float32), np.arange(w, dtype=np.float32), indexing="ij")
    logits = np.zeros((N, C, h, w), dtype=np.float32)
    for n in range(N):
        for c in range(C):
            for _ in range(3):
                fy, fx = g.uniform(0.5, 2.5, size=2) * 2 * np.pi / np.array([h, w])
                logits[n, c] += g.uniform(1.0, 3.0) * np.sin(fy * yy + fx * xx + g.uniform(0, 2 * np.pi)).astype(np.float32)
    e = np.exp(logits - logits.max(axis=1, keepdims=True))
    masks = (e / e.sum(axis=1, keepdims=True)).astype(np.float32)
    YY, XX = np.meshgrid(np.arange(H, dtype=np.float32), np.arange(W, dtype=np.float32), indexing="ij")
    ann = np.zeros((N, H, W), dtype=np.uint8)
    for n in range(N):
        cy, cx = g.uniform(0.3, 0.7) * H, g.uniform(0.3, 0.7) * W
        ry, rx = g.uniform(0.15, 0.35) * H, g.uniform(0.15, 0.35) * W
        d = ((YY - cy) / ry) ** 2 + ((XX - cx) / rx) ** 2
        ann[n][d < 1.0] = 255
        ann[n][(d >= 1.0) & (d < 1.15)] = 128                  # a ring of "ignore" pixels around the object
    ann[N - 1] = 0                                             # an empty annotation
    names = [f"seq{n // 2}" for n in range(N)]
    return masks, ann, names


DAVIS_KINDS = ("blobs", "empty_pred", "empty_gt", "both_empty", "all_ones", "pixels", "lines", "checker")


def _davis_blobs(g, H, W):
    """u8 [H,W]: integer discs, rectangles, 1-px lines and sparse noise -- no pixel sits on a float threshold"""
    m = np.zeros((H, W), dtype=np.uint8)
    yy, xx = np.ogrid[:H, :W]
    for _ in range(int(g.integers(1, 4))):
        cy, cx = int(g.integers(0, H)), int(g.integers(0, W))
        rr = int(g.integers(1, max(2, min(H, W) // 3)))
        m[(yy - cy) ** 2 + (xx - cx) ** 2 <= rr * rr] = 1
    for _ in range(int(g.integers(0, 3))):
        y0, x0 = int(g.integers(0, H)), int(g.integers(0, W))
        m[y0:y0 + int(g.integers(1, H + 1)), x0:x0 + int(g.integers(1, W + 1))] ^= 1
    if H > 2 and W > 2:
        m[int(g.integers(0, H)), :] ^= 1
        m[:, int(g.integers(0, W))] ^= 1
    m[g.integers(0, 1000, size=(H, W)) < 3] ^= 1
    return m


def davis_inputs(seed, N=1, H=480, W=854, kind="blobs", void=False):
    """Inputs of the DAVIS-metric fixtures (tests/golden/make_golden_davis.py): pred, gt u8 [N,H,W] in {0,1} and, with
    `void`, a u8 [N,H,W] void mask (a rectangle plus sparse pixels), else None.  Integer arithmetic only."""
    g = _rng(seed)
    pred, gt = np.zeros((N, H, W), dtype=np.uint8), np.zeros((N, H, W), dtype=np.uint8)
    for n in range(N):
        if kind == "blobs":
            gt[n] = _davis_blobs(g, H, W)
            pred[n] = gt[n].copy()
            dy, dx = int(g.integers(-3, 4)), int(g.integers(-3, 4))
            pred[n] = np.roll(pred[n], (dy, dx), axis=(0, 1))
            pred[n] ^= (_davis_blobs(g, H, W) & (g.integers(0, 4, size=(H, W)) == 0)).astype(np.uint8)
        elif kind in ("empty_pred", "empty_gt"):
            m = _davis_blobs(g, H, W)
            (gt if kind == "empty_pred" else pred)[n] = m
        elif kind == "all_ones":
            pred[n], gt[n] = 1, 1
        elif kind == "pixels":                       # single pixels in the corners and on the edges
            for y, x in ((0, 0), (0, W - 1), (H - 1, 0), (H - 1, W - 1)):
                (pred if g.integers(0, 2) else gt)[n, y, x] = 1
            for _ in range(4):
                pred[n, 0, int(g.integers(0, W))] = 1
                gt[n, H - 1, int(g.integers(0, W))] = 1
                pred[n, int(g.integers(0, H)), W - 1] = 1
                gt[n, int(g.integers(0, H)), 0] = 1
        elif kind == "lines":                        # 1-px lines: horizontal, vertical, diagonal
            for a in (pred[n], gt[n]):
                a[int(g.integers(0, H)), :] = 1
                a[:, int(g.integers(0, W))] = 1
                k = int(g.integers(-W, H))
                yy, xx = np.ogrid[:H, :W]
                a[(yy - xx) == k] = 1
        elif kind == "checker":
            yy, xx = np.ogrid[:H, :W]
            gt[n] = ((yy + xx) % 2).astype(np.uint8)
            pred[n] = (((yy // 2) + (xx // 3)) % 2).astype(np.uint8)
        elif kind != "both_empty":
            raise ValueError(f"unknown kind {kind}")
    vd = None
    if void:
        vd = (g.integers(0, 200, size=(N, H, W)) == 0).astype(np.uint8)
        y0, x0 = int(g.integers(0, H)), int(g.integers(0, W))
        vd[:, y0:y0 + max(1, H // 4), x0:x0 + max(1, W // 5)] = 1
    return pred, gt, vd


DAVIS_TREE = (("bear", 6, None), ("car-turn", 5, (240, 427)), ("dance", 7, None))   # (sequence, frames, export size)


def davis_tree(root, seed=2016, step=0):
    """A synthetic DAVIS-2016 tree under `root`: ImageSets/480p/val.txt, JPEGImages/480p (tiny placeholder files: only
    their number is read), Annotations/480p (u8 PNG, 0 / 255, 480x854) and, under root/results, the exported
    pred_seg_{seq}_{id}_{step:07}.png masks (RGB PNG; one sequence exported at 240x427, so the evaluator resizes it).
    Returns (davis_path, results_path)."""
    import os
    from PIL import Image
    g = _rng(seed)
    res = os.path.join(root, "results")
    os.makedirs(os.path.join(root, "ImageSets", "480p"), exist_ok=True)
    os.makedirs(res, exist_ok=True)
    lines = []
    for si, (seq, T, size) in enumerate(DAVIS_TREE):
        for d in ("JPEGImages", "Annotations"):
            os.makedirs(os.path.join(root, d, "480p", seq), exist_ok=True)
        _, gt, _ = davis_inputs(seed + si, N=T, H=480, W=854, kind="blobs")
        for t in range(T):
            fid = f"{t:05d}"
            lines.append(f"/JPEGImages/480p/{seq}/{fid}.jpg /Annotations/480p/{seq}/{fid}.png\n")
            with open(os.path.join(root, "JPEGImages", "480p", seq, fid + ".jpg"), "wb") as f:
                f.write(b"placeholder")
            Image.fromarray(gt[t] * 255).save(os.path.join(root, "Annotations", "480p", seq, fid + ".png"))
            # prediction: the annotation shifted, with a blob toggled; u8 0 / 255 with a few mid-grey pixels
            p = np.roll(gt[t], (int(g.integers(-6, 7)), int(g.integers(-6, 7))), axis=(0, 1)) * 255
            p[(_davis_blobs(g, 480, 854) == 1) & (g.integers(0, 3, size=(480, 854)) == 0)] ^= 255
            p[g.integers(0, 50, size=(480, 854)) == 0] = 128
            if si == 1 and t == 2:
                p[:] = 0                                           # an empty prediction frame
            img = Image.fromarray(np.stack([p, p, p], -1).astype(np.uint8))
            if size is not None:
                img = img.resize((size[1], size[0]), resample=Image.NEAREST)
            img.save(os.path.join(res, f"pred_seg_{seq}_{fid}_{step:07}.png"))
    with open(os.path.join(root, "ImageSets", "480p", "val.txt"), "w") as f:
        f.writelines(lines)
    return root, res


# ---- MAA (motion-appearance alignment, rcf_amd.maa): inputs on which the soft NCut tells masks apart -----------------------
# The seeded ViT weights give nearly identical tokens (affinity all ones, NCut == 1 for every mask), so these fixtures
# bring their own features: clustered keys laid out as spatial regions.


def maa_regions(hf, wf):
    """int [hf,wf] region labels: background 0, a rectangle 1, an ellipse 2, a bottom band 3"""
    yy, xx = np.mgrid[:hf, :wf]
    lab = np.zeros((hf, wf), dtype=np.int64)
    lab[yy >= hf - max(1, hf // 6)] = 3
    lab[(yy >= hf // 8) & (yy < hf // 8 + max(1, hf // 3)) & (xx >= wf // 10) & (xx < wf // 10 + max(1, wf // 4))] = 1
    cy, cx, ry, rx = 0.5 * hf, 0.68 * wf, max(1.0, 0.22 * hf), max(1.0, 0.18 * wf)
    lab[((yy - cy) / ry) ** 2 + ((xx - cx) / rx) ** 2 < 1.0] = 2
    return lab


def maa_features(seed, hf, wf, noise, dim=384):
    """f32 [1, 1 + hf*wf, dim]: a [CLS] row, then one key per cell = the centre of the cell's region (maa_regions) +
    `noise` * N(0, 1).  Centres are N(0, 1), so keys of one region have cosine ~ 1 / (1 + noise^2) and keys of two
    regions ~ 0: noise 1.2 puts the two modes at 0.41 / 0 around tau = 0.2, noise 2.0 puts the upper mode ON tau."""
    g = _rng(seed)
    lab = maa_regions(hf, wf).reshape(-1)
    centers = g.standard_normal((4, dim))
    fe = centers[lab] + noise * g.standard_normal((hf * wf, dim))
    return np.concatenate([g.standard_normal((1, dim)), fe])[None].astype(np.float32)


def maa_masks(seed, hf, wf, M):
    """f32 [M,hf,wf], values in (0, 1): mask 0 aligned with regions 1 + 2 of maa_regions (~0.9 inside, ~0.1 outside), 1 a
    shifted copy of it, 2 uniform random, 3 constant; masks 4.. repeat the four kinds on other regions / shifts / draws /
    levels.  Levels and shifts come from the seed."""
    g = _rng(seed)
    lab = maa_regions(hf, wf)
    out = []
    for m in range(M):
        kind, rep = m % 4, m // 4
        hi, lo, level = 0.85 + 0.1 * g.random(), 0.05 + 0.1 * g.random(), g.uniform(0.3, 0.7)
        dy, dx = max(1, hf // 4) + int(g.integers(0, 3)), max(1, wf // 4) + int(g.integers(0, 3))
        inside = ((lab == 1) | (lab == 2)) if rep == 0 else (lab == 1 + rep % 3)
        if kind == 0:
            x = np.where(inside, hi, lo)
        elif kind == 1:
            x = np.roll(np.where((lab == 1) | (lab == 2), hi, lo), (dy, dx), axis=(0, 1))
        elif kind == 2:
            x = g.uniform(0.05, 0.95, size=(hf, wf))
        else:
            x = np.full((hf, wf), level)
        out.append(x)
    return np.stack(out).astype(np.float32)


class PatchFeatures(torch.nn.Module):
    """A stand-in for the DINO ViT with the one method the NCut heads call, get_last_qkv(imgs [B,3,H,W], which) ->
    [B, 1 + (H/8)(W/8), dim]: the mean colour of every 8x8 patch goes through a seeded random projection and a cosine
    (random Fourier features of a Gaussian kernel of width 1/scale in standardised colour units), plus a [CLS] row.
    Patches of one flat colour map to one point, patches of colours further apart than ~1/scale to nearly orthogonal
    ones: the Gram values of an image of flat regions are bimodal (~1 / ~0) around tau.  Plain torch, CPU or GPU: it is a
    test input, not a product path."""

    def __init__(self, seed=31, dim=384, patch_size=8, scale=3.0):
        super().__init__()
        g = _rng(seed)
        self.patch_size, self.embed_dim = patch_size, dim
        self.register_buffer("proj", torch.from_numpy((scale * g.standard_normal((dim, 3))).astype(np.float32)))
        self.register_buffer("phase", torch.from_numpy(g.uniform(0, 2 * np.pi, size=dim).astype(np.float32)))
        self.register_buffer("cls", torch.from_numpy(g.standard_normal(dim).astype(np.float32)))

    @torch.no_grad()
    def get_last_qkv(self, imgs, which="k"):
        assert which in ("q", "k", "v"), which
        c = torch.nn.functional.avg_pool2d(imgs.float(), self.patch_size)            # [B,3,hf,wf]
        c = c.flatten(2).transpose(1, 2)                                             # [B,n,3]
        f = torch.cos(c @ self.proj.T + self.phase)
        return torch.cat([self.cls.expand(c.shape[0], 1, -1), f], dim=1)


MAA_TREE = (("blackswan", 3, None), ("camel", 2, (240, 427)), ("dog", 3, None))   # (DAVIS val sequence, frames, export size)
MAA_TREE_CHANNELS, MAA_TREE_OBJECT = 3, 1


def _maa_frame(g, si, t):
    """u8 [480,854,3] frame of flat coloured rectangles with N(0, 2) noise, and the bool [480,854] object rectangle"""
    H, W = 480, 854
    bg = np.array([(60, 140, 70), (150, 130, 90), (70, 90, 160)][si], dtype=np.float32)
    obj = np.array([(220, 60, 50), (40, 60, 200), (230, 210, 60)][si], dtype=np.float32)
    other = np.array([(30, 30, 40), (240, 240, 235), (120, 30, 130)][si], dtype=np.float32)
    img = np.empty((H, W, 3), dtype=np.float32)
    img[:] = bg
    img[392:, :] = other                                            # a band that is neither object nor background
    y0, x0 = 96 + 16 * si, 150 + 120 * si + 40 * t                  # the object moves 40 px per frame
    m = np.zeros((H, W), dtype=bool)
    m[y0:y0 + 184, x0:x0 + 240] = True
    img[m] = obj
    img += g.normal(0, 2.0, size=img.shape).astype(np.float32)
    return np.clip(img + 0.5, 0, 255).astype(np.uint8), m


def maa_tree(root, seed=77, step=0):
    """A synthetic DAVIS tree for rcf_amd.maa under `root`: root/data/data_davis/JPEGImages/480p/{seq}/{frame:05}.jpg (real
    480x854 JPEGs of flat coloured regions with mild noise) and root/saved_eval_export/{channel}/pred_seg_{seq}_{frame}_
    {step:07}.png for 3 channels (RGB PNG; one sequence exported at 240x427, so the loader's resize runs).  Channel
    MAA_TREE_OBJECT is aligned with the coloured object in every frame (230 inside / 25 outside); channel 0 is the same
    rectangle shifted by half its size, channel 2 the complement of a copy shifted the other way.
    Returns (pretrain_dir, data_dir) = (root, root/data)."""
    import os
    from PIL import Image
    g = _rng(seed)
    images = os.path.join(root, "data", "data_davis", "JPEGImages", "480p")
    for ch in range(MAA_TREE_CHANNELS):
        os.makedirs(os.path.join(root, "saved_eval_export", str(ch)), exist_ok=True)
    for si, (seq, T, size) in enumerate(MAA_TREE):
        os.makedirs(os.path.join(images, seq), exist_ok=True)
        for t in range(T):
            fid = f"{t:05d}"
            img, m = _maa_frame(g, si, t)
            Image.fromarray(img).save(os.path.join(images, seq, fid + ".jpg"), quality=95)
            chans = (np.roll(m, (92, 120), axis=(0, 1)), m, ~np.roll(m, (-70, -160), axis=(0, 1)))
            for ch, cm in enumerate(chans):
                p = np.where(cm, 230, 25).astype(np.uint8)
                im = Image.fromarray(np.stack([p, p, p], -1))
                if size is not None:
                    im = im.resize((size[1], size[0]), resample=Image.NEAREST)
                im.save(os.path.join(root, "saved_eval_export", str(ch), f"pred_seg_{seq}_{fid}_{step:07}.png"))
    return root, os.path.join(root, "data")


# ---- SegTrackv2 / FBMS59 evaluation (rcf_amd.stv2_fbms) ---------------------------------------------------------------------
# (dataset, sequence, frames, export size, annotation size, prediction mode, annotation mode): both directions of the
# resize, one sequence with equal sizes, one with a single axis differing, one L export, one RGB annotation
STV2_FBMS_TREE = (
    ("SegTrackv2", "birdfall", 4, (48, 80), (97, 150), "RGB", "L"),        # enlargement, odd target
    ("SegTrackv2", "frog", 3, (120, 200), (45, 67), "RGB", "L"),           # reduction
    ("SegTrackv2", "worm", 5, (60, 90), (60, 90), "L", "L"),               # equal sizes, L export
    ("FBMS59", "cats01", 5, (64, 96), (64, 130), "RGB", "L"),              # one axis only
    ("FBMS59", "dogs02", 4, (50, 70), (121, 161), "RGB", "RGB"),           # enlargement, RGB annotation
    ("FBMS59", "marple7", 3, (90, 140), (40, 131), "RGB", "L"),            # reduction of one axis, mild one of the other
)
STV2_FBMS_LISTS = {"SegTrackv2": ("data_SegTrackv2", "trainval.txt"), "FBMS59": ("data_fbms59", "val_all.txt")}
STV2_FBMS_EMPTY = {("frog", 1), ("cats01", 3)}          # (sequence, frame): prediction and annotation both empty -> IoU nan
STV2_FBMS_UNANNOTATED = {("cats01", 1), ("dogs02", 0), ("dogs02", 2), ("marple7", 2)}   # FBMS59 frames without annotation


def _stv2_fbms_soft(g, H, W):
    """u8 [H,W]: a shallow cone around an ellipse with a sawtooth ripple -- most of the frame lies within a few grey levels of
    the evaluator's threshold (89 / 90), so one wrong rounding in the resize flips pixels.  Only + - * / sqrt and fmod: the
    same bytes on every machine."""
    yy, xx = np.meshgrid(np.arange(H, dtype=np.float64), np.arange(W, dtype=np.float64), indexing="ij")
    cy, cx = g.uniform(0.35, 0.65) * H, g.uniform(0.35, 0.65) * W
    ry, rx = g.uniform(0.2, 0.3) * H, g.uniform(0.2, 0.3) * W
    d = np.sqrt(((yy - cy) / ry) ** 2 + ((xx - cx) / rx) ** 2)
    period = g.uniform(5.0, 9.0)
    saw = np.abs(np.fmod(xx * g.uniform(0.6, 1.0) + yy * g.uniform(0.6, 1.0), period) / period - 0.5)
    v = 89.5 + 8.0 * (1.0 - d) + 9.0 * (saw - 0.25)
    return np.clip(np.floor(v + 0.5), 0, 255).astype(np.uint8), (cy, cx, ry, rx)


def stv2_fbms_tree(root, seed=59, step=0):
    """A synthetic tree for both datasets of rcf_amd.stv2_fbms under `root`, laid out as the reference's eval_tool.py reads it
    from its working directory: root/data/data_SegTrackv2/trainval.txt and root/data/data_fbms59/val_all.txt with lines
    `JPEGImages/<seq>/ 00000.jpg 00001.jpg ...`, annotations under .../Annotations/<seq>/ (u8 0 / 255; SegTrackv2 under the
    frame's own name -- a PNG stream whatever the name says, Pillow opens by content --, FBMS59 as .png and missing for the
    frames of STV2_FBMS_UNANNOTATED) and the exported masks root/pred/<dataset>/pred_seg_{seq}_{frame:05}_{step:07}.png.
    Returns (root/data, {dataset: prediction directory})."""
    import os
    from PIL import Image
    g = _rng(seed)
    data = os.path.join(root, "data")
    pred_dirs = {ds: os.path.join(root, "pred", ds) for ds in STV2_FBMS_LISTS}
    lines = {ds: [] for ds in STV2_FBMS_LISTS}
    for d in pred_dirs.values():
        os.makedirs(d, exist_ok=True)
    for ds, seq, T, (h, w), (H, W), pmode, amode in STV2_FBMS_TREE:
        ann_dir = os.path.join(data, STV2_FBMS_LISTS[ds][0], "Annotations", seq)
        os.makedirs(ann_dir, exist_ok=True)
        lines[ds].append(f"JPEGImages/{seq}/ " + " ".join(f"{t:05d}.jpg" for t in range(T)) + "\n")
        for t in range(T):
            p, (cy, cx, ry, rx) = _stv2_fbms_soft(g, h, w)
            yy, xx = np.meshgrid(np.arange(H, dtype=np.float64), np.arange(W, dtype=np.float64), indexing="ij")
            sy, sx = g.uniform(-0.1, 0.1) * H, g.uniform(-0.1, 0.1) * W           # the annotation: that ellipse, shifted
            a = (((yy - cy * H / h - sy) / (ry * H / h)) ** 2 + ((xx - cx * W / w - sx) / (rx * W / w)) ** 2 < 1.0)
            a = a.astype(np.uint8) * 255
            if (seq, t) in STV2_FBMS_EMPTY:
                p[:], a[:] = 0, 0
            pim = Image.fromarray(p if pmode == "L" else np.stack([p, p, p], -1))
            pim.save(os.path.join(pred_dirs[ds], f"pred_seg_{seq}_{t:05d}_{step:07}.png"))
            if ds == "FBMS59" and (seq, t) in STV2_FBMS_UNANNOTATED:
                continue
            aim = Image.fromarray(a if amode == "L" else np.stack([a, a // 2, 255 - a], -1))
            name = f"{t:05d}.png" if ds == "FBMS59" else f"{t:05d}.jpg"
            aim.save(os.path.join(ann_dir, name), format="PNG")
    for ds, (sub, name) in STV2_FBMS_LISTS.items():
        with open(os.path.join(data, sub, name), "w") as f:
            f.writelines(lines[ds])
    return data, pred_dirs


def fill_state_dict(shapes, seed=7, bn3_gamma=0.5, seg_scale=10.0):
    """Seeded weights for every entry of a state-dict `shapes` mapping name -> shape.

    conv/linear weights: He-normal(fan_out); BN gamma 1 (bn3: `bn3_gamma`, so residual branches
    are alive), beta 0, running stats (0,1); conv_seg scaled by `seg_scale` so the 4 mask logits
    separate (SURVEY §7 'bit-exact argmax' note).  Order of draws = sorted(names)."""
    g = _rng(seed)
    out = {}
    for name in sorted(shapes):
        shp = tuple(shapes[name])
        leaf = name.rsplit(".", 1)[-1]
        if leaf == "num_batches_tracked":
            out[name] = np.zeros((), dtype=np.int64)
        elif leaf == "running_mean":
            out[name] = np.zeros(shp, dtype=np.float32)
        elif leaf == "running_var":
            out[name] = np.ones(shp, dtype=np.float32)
        elif len(shp) == 1 and leaf == "weight":            # BN gamma
            gamma = bn3_gamma if name.split(".")[-2] == "bn3" else 1.0
            out[name] = np.full(shp, gamma, dtype=np.float32)
        elif len(shp) == 1 and leaf == "bias":
            is_bn = (name[:-len("bias")] + "running_mean") in shapes
            out[name] = np.zeros(shp, dtype=np.float32) if is_bn else \
                g.normal(0, 0.01, size=shp).astype(np.float32)
        else:                                               # conv weight [Co,Ci,(k,k)|(k)]
            fan_out = shp[0] * int(np.prod(shp[2:]))
            w = g.normal(0, np.sqrt(2.0 / fan_out), size=shp).astype(np.float32)
            if "conv_seg" in name:
                w *= seg_scale
            out[name] = w
    return out


def fill_vit_state_dict(shapes, seed=21):
    """Seeded weights for the DINO ViT parity fixtures (no checkpoint can be downloaded): N(0, 0.05) matrices,
    N(0, 0.02) biases / tokens, LayerNorm scale 1 + N(0, 0.1).  Same generator on both sides of every comparison."""
    g = np.random.Generator(np.random.PCG64(seed))
    out = {}
    for k, shp in shapes.items():
        if "norm" in k and k.endswith("weight"):
            out[k] = (1.0 + 0.1 * g.standard_normal(shp)).astype(np.float32)
        elif k.endswith("bias") or k in ("cls_token", "pos_embed"):
            out[k] = (0.02 * g.standard_normal(shp)).astype(np.float32)
        else:
            out[k] = (0.05 * g.standard_normal(shp)).astype(np.float32)
    return out


def grad_sketch(named_grads, k=8):
    """A small linear fingerprint of a set of gradient tensors: per tensor, k sums of its elements under pseudo-random +-1
    sign patterns (a hash of the element index: the same pattern on every device and in every process).  E[(s - t)^2] of two
    sketches is the squared distance of the tensors they came from, so |sketch(g) - sketch(truth)| / |sketch(truth)| over a
    module's tensors estimates the relative VECTOR error of the module's gradient from a few kilobytes of fixture instead of
    100 MB of float64 gradients (tools/oracle_b8_selfdev.py, tests/test_model_gpu.py::test_fullsize_b8_gradients_vs_oracle).
    named_grads: {name: torch tensor}; returns {name: [k floats]}."""
    import torch
    out = {}
    for name, g in named_grads.items():
        v = g.detach().reshape(-1).double()
        idx = torch.arange(v.numel(), device=v.device, dtype=torch.int64)
        row = []
        for j in range(k):
            h = idx * (2654435761 + 81006 * j) + 2654435769 * (j + 1)
            h = (h ^ (h >> 15)) * 2246822519
            h = h ^ (h >> 13)
            sign = 1.0 - 2.0 * ((h >> 7) & 1).double()
            row.append(float((sign * v).sum()))
        out[name] = row
    return out


def sketch_error(sketch, truth, prefix=None):
    """relative distance of two grad_sketch() results over the tensors whose name starts with `prefix` (None: all)"""
    num = den = 0.0
    for name, t in truth.items():
        if prefix is not None and not name.startswith(prefix):
            continue
        s = sketch[name]
        num += sum((a - b) ** 2 for a, b in zip(s, t))
        den += sum(b ** 2 for b in t)
    return (num / den) ** 0.5 if den > 0 else 0.0
