"""Edge-shape cases of the warp, occlusion and photometric kernels (csrc/warp.hip) and their reference.

Shared by tests/test_warp_sweep_cpu.py (the restatement agrees with oracle/rcf_torch.py in float64; the oracle's float32 run sits
inside every bound; the 3-operation division is float32's own; the tables reach the dispatch and geometry branches they name) and
tests/test_warp_sweep_gpu.py (the kernels against the restatement).  numpy / torch on the CPU; nothing of the HIP package enters.

The sample position is computed exactly as utils/warp_utils.py, torch's grid_sample and both kernel families compute it, in
FLOAT32 and in this order (`sample_pos`):  p = float32(index) + flow;  g = 2 p / (size - 1) - 1;  i = ((g + 1) / 2) (size - 1);
in border mode i -> 0 where !(i > 0) (NaN included), i -> size - 1 where i >= size - 1.  numpy's float32 arithmetic is IEEE (and
the library is compiled without contraction), so floors, clips and tap choices are the decisions the kernels make.  Everything
after the position is float64, written out tap by tap: weights 1 - w and w of the fractional part, blends, the scatter of the
backward (np.bincount), sums.  With every result comes its MASS, the sum of the absolute values of the terms added into it; the
bounds are per element against that mass.  `pdt=np.float64` runs the position in float64 too: that form is what the oracle's
float64 run computes and exists only to be compared with it.

Non-finite flows.  In zeros mode torch's CPU grid_sample converts the floor of an inf / NaN position to an index unchecked --
undefined behaviour: a segmentation fault has been seen, another run returned NaN pixels -- so non-finite flows appear in BORDER
mode only, and there the restatement alone defines the answer: the clip above (+inf and an overflowing 2 p to size - 1, -inf and
NaN to 0), gradient 0 on the clipped coordinate.

Bounds, u = 2^-24 (`U`):  warped pixel and dflow 16 u mass (the kernels round at most 7 times per term; 16 is the constant of the
resize sweep);  dx (16 + n) u mass with n the non-zero contributions to the element, in any order;  the fused L1 sum: the sum
over the pixels of  16 u occ (|target| + mass of the warped value) summed over channels  (the warped value's roundings, one for
the difference, C for the channel sum, one for the mask product; the fp64 accumulation adds 1e-16 relative).  Masks: equal outside
the TIE set -- a float64 splat count within 1e-4 of th, a bidirectional margin within 1e-4 of the sum of its two sides.

`tile_plan`, `l1_plan`, `pixel_plan` restate the launch geometry of csrc/warp.hip to CHOOSE cases and to assert what the table
reaches -- never as a reference for a value.
"""
import dataclasses
import functools
import math

import numpy as np
import torch

U = 2.0 ** -24
TIE = 1e-4
PHOTO_RTOL = 1e-4                                    # the suite's limit on the photometric loss (tests/test_kernels_gpu.py)
PX_TRIP = 16384 * 256                                # px_blocks: pixels one trip of the backward / splat / threshold / bidirectional loops covers
PHOTO_TRIP = 2048 * 256
f32 = np.float32


# ====================================================================================================== the sample position
def sample_pos(p, size, border, pdt=np.float32):
    """p: positions index + flow, already of type pdt.  -> (i, live): the un-normalised (and, in border mode, clipped) coordinate and
    whether the gradient with respect to it survives the clip"""
    d = pdt(size - 1)
    with np.errstate(all="ignore"):
        g = pdt(2) * p / d - pdt(1)
        i = ((g + pdt(1)) / pdt(2)) * d
    assert i.dtype == pdt
    live = np.ones(i.shape, dtype=bool)
    if border:
        lo = ~(i > 0)
        hi = ~lo & (i >= d)
        i = np.where(lo, pdt(0), np.where(hi, d, i))
        live = ~(lo | hi)
    return i, live


def positions(flow, pdt=np.float32, rows=None):
    """flow [B, 2, H, W] -> (px, py) [B, H, W] of type pdt: index + flow in pdt.  `rows`: the image rows that flow holds (default all)"""
    B, _, H, W = flow.shape
    rows = np.arange(H) if rows is None else np.asarray(rows)
    xs, ys = np.arange(W, dtype=pdt)[None, None, :], rows.astype(pdt)[None, :, None]
    with np.errstate(all="ignore"):
        return xs + flow[:, 0].astype(pdt), ys + flow[:, 1].astype(pdt)


@dataclasses.dataclass
class Taps:
    idx: np.ndarray          # [4, B, H, W] int64: y W + x of taps (y0, x0), (y0, x0+1), (y0+1, x0), (y0+1, x0+1); 0 where invalid
    w: np.ndarray            # [4, B, H, W] float64 weights
    ok: np.ndarray           # [4, B, H, W] tap inside the image
    wx: np.ndarray           # [B, H, W] float64 fractional parts
    wy: np.ndarray
    live_x: np.ndarray
    live_y: np.ndarray


def make_taps(flow, pad, pdt=np.float32, rows=None, H=None):
    """taps of the pixels flow holds: the whole [B, 2, H, W] field, or its `rows` of an image H high"""
    B, _, _, W = flow.shape
    H = flow.shape[2] if H is None else H
    px, py = positions(flow, pdt, rows)
    ix, lx = sample_pos(px, W, pad == "border", pdt)
    iy, ly = sample_pos(py, H, pad == "border", pdt)
    assert np.isfinite(ix).all() and np.isfinite(iy).all(), "non-finite positions are defined in border mode only"
    fx, fy = np.floor(ix), np.floor(iy)
    wx, wy = ix.astype(np.float64) - fx.astype(np.float64), iy.astype(np.float64) - fy.astype(np.float64)
    x0, y0 = np.clip(fx, -2, W + 1).astype(np.int64), np.clip(fy, -2, H + 1).astype(np.int64)
    idx, w, ok = [], [], []
    for dy in (0, 1):
        for dx in (0, 1):
            xx, yy = x0 + dx, y0 + dy
            v = (xx >= 0) & (xx < W) & (yy >= 0) & (yy < H)
            idx.append(np.where(v, yy * W + xx, 0))
            w.append((wy if dy else 1 - wy) * (wx if dx else 1 - wx))
            ok.append(v)
    return Taps(np.stack(idx), np.stack(w), np.stack(ok), wx, wy, lx, ly)


def _gather(x, t):
    """x [B, C, H, W] float64 -> the four tap values [4, B, C, H, W], 0 where the tap is outside"""
    B, C, H, W = x.shape
    flat = x.reshape(B, C, H * W)
    n = t.idx.shape[2]
    out = []
    for k in range(4):
        v = np.take_along_axis(flat, np.broadcast_to(t.idx[k].reshape(B, 1, n * W), (B, C, n * W)), axis=2).reshape(B, C, n, W)
        out.append(np.where(t.ok[k][:, None], v, 0.0))
    return np.stack(out)


# ================================================================================================================= forward
def warp_ref(x, flow, pad, pdt=np.float32, rows=None):
    """x [B, C, H, W], flow [B, 2, H, W] (numpy) -> (warped, mass) float64 [B, C, H, W]; with `rows`, of those output rows only"""
    t = make_taps(flow if rows is None else flow[:, :, rows], pad, pdt, rows, x.shape[2])
    v = _gather(x.astype(np.float64), t)
    w = (t.w * t.ok)[:, :, None]
    return (w * v).sum(0), (np.abs(w) * np.abs(v)).sum(0)


# ================================================================================================================ backward
def warp_bwd_ref(x, flow, dout, pad, pdt=np.float32, rows=None):
    """-> dx, dx_mass [B, C, H, W], n [B, H, W] (non-zero contributions per element), dflow, dflow_mass [B, 2, H, W].  With `rows`:
    the part of the backward that the output pixels of those rows contribute (dx: their terms alone; dflow: those rows)"""
    B, C, H, W = x.shape
    sub = (lambda a: a) if rows is None else (lambda a: a[:, :, rows])
    t = make_taps(sub(flow), pad, pdt, rows, H)
    g = sub(dout).astype(np.float64)
    v = _gather(x.astype(np.float64), t)
    dx, mass, n = np.zeros((B, C, H * W)), np.zeros((B, C, H * W)), np.zeros((B, H * W), dtype=np.int64)
    for b in range(B):
        for k in range(4):
            sel = t.ok[k, b].reshape(-1)
            at = t.idx[k, b].reshape(-1)[sel]
            wk = t.w[k, b].reshape(-1)[sel]
            n[b] += np.bincount(at, weights=(wk != 0).astype(np.float64), minlength=H * W).astype(np.int64)
            for c in range(C):
                term = g[b, c].reshape(-1)[sel] * wk
                dx[b, c] += np.bincount(at, weights=term, minlength=H * W)
                mass[b, c] += np.bincount(at, weights=np.abs(term), minlength=H * W)
    v00, v01, v10, v11 = v
    a = np.abs(v)
    wx, wy = t.wx[:, None], t.wy[:, None]
    gx = (g * ((1 - wy) * (v01 - v00) + wy * (v11 - v10))).sum(1)
    gy = (g * ((1 - wx) * (v10 - v00) + wx * (v11 - v01))).sum(1)
    mx = (np.abs(g) * ((1 - wy) * (a[1] + a[0]) + wy * (a[3] + a[2]))).sum(1)
    my = (np.abs(g) * ((1 - wx) * (a[2] + a[0]) + wx * (a[3] + a[1]))).sum(1)
    dflow = np.stack([np.where(t.live_x, gx, 0.0), np.where(t.live_y, gy, 0.0)], 1)
    fmass = np.stack([np.where(t.live_x, mx, 0.0), np.where(t.live_y, my, 0.0)], 1)
    return dx.reshape(B, C, H, W), mass.reshape(B, C, H, W), n.reshape(B, H, W), dflow, fmass


# ============================================================================================================ forward splat
def splat_ref(flow, pdt=np.float32, rows=None):
    """utils/warp_utils.py:27-81: the four bilinear weights of every pixel's target splatted forward, corners that a clamp into the
    image moves dropped.  -> count [B, H, W] float64 (with `rows`: what the pixels of those rows splat)"""
    B, _, H, W = flow.shape
    x, y = positions(flow if rows is None else flow[:, :, rows], pdt, rows)
    assert np.isfinite(x).all() and np.isfinite(y).all()
    x1, y1 = np.floor(x), np.floor(y)
    x0, y0 = x1 + 1, y1 + 1
    xf, yf, xc, yc = np.clip(x1, 0, W - 1), np.clip(y1, 0, H - 1), np.clip(x0, 0, W - 1), np.clip(y0, 0, H - 1)
    xco, yco, xfo, yfo = x0 != xc, y0 != yc, x1 != xf, y1 != yf
    x64, y64 = x.astype(np.float64), y.astype(np.float64)
    cnt = np.zeros((B, H * W))
    for xs, ys, bad in ((xc, yc, xco | yco), (xc, yf, xco | yfo), (xf, yc, xfo | yco), (xf, yf, xfo | yfo)):
        val = (1 - np.abs(x64 - xs)) * (1 - np.abs(y64 - ys))
        at = (ys.astype(np.int64) * W + xs.astype(np.int64))
        for b in range(B):
            keep = ~bad[b].reshape(-1)
            cnt[b] += np.bincount(at[b].reshape(-1)[keep], weights=val[b].reshape(-1)[keep], minlength=H * W)
    return cnt.reshape(B, H, W)


def occ_backward_ref(flow21, th=0.2, pdt=np.float32, rows=None):
    """-> (mask [B, 1, H, W] float64 of 0 / 1, tie [B, 1, H, W] bool)"""
    cnt = splat_ref(flow21, pdt, rows)[:, None]
    th = float(f32(th))
    return (np.clip(cnt, 0, 1) < th).astype(np.float64), np.abs(cnt - th) <= TIE


def occ_bidir_ref(f12, f21, scale=0.01, bias=0.5, pdt=np.float32, rows=None):
    """utils/warp_utils.py:97-104 with f21 sampled in zeros mode.  -> (mask, tie) [B, 1, H, W] (with `rows`: of those rows)"""
    w, _ = warp_ref(f21, f12, "zeros", pdt, rows)
    a = (f12 if rows is None else f12[:, :, rows]).astype(np.float64)
    d = a + w
    lhs = (d * d).sum(1, keepdims=True)
    rhs = float(f32(scale)) * ((a * a).sum(1, keepdims=True) + (w * w).sum(1, keepdims=True)) + float(f32(bias))
    return (lhs > rhs).astype(np.float64), np.abs(lhs - rhs) <= TIE * (lhs + rhs)


# ============================================================================================================== fused L1
def l1_pair_ref(im1, im2, flow, occ, pad, pdt=np.float32):
    """-> (sum of occ sum_c |im1 - warp(im2)|, sum of occ, bound on the first)"""
    w, mass = warp_ref(im2, flow, pad, pdt)
    t = im1.astype(np.float64)
    o = np.ones((im1.shape[0], 1) + im1.shape[2:]) if occ is None else occ.astype(np.float64)
    s = (np.abs(t - w).sum(1, keepdims=True) * o).sum()
    bound = 16 * U * ((np.abs(t) + mass).sum(1, keepdims=True) * np.abs(o)).sum()
    return float(s), float(o.sum()), float(bound)


# =========================================================================================================== photometric
def _box3(a):
    """mean over the 3 x 3 window of every interior pixel: [B, C, H - 2, W - 2]"""
    H, W = a.shape[2:]
    s = np.zeros(a.shape[:2] + (H - 2, W - 2))
    for dy in range(3):
        for dx in range(3):
            s = s + a[:, :, dy:dy + H - 2, dx:dx + W - 2]
    return s / 9.0


def photometric_ref(im, recon, occ, w_l1=0.15, w_ssim=0.85, dt=np.float64):
    """models/amd/flow_loss.py:15-29: [w_l1 mean(|im - recon| occ) + w_ssim mean(SSIM distance of recon occ, im occ over the interior
    pixels)] / mean(occ), a weight of zero dropping its term"""
    im, recon, occ = im.astype(dt), recon.astype(dt), occ.astype(dt)
    loss = dt(0)
    with np.errstate(all="ignore"):
        if w_l1 > 0:
            loss = loss + dt(w_l1) * (np.abs(im - recon) * occ).mean(dtype=dt)
        if w_ssim > 0:
            x, y = recon * occ, im * occ
            mx, my = _box3(x), _box3(y)
            sx, sy, sxy = _box3(x * x) - mx * mx, _box3(y * y) - my * my, _box3(x * y) - mx * my
            n = (2 * mx * my + 0.01 ** 2) * (2 * sxy + 0.03 ** 2)
            d = (mx * mx + my * my + 0.01 ** 2) * (sx + sy + 0.03 ** 2)
            loss = loss + dt(w_ssim) * np.clip((1 - n / d) / 2, 0, 1).mean(dtype=dt)
        return float(loss / occ.mean(dtype=dt))


# ================================================================================================================ margins
def elem_margin(got, ref, bound):
    """worst |got - ref| / bound over the elements; an error under a zero bound, or a NaN anywhere, gives inf"""
    got, ref = np.asarray(got, dtype=np.float64), np.asarray(ref, dtype=np.float64)
    d = np.abs(got - ref)
    if np.isnan(d).any():
        return float("inf")
    if not d.size:
        return 0.0
    with np.errstate(all="ignore"):
        r = np.where(d == 0, 0.0, d / bound)
    return float(r.max())


def warp_bound(mass):
    return 16 * U * mass


def dx_bound(mass, n):
    return (16 + n[:, None].astype(np.float64)) * U * mass


def mask_mismatch(got, ref, tie):
    """number of pixels outside the tie set on which the masks differ"""
    return int(((np.asarray(got, dtype=np.float64) != ref) & ~tie).sum())


# ========================================================================================== the division of the tile kernels
def fma32(a, b, c):
    """float32 fma(a, b, c), rounded once: the product of two float32 is exact in float64; the float64 sum is turned into a
    round-to-odd one with the error term of TwoSum, after which the rounding to float32 is the rounding of the exact value"""
    prod = np.asarray(a, dtype=np.float32).astype(np.float64) * np.asarray(b, dtype=np.float32).astype(np.float64)
    c = np.broadcast_to(np.asarray(c, dtype=np.float32).astype(np.float64), prod.shape)
    s = prod + c
    bb = s - prod
    err = (prod - (s - bb)) + (c - bb)
    bits = s.view(np.int64).copy()
    nudge = (err != 0) & ((bits & 1) == 0)
    away = (err > 0) == (s > 0)                                    # the exact value lies further from zero than s
    bits = np.where(nudge, bits + np.where(away, 1, -1), bits)
    return bits.view(np.float64).astype(np.float32)


def div3(t, d):
    """q = t r; q += fma(-q, d, t) r with r = float32(1) / d: the tile kernels' t / d, float32 in and out"""
    t, d = np.asarray(t, dtype=np.float32), f32(d)
    r = f32(1) / d
    q = t * r
    assert q.dtype == np.float32
    return fma32(fma32(-q, d, t), r, q)


# ================================================================================================= launch geometry restated
def cdiv(a, b):
    return -(-a // b)


def tile_applies(C, H, W, pad):
    return C == 3 and pad == "border" and W >= 2 and H >= 2


def warp_kernel(C, H, W, pad):
    """which kernel rcf_flow_warp_f32 launches"""
    return "rows" if tile_applies(C, H, W, pad) and W >= 256 else "pixel"


def l1_kernel(C, H, W, pad):
    if not tile_applies(C, H, W, pad):
        return "pixel"
    return "rows2" if W % 2 == 0 else "rows"


def tile_plan(B, H, W, tile_w, tile_h, Q_of):
    """the XCD shares of a tile kernel: Q workgroups per XCD, per-XCD tile counts, the largest number of loop trips"""
    tx, ty = cdiv(W, tile_w), cdiv(H, tile_h)
    n = tx * ty
    R = B * cdiv(n, 8)
    Q = Q_of(R)
    per = [n * (k + 1) // 8 - n * k // 8 for k in range(8)]
    return dict(tx=tx, ty=ty, Q=Q, per=per, trips=max(cdiv(B * p, Q) for p in per))


def warp_tile_plan(B, H, W):
    return tile_plan(B, H, W, 64, 16, lambda R: min(R, 1024))


def l1_tile_plan(B, H, W):
    two = W % 2 == 0
    return tile_plan(B, H, W, 128 if two else 64, 8 if two else 16, lambda R: 1 if R < 4 else min(R // 4, 512))


def pixel_plan(B, H, W):
    """band_map: rows per band, pixels per band, 512-pixel runs per band; the fused L1's Q and trips"""
    rb = (H + 7) >> 3
    rows = [min(min(k * rb, H) + rb, H) - min(k * rb, H) for k in range(8)]
    runs = cdiv(rb * W, 512)
    Q = min(B * runs, 256)
    return dict(rb=rb, rows=rows, band_px=[r * W for r in rows], runs=runs, Q=Q, trips=cdiv(B * runs, Q))


def px_blocks(total):
    return max(1, min(cdiv(total, 256), 16384))


# =================================================================================================================== cases
FINITE_FLOWS = ("gauss", "integer", "half", "edges", "far")
BORDER_ONLY_FLOWS = ("nan", "inf", "huge", "denorm")           # flows torch's zeros mode cannot take
SHAPES_MIN = [(2, 2)]
SHAPES_SEAMS = [(2, 3), (9, 70), (17, 200), (7, 9)]
SHAPES_TILE = [(2, 256), (16, 256), (17, 257), (33, 300)]      # W >= 256: flow_warp's tile kernel; 16 x 256 runs with B = 1
SHAPES_L1 = [(9, 130), (8, 128), (17, 65), (3, 2)]
FLOW_SHAPES = [(9, 70), (17, 257)]


@dataclasses.dataclass(frozen=True)
class Case:
    H: int
    W: int
    C: int = 3
    B: int = 2
    flow: str = "gauss"

    @property
    def name(self):
        return f"{self.H}x{self.W}-c{self.C}-b{self.B}-{self.flow}"

    @property
    def pads(self):
        return ("border",) if self.flow in BORDER_ONLY_FLOWS else ("border", "zeros")

    @property
    def seed(self):
        return 1000 * self.H + 10 * self.W + self.C + 7 * (FINITE_FLOWS + BORDER_ONLY_FLOWS).index(self.flow)


def _cases():
    out = [Case(H, W, B=1 if (H, W) == (16, 256) else 2) for H, W in SHAPES_MIN + SHAPES_SEAMS + SHAPES_TILE + SHAPES_L1]
    out += [Case(9, 70, C=c) for c in (1, 2, 4)]
    out += [Case(H, W, flow=f) for H, W in FLOW_SHAPES for f in FINITE_FLOWS[1:] + BORDER_ONLY_FLOWS]
    return out


CASES = _cases()
MASK_CASES = [c for c in CASES if c.C == 3 and c.flow in FINITE_FLOWS]                       # the masks take finite flows only
BIG_PX = (1, 1, 2049, 2048)                          # backward, splat, threshold, bidirectional: just past 16384 x 256 pixels
BIG_PX_TAIL, BIG_PX_REACH = 48, 24                   # ... checked on the pixels of the last 48 rows; no flow there reaches 24 rows
BIG_PHOTO = (1, 1, 725, 725)                         # photometric: just past 2048 x 256 pixels
BIG_TILE = (1, 3, 26209, 257)                        # flow_warp's tile kernel: 5 x 1639 = 8195 tiles > 8 x 1024
L1_MANY = (300, 2, 2)                                # B, H, W: 300 one-run images, warp_l1_kernel's Q = 256 workgroups per band take a second trip
PHOTO_CASES = [                                      # name, B, C, H, W, mask kind, im == recon, w_l1, w_ssim
    ("one_interior", 2, 3, 3, 3, "random", False, 0.15, 0.85),
    ("4x5", 2, 3, 4, 5, "random", False, 0.15, 0.85),
    ("patches", 2, 3, 13, 21, "patches", False, 0.15, 0.85),
    ("ones_c1", 2, 1, 9, 70, "ones", False, 0.15, 0.85),
    ("same", 2, 3, 13, 21, "random", True, 0.15, 0.85),
    ("no_l1", 2, 3, 13, 21, "random", False, 0.0, 0.85),
    ("no_ssim", 2, 3, 13, 21, "random", False, 0.15, 0.0),
    ("zero_mask", 2, 3, 7, 9, "zeros", False, 0.15, 0.85),
]


def make_flow(c, g):
    """float32 numpy [B, 2, H, W] of kind c.flow; the special kinds are planted into a Gaussian sigma = 2.5 field"""
    B, H, W = c.B, c.H, c.W
    fl = (torch.randn(B, 2, H, W, generator=g) * 2.5).numpy()
    ys, xs = np.arange(H, dtype=np.float32)[:, None], np.arange(W, dtype=np.float32)[None, :]
    k = torch.rand(B, H, W, generator=g).numpy()
    if c.flow == "integer":
        fl = np.round(fl)
    elif c.flow == "half":
        fl = np.floor(fl) + f32(0.5)
    elif c.flow == "edges":                                        # positions exactly on 0, size - 1, -1 and size, each axis on its own
        pick = lambda n, size: np.choose(n % 4, [0, size - 1, -1, size]).astype(np.float32)
        n = np.arange(H * W).reshape(H, W)
        fl[0, 0], fl[0, 1] = pick(n, W) - xs, pick(n // 4, H) - ys
        fl[1, 0] = np.where(k[1] < 0.5, pick(n // 2, W) - xs, fl[1, 0])          # an edge on one axis, a Gaussian on the other
        fl[1, 1] = np.where(k[1] >= 0.5, pick(n, H) - ys, fl[1, 1])
    elif c.flow != "gauss":
        hi, lo = {"far": (1e9, -1e9), "nan": (math.nan, math.nan), "inf": (math.inf, -math.inf), "huge": (3e38, -3e38),
                  "denorm": (1e-40, -1e-40)}[c.flow]
        # a quarter of the pixels: x alone, y alone, both; the first rows / columns and the last ones included
        fl[:, 0] = np.where(k < 0.08, f32(hi), np.where(k < 0.16, f32(lo), fl[:, 0]))
        fl[:, 1] = np.where((k >= 0.12) & (k < 0.2), f32(hi), np.where((k >= 0.2) & (k < 0.28), f32(lo), fl[:, 1]))
        fl[0, :, 0, 0], fl[0, :, -1, -1], fl[1, :, 0, -1], fl[1, :, -1, 0] = hi, lo, hi, lo
        if c.flow == "denorm":                                     # alone on the axis: index + 1e-40 is the index, except at index 0
            fl[0, :, :, 0], fl[0, :, 0, :] = hi, hi
    return np.ascontiguousarray(fl, dtype=np.float32)


def smooth_flow(B, H, W, g, amp_y=3.5):
    """a plane wave per image and component, amplitude 3.5 (sigma 2.5), at least 64 pixels long, under white noise of 0.2: a flow
    whose backward warp by itself nearly undoes it, so that the bidirectional check has something to decide"""
    y, x = torch.arange(H).double()[:, None], torch.arange(W).double()[None, :]
    ph = 6.283 * torch.rand(B, 2, 1, 1, generator=g).double()
    amp = torch.tensor([min(3.5, 0.4 * (W - 1)), min(amp_y, 0.4 * (H - 1))]).double().view(1, 2, 1, 1)      # a thin image keeps its samples inside
    f = amp * torch.sin(6.283 * (x / max(2 * W, 64) + y / max(2 * H, 64))[None, None] + ph)
    return (f + 0.2 * torch.randn(B, 2, H, W, generator=g).double()).float().numpy()


@functools.lru_cache(maxsize=4)
def inputs(c):
    """x, y [B, C, H, W] uniform images, flow f12, dout, a 0 / 1 mask with 30 % zeros; for the occlusion masks m12 (f12 itself, but
    on the Gaussian cases a smooth flow of the same sigma) and f21 = -(m12 warped by m12) + noise of 0.6.  Two independent
    Gaussian flows, and white noise warped by itself, leave 96 % of the bidirectional mask occluded, which tests nothing.
    float32 numpy; callers leave them unchanged."""
    g = torch.Generator().manual_seed(c.seed)
    B, C, H, W = c.B, c.C, c.H, c.W
    x, y = torch.rand(B, C, H, W, generator=g).numpy(), torch.rand(B, C, H, W, generator=g).numpy()
    f12 = make_flow(c, g)
    dout = torch.randn(B, C, H, W, generator=g).numpy()
    occ = (torch.rand(B, 1, H, W, generator=g) > 0.3).float().numpy()
    m12 = f21 = None
    if c.flow in FINITE_FLOWS:
        m12 = smooth_flow(B, H, W, g) if c.flow == "gauss" else f12
        back, _ = warp_ref(m12, m12, "zeros")
        f21 = (-back + 0.6 * torch.randn(B, 2, H, W, generator=g).numpy()).astype(np.float32)
    return dict(x=x, y=y, f12=f12, dout=dout, occ=occ, m12=m12, f21=f21)


@functools.lru_cache(maxsize=4)
def warp_truth(c, pad):
    d = inputs(c)
    return warp_ref(d["x"], d["f12"], pad)


@functools.lru_cache(maxsize=2)
def bwd_truth(c, pad):
    d = inputs(c)
    return warp_bwd_ref(d["x"], d["f12"], d["dout"], pad)


def photo_inputs(name):
    _, B, C, H, W, kind, same, w1, ws = next(p for p in PHOTO_CASES if p[0] == name)
    g = torch.Generator().manual_seed(100 * H + W + len(name))
    im = torch.rand(B, C, H, W, generator=g).numpy()
    rec = im.copy() if same else np.clip(im + 0.1 * torch.randn(B, C, H, W, generator=g).numpy(), 0, 1).astype(np.float32)
    occ = (torch.rand(B, 1, H, W, generator=g) > 0.3).float().numpy()
    if kind == "patches":
        occ[:, :, 2:7, 3:9] = 0                                    # whole windows of zeros inside, and a zero corner
        occ[:, :, -3:, -4:] = 0
    if kind == "ones":
        occ[:] = 1
    if kind == "zeros":
        occ[:] = 0
    return im, rec, occ, w1, ws


def big_flow(B, H, W, seed):
    """a smooth-ish sigma = 2.5 flow for the second-trip cases, float32 numpy"""
    g = torch.Generator().manual_seed(seed)
    return (torch.randn(B, 2, H, W, generator=g) * 2.5).numpy()


def big_photo_inputs():
    B, C, H, W = BIG_PHOTO
    g = torch.Generator().manual_seed(725)
    im = torch.rand(B, C, H, W, generator=g).numpy()
    rec = np.clip(im + 0.1 * torch.randn(B, C, H, W, generator=g).numpy(), 0, 1).astype(np.float32)
    occ = (torch.rand(B, 1, H, W, generator=g) > 0.3).float().numpy()
    return im, rec, occ
