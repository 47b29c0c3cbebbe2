"""What the export tests share (tests/test_export_cpu.py, tests/test_export_gpu.py, tools/time_export.py): a numpy restatement of the
panel arithmetic as include/rcf_hip.h states it for rcf_export_panels_u8, the case list and the comparison rule.

levels(plane, size, align, T): the level t = v 255 + 0.5 before the clamp, with the expression tree of csrc/resize_pos.h -- the
float32 source position of an output index, its two taps and weights, the blend hy (hx v00 + lx v01) + ly (hx v10 + lx v11) -- and
then, for a frame, (v + 2) / 4.  T = float32 is the kernel's arithmetic, every step rounded once.  T = float64 is the yardstick: the
SAME float32 source positions and weights (they define which resize is meant), everything from the blend on in float64.

The rule (random cases).  byte = floor(clamp(level)).  A byte may differ from the float64 byte by at most one level, and only where
the float64 level lies within EPS = 8 2^-24 255 of an integer; at most CAP = 1e-3 of a case's elements may take that exemption.  The 8:
in units of 2^-24 of a value in [0, 1], the blend's products and sums weigh to at most 4 roundings (the weights of a level sum to
1), x 255 is one and + 0.5 is one; a frame in [-2, 2] is at half a unit per blend rounding after its / 4 (exact) and adds one for
+ 2.  The random masks are softmax of 3 N(0, 1) logits with C = 5, which keeps the float64 levels' share within EPS of an integer at
NEAR_SHARE = 3.1e-4 or less (tests/test_export_cpu.py asserts it for every case); constants and ties are judged by bit-equality with
the torch route alone, since a level that sits ON an integer in exact arithmetic may fall either way.
"""
import collections

import numpy as np

EPS = 8 * 2.0 ** -24 * 255.0
CAP = 1e-3
NEAR_SHARE = 3.1e-4
F32 = np.float32


def host_scale(n_in, n_out, align):
    if align:
        return F32(n_in - 1) / F32(n_out - 1) if n_out > 1 else F32(0)
    return F32(n_in) / F32(n_out)


def src_index(n_out, n_in, align):
    """(i0, i1, l1) of every output index: int32, int32, float32 -- csrc/resize_pos.h src_index in float32"""
    dst = np.arange(n_out).astype(F32)
    scale = host_scale(n_in, n_out, align)
    s = scale * dst if align else np.maximum(scale * (dst + F32(0.5)) - F32(0.5), F32(0))
    assert s.dtype == F32
    i0 = np.minimum(s.astype(np.int32), n_in - 1)
    i1 = i0 + (i0 < n_in - 1)
    return i0, i1.astype(np.int32), (s - i0.astype(F32)).astype(F32)


def levels(plane, size, align, T=F32, frame=False):
    """plane [h, w] float32 -> level [Ho, Wo] in T (before the clamp)"""
    assert plane.dtype == F32 and plane.ndim == 2
    y0, y1, ly = src_index(size[0], plane.shape[0], align)
    x0, x1, lx = src_index(size[1], plane.shape[1], align)
    hy, hx = (F32(1) - ly).astype(T)[:, None], (F32(1) - lx).astype(T)[None, :]
    ly, lx = ly.astype(T)[:, None], lx.astype(T)[None, :]
    p = plane.astype(T)
    with np.errstate(all="ignore"):
        v = hy * (hx * p[y0][:, x0] + lx * p[y0][:, x1]) + ly * (hx * p[y1][:, x0] + lx * p[y1][:, x1])
        if frame:
            v = (v + T(2)) / T(4)
        t = v * T(255)
        t = t + T(0.5)
    assert t.dtype == T
    return t


def to_bytes(level):
    """NaN -> 0, clamp to [0, 255], truncate"""
    with np.errstate(all="ignore"):
        t = np.where(np.isnan(level), 0, np.clip(level, 0, 255))
    return np.floor(t).astype(np.uint8)


def panel_bytes(plane, size, align, frame=False):
    return to_bytes(levels(plane, size, align, F32, frame))


def near_integer(level64):
    return np.abs(level64 - np.round(level64)) <= EPS


def judge(got, level64):
    """(worst |difference| in levels, exemptions taken, elements, differences outside the exemption) of bytes against float64 levels"""
    want = to_bytes(level64).astype(np.int32)
    d = np.abs(got.astype(np.int32) - want)
    return int(d.max(initial=0)), int((d != 0).sum()), d.size, int(((d != 0) & ~near_integer(level64)).sum())


def passes(got, level64):
    worst, taken, n, outside = judge(got, level64)
    return worst <= 1 and outside == 0 and taken <= max(CAP * n, 0)


# ---- inputs ------------------------------------------------------------------------------------------------------------------
Case = collections.namedtuple("Case", "name B C h w Ho Wo align kind H W sel xoff seed")


def _case(name, B, C, h, w, Ho=None, Wo=None, align=False, kind="random", H=None, W=None, sel=None, xoff=0, seed=0):
    return Case(name, B, C, h, w, Ho or 2 * h, Wo or 2 * w, align, kind, H or 2 * h + 1, W or 3 * w + 2, sel, xoff, seed)


def seam_cases(geometry):
    """one past each seam of the mapping, in both dimensions: a workgroup takes threads x items runs of `run` pixels, numbered
    row-major, so the seams are a row's last (short) run, and run counts of threads and threads x items"""
    run, threads, items = geometry[:3]
    out = []
    for n in (threads, threads * items):
        out.append(_case(f"seam_tall_{n}", 1, 5, n // 2 + 1, 1, Ho=n + 1, seed=n))                                 # n + 1 rows of one run
        out.append(_case(f"seam_wide_{n}", 1, 5, 1, (n + 1) * run // 2, Ho=1, Wo=(n + 1) * run - 1, seed=n + 1))   # one row of n + 1 runs
    out.append(_case("seam_run", 2, 5, 5, (3 * run + 2) // 2, Wo=3 * run + 1, seed=5))                             # a row's last run holds one pixel
    return out


def cases(geometry=(4, 256, 4, 2)):
    cs = [
        _case("1x1", 1, 5, 1, 1), _case("1x1_align", 2, 5, 1, 1, align=True, seed=1),
        _case("h1", 2, 5, 1, 5, seed=2), _case("w1", 2, 5, 5, 1, seed=3, xoff=1),
        _case("3x5", 2, 5, 3, 5, seed=4, xoff=2), _case("3x5_align", 1, 5, 3, 5, align=True, seed=5, xoff=3),
        _case("7x3_to_10x9", 2, 5, 7, 3, Ho=10, Wo=9, seed=6, xoff=1), _case("7x3_to_10x9_align", 2, 5, 7, 3, Ho=10, Wo=9, align=True, seed=7),
        _case("w2", 1, 5, 4, 2, seed=8, xoff=3), _case("w3", 2, 5, 4, 3, seed=9, xoff=2), _case("w5", 1, 5, 2, 5, seed=10, xoff=1),
        _case("b9", 9, 5, 6, 7, seed=11, xoff=1), _case("b9_single", 9, 5, 6, 7, sel=3, seed=12),
        _case("17x65", 2, 5, 17, 65, seed=13, xoff=2), _case("17x65_align", 2, 5, 17, 65, align=True, seed=14, xoff=1),
    ]
    cs += [_case(f"c{C}", 2, C, 5, 6, kind="random_c", seed=20 + C, xoff=C % 4) for C in (1, 2, 3, 4)]
    cs += seam_cases(geometry)
    cs += [_case("zero_one", 2, 4, 5, 7, kind="zero_one"), _case("levels", 2, 5, 4, 6, kind="levels", xoff=1),
           _case("ties", 2, 5, 4, 6, kind="ties", align=True, xoff=2), _case("outside", 2, 5, 5, 5, kind="outside", xoff=3),
           _case("nonfinite", 2, 5, 6, 5, kind="nonfinite", xoff=1), _case("frames_pm2", 2, 2, 3, 4, kind="frames_pm2")]
    return cs


RANDOM_KINDS = ("random",)           # judged by the float64 rule too (C = 5, softmax of 3 N(0, 1))


def softmax_masks(rng, B, C, h, w):
    z = (3.0 * rng.standard_normal((B, C, h, w))).astype(F32)
    e = np.exp(z - z.max(1, keepdims=True))
    return (e / e.sum(1, keepdims=True)).astype(F32)


def inputs(c):
    """(masks [B, C, h, w], frames [B, 3, H, W]) float32"""
    rng = np.random.RandomState(1000 + c.seed)
    masks = softmax_masks(rng, c.B, c.C, c.h, c.w)
    frames = np.clip(rng.standard_normal((c.B, 3, c.H, c.W)), -2, 2).astype(F32)
    if c.kind == "zero_one":
        masks = (rng.rand(c.B, c.C, c.h, c.w) < 0.5).astype(F32)
        masks[:, 0], masks[:, 1] = 0, 1
    elif c.kind in ("levels", "ties"):
        k = rng.randint(0, 255, size=(c.B, c.C, 1, 1)).astype(F32)
        k[0, 0], k[0, 1] = 0, 254
        masks = np.broadcast_to((k + F32(0.5 if c.kind == "ties" else 0)) / F32(255), masks.shape).astype(F32).copy()
    elif c.kind == "outside":
        masks = (2.0 * rng.standard_normal(masks.shape)).astype(F32)
        masks[:, 0], masks[:, 1] = -0.3, 1.7
        frames = (3.0 * rng.standard_normal(frames.shape)).astype(F32)
    elif c.kind == "nonfinite":
        masks[:, 0], masks[:, 1], masks[:, 2] = np.nan, np.inf, 3e38
        masks[1, 1] = -np.inf
    elif c.kind == "frames_pm2":
        frames = np.where(rng.rand(*frames.shape) < 0.5, F32(-2), F32(2)).astype(F32)
        frames[0, 0], frames[0, 1] = -2, 2
    return masks, frames


def dirty_planes(c):
    """mask channels whose values are not finite (their panels follow the documented bytes, not the torch route)"""
    return (0, 1, 2) if c.kind == "nonfinite" else ()
