"""What the flow-colour tests share (tests/test_flowvis_cpu.py, tests/test_flowvis_gpu.py, tools/time_flowvis.py): a restatement of the
Middlebury colour pass as include/rcf_hip.h states it for rcf_flow_color_f32 (the published wheel, as the flow_vis package's
flow_to_color evaluates it -- written from that statement, not from the package's text), the case list and the comparison rule.

color_levels(flow, head=np.float64) is the yardstick: float64 throughout, on the float32 inputs, with the package's second branch
(col * 0.75 where rad > 1), which is dead in exact arithmetic.  head=np.float32 is the arithmetic of the kernel (and of numpy on
float32 flows): float32 up to the radius and the wheel position, float64 from the interpolation on, where the package's float64
wheel table promotes it; it has no second branch and clamps the level to 0 .. 255, like the kernel.

The rule.  byte = floor(level), level = 255 col.  A byte may differ from floor(level64) by at most 1, and only where level64 lies
within EPS = K 2^-24 255 of an integer; at most CAP of a case's elements may differ.  K bounds the error of col in units of 2^-24
(one rounding of a value <= 1), from the float32 chain (rad <= 1, 1 - col <= 1, so d col <= d rad + d c, d c = d f max|wheel step|):
    rad   u^2, v^2 (1 each; their sum of positives keeps 1), the sum (1), the square root halves that and rounds (1): 2.
          The maximum is one of those (2); + 1e-5f: the sum (1) and the constant's own rounding (1): 4.  A quotient: 5.  The second
          radius: squares 2 x 5 + 1 = 11, sum 12, root 6 + 1:                                                             K_RAD = 7
    f     the divisor is common to both quotients and cancels in the angle; their own roundings (1 + 1) move it by at most half
          their sum: 1.  atan2f: 2 ulp (the bound HIP's documentation lists for it), an ulp of a result in [2, 4) is 4 units: 8.
          / pi: 9 / pi = 2.87, the float32 pi's own error 0.47, the division 1: 4.34.  + 1 (a result up to 2 rounds by 2): 6.34.
          / 2 is exact: 3.17.  x 54: 171.2 and the product's rounding 54: 225.2 units on fk; fk - floor(fk) is exact.
          The steepest wheel step is 64 / 255 (the 4-row green-cyan ramp: 191 -> 255):                             K_F = 225.2 x 64 / 255 = 56.5
    tail  float64, then one conversion:                                                                                  K_TAIL = 1
K = ceil(7 + 56.5 + 1) = 65, EPS = 9.9e-4 levels.  (The interpolation is continuous across k0, so an fk that crosses an integer moves
col by no more than d f times a step, like any other.)"""
import collections
import functools

import numpy as np

NCOLS = 55
SEGMENTS = (("RY", 15), ("YG", 6), ("GC", 4), ("CB", 11), ("BM", 13), ("MR", 6))
K_RAD, K_F, K_TAIL = 7.0, 225.2 * 64.0 / 255.0, 1.0
K = int(np.ceil(K_RAD + K_F + K_TAIL))
EPS = K * 2.0 ** -24 * 255.0
CAP = 1e-3


@functools.lru_cache(None)
def wheel():
    """[55, 3] levels: red -> yellow -> green -> cyan -> blue -> magenta -> red; one channel ramps, one is held at 255"""
    w = np.zeros((NCOLS, 3), dtype=np.int64)
    held = dict(RY=0, YG=1, GC=1, CB=2, BM=2, MR=0)
    ramp = dict(RY=(1, +1), YG=(0, -1), GC=(2, +1), CB=(1, -1), BM=(0, +1), MR=(2, -1))
    col = 0
    for name, n in SEGMENTS:
        r = np.floor(255 * np.arange(n) / n).astype(np.int64)
        ch, sign = ramp[name]
        w[col:col + n, held[name]] = 255
        w[col:col + n, ch] = r if sign > 0 else 255 - r
        col += n
    assert col == NCOLS
    return w


def color_levels(flow, clip=None, head=np.float64):
    """flow [2, h, w] float32 -> level = 255 col as float64 [3, h, w] (plane order red, green, blue)"""
    assert flow.dtype == np.float32 and flow.shape[0] == 2
    T = head
    with np.errstate(all="ignore"):
        u, v = flow[0].astype(T), flow[1].astype(T)
        if clip is not None:
            u, v = np.clip(u, T(0), T(clip)), np.clip(v, T(0), T(clip))
        rad = np.sqrt(u * u + v * v)
        d = rad.max() + T(1e-5)
        u, v = u / d, v / d
        rad = np.sqrt(u * u + v * v)
        a = np.arctan2(-v, -u) / T(np.pi)
        fk = (a + T(1)) / T(2) * T(NCOLS - 1)
        assert fk.dtype == T
        k0 = np.clip(np.floor(fk), 0, NCOLS - 1).astype(np.int64)
        k1 = np.where(k0 + 1 == NCOLS, 0, k0 + 1)
        f = (fk - k0.astype(T)).astype(np.float64)
        if T is not np.float64:
            rad = np.minimum(rad, T(1))               # exact arithmetic never exceeds 1; float32 can, by one rounding
        rad = rad.astype(np.float64)
        tab = wheel().astype(np.float64) / 255.0
        out = np.empty((3,) + u.shape, dtype=np.float64)
        for c in range(3):
            col = (1.0 - f) * tab[k0, c] + f * tab[k1, c]
            lit = 1.0 - rad * (1.0 - col)
            if T is np.float64:
                lit = np.where(rad <= 1.0, lit, col * 0.75)             # the package's out-of-range branch: dead here
            out[c] = 255.0 * lit
    return out


def to_bytes(level):
    """floor, with the kernel's clamp (a float32 radius of 1 + 2^-23 can put a level just below 0)"""
    return np.clip(np.floor(level), 0, 255).astype(np.uint8)


def planes(b, bgr=False):
    return b[::-1] if bgr else b


Verdict = collections.namedtuple("Verdict", "ok differing share worst_step worst_distance")


def judge(got, level64):
    """got: uint8 [3, h, w]; level64: color_levels(...).  -> Verdict; ok = the rule of this file's docstring"""
    want = np.floor(level64)
    step = got.astype(np.float64) - want
    bad = step != 0
    dist = np.abs(level64 - np.rint(level64))
    n = int(bad.sum())
    worst_step = float(np.abs(step).max()) if step.size else 0.0
    worst_dist = float(dist[bad].max()) if n else 0.0
    ok = worst_step <= 1 and worst_dist <= EPS and n <= CAP * bad.size
    return Verdict(bool(ok), n, n / bad.size, worst_step, worst_dist)


# ------------------------------------------------------------------------------------------------------------------- cases
BASE_SHAPES = [(1, 1), (1, 2), (3, 5), (1, 63), (1, 64), (1, 65), (48, 48), (96, 160)]
FINITE_KINDS = ("normal", "ints", "zero", "const", "outlier", "tiny", "huge")
BIT_EQUAL_KINDS = ("ints", "zero", "const")         # no difference at all is allowed here


def geometry_shapes(one_wg_pixels):
    """one image just above what a workgroup takes in the one-launch form, one above twice that (both odd-sized)"""
    a, b = one_wg_pixels + 1, 2 * one_wg_pixels + 1
    def rows(n):
        for h in (3, 7, 17, 1):
            if n % h == 0:
                return (h, n // h)
    return [rows(a), rows(b)]


def draw(kind, h, w, seed=0):
    """one flow image [2, h, w] float32"""
    g = np.random.default_rng(1000 * h + 7 * w + seed + sum(map(ord, kind)))
    if kind == "normal":
        f = 3.0 * g.standard_normal((2, h, w))
    elif kind == "ints":
        f = g.integers(-4, 5, size=(2, h, w)).astype(np.float64)
        f = np.where((f == 0) & (g.random((2, h, w)) < 0.5), -0.0, f)
        flat = f.reshape(2, -1)
        if flat.shape[1] >= 3:                       # (u > 0, v = +0), (u > 0, v = -0) and a larger flow next to them
            flat[:, 0], flat[:, 1], flat[:, 2] = (1.0, 0.0), (1.0, -0.0), (3.0, -4.0)
    elif kind == "zero":
        f = np.zeros((2, h, w))
    elif kind == "const":
        f = np.broadcast_to(np.array([1.5, -0.25]).reshape(2, 1, 1), (2, h, w)).copy()
    elif kind == "outlier":
        # The outlier's own radius is 1 - 1e-14, so its level is 255 c + 1e-12: at an angle where 255 c is an integer (a diagonal:
        # fk = 47.25, 255 c = 220 exactly) floor() is discontinuous there and two float64 evaluations in different orders already
        # disagree (220.0000000000002 against 219.99999999999997).  A generic angle (fk = 51.9, 255 c = 132.6) tests the kernel.
        f = g.standard_normal((2, h, w))
        f.reshape(2, -1)[:, (h * w) // 2] = (1e9, -2.5e8)
    elif kind == "tiny":
        f = 1e-30 * g.standard_normal((2, h, w))
    elif kind == "huge":
        f = 1e18 * g.uniform(-1, 1, size=(2, h, w))
    else:
        raise ValueError(kind)
    return f.astype(np.float32)


@functools.lru_cache(None)
def batch(h, w, kinds=FINITE_KINDS, seed=0):
    """(flows [len(kinds), 2, h, w] float32, levels64 [len(kinds), 3, h, w]): computed once, shared, read-only"""
    flows = np.stack([draw(k, h, w, seed) for k in kinds])
    levels = np.stack([color_levels(f) for f in flows])
    flows.setflags(write=False)
    levels.setflags(write=False)
    return flows, levels


# ------------------------------------------------------------------------------------------------------------------- the grid
def reference_route(flow_1chw, let_upload):
    """the reference's let_tensor_vis for one [1, 2, h, w] device tensor, restated: clone, .cpu(), numpy's wheel, upload"""
    t = flow_1chw.clone().squeeze(0).permute(1, 2, 0).cpu().numpy()
    rgb = to_bytes(color_levels(np.ascontiguousarray(t.transpose(2, 0, 1)), head=np.float32))
    return let_upload(rgb[None])
