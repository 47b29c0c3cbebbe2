"""Edge-shape cases of the pooling, resize and layout kernels (csrc/spatial.hip) and their reference.

Shared by tests/test_spatial_sweep_cpu.py (the tables reach the dispatch branches they name; the restatement agrees with torch's
float64 F.interpolate / F.max_pool2d / autograd; its own float32 run sits within a quarter of every bound) and
tests/test_spatial_sweep_gpu.py (the kernels against the float64 truth).  The reference is numpy / torch on the CPU, written out
tap by tap; nothing of the HIP package enters this module.

Bilinear resize.  Per axis, PyTorch's area_pixel_compute_source_index in float32 (`axis_taps`): scale = in / out (align_corners:
(in - 1) / (out - 1), 0 for one output), position max(scale * (dst + 0.5) - 0.5, 0) (align_corners: scale * dst), i0 the
truncated position clamped to in - 1, i1 = i0 + (i0 < in - 1), lambda = position - i0.  The two taps of an output index are laid
down with weights 1 - lambda and lambda as one row of a [out, in] matrix per axis (float64; a clamped border row holds their
sum), the forward applies the two matrices to the input in float64 and the backward their transposes (the exact transpose,
scattered in float64).  Alongside: the mass sum |w| |v| per element and, for the backward, the number of non-zero terms.

Two kinds of resize case.
  exact    the float32 scale and every float32 source position are exact, with or without a fused multiply-add, so the
           reference's weights ARE the kernel's weights.  Sufficient: without align_corners out / gcd(in, out) is a power of two
           (an output size that is a power of two, and every exact 2x), with it (out - 1) / gcd(in - 1, out - 1) is (or out is 1):
           then scale is a dyadic rational of a few bits and scale * (2 dst + 1) / 2 needs no rounding.  The CPU test checks the
           positions against rational arithmetic.  Bounds PER ELEMENT:
               forward   16 * 2^-24 * mass                 (the expression hy (hx a + lx b) + ly (hx c + lx d) has 7 roundings)
               backward  (16 + terms) * 2^-24 * mass       (2 roundings per term g (wy wx), plus the additions)
           accumulating onto a prior value (beta = 1) the prior value is one more term of the sum: terms + 1, mass + |old|.  On
           16-bit storage half an ulp of the storage type at |ref| is added for the single rounding of the result; inputs are
           drawn already representable.
  inexact  (7x9 -> 20x31, 60x107 -> 480x854, ...) the last bit of a position depends on contraction: the project's floors,
           2e-5 of max |ref| per image for fp32 tensors and 5e-3 (FLOOR_BF16 of bn_cases.py) for 16-bit storage.

Frame forms: the forward writes only the output pixels within `frame` of the border (the same values there; the rest keeps its
NaN fill), the backward takes the gradient as zero off that frame (and must not read it there: it holds NaN).

Max-pool 3x3 / stride 2 / pad 1: the window maximum with the index of the first valid tap; a later tap replaces it on a strict
`>` or on NaN (torch's max_pool2d).  The maximum is exact in every storage type.  Backward: a float64 scatter to that index.

Layout kernels, copy2d, copy2d_batched, split_rect: plain indexing, compared for equal bits; a cast or an accumulation into a
16-bit destination against the float32 sum rounded once by torch.

Dispatch conditions of rcf_resize_bilinear_nhwc_{fwd,bwd}_mp are restated below (`fwd_branch`, `bwd_branch`) to CHOOSE inputs
and to assert that the tables reach every branch -- never as a reference for a value.
"""
import dataclasses
import functools
import math
from fractions import Fraction

import numpy as np
import pytest
import torch

U32 = 2.0 ** -24                                     # unit roundoff of float32
FLOOR_F32, FLOOR_H16 = 2e-5, 5e-3                    # the project's floors (tests/test_kernels_gpu.py; bn_cases.FLOOR_BF16)
FILL = 7.0                                           # what guard channels hold
SLICE0 = 8                                           # first channel of a pitched operand inside its buffer
TRIP = 8192 * 256                                    # work items one trip of a grid-stride loop covers (ew_blocks caps at 8192 blocks)
TORCH = {"f32": torch.float32, "bf16": torch.bfloat16, "f16": torch.float16}
MANT = {"bf16": 7, "f16": 10}                        # stored fraction bits
EMIN = {"bf16": -126, "f16": -14}


# =================================================================================================== resize: the reference
def host_scale(inp, out, align):
    if align:
        return np.float32(inp - 1) / np.float32(out - 1) if out > 1 else np.float32(0)
    return np.float32(inp) / np.float32(out)


def axis_taps(out, inp, align):
    """(i0, i1, lambda) of every output index along one axis, in float32 as PyTorch computes them"""
    s = host_scale(inp, out, align)
    d = np.arange(out, dtype=np.float32)
    half = np.float32(0.5)
    pos = s * d if align else np.maximum(s * (d + half) - half, np.float32(0))
    assert pos.dtype == np.float32
    i0 = np.minimum(pos.astype(np.int64), inp - 1)
    i1 = i0 + (i0 < inp - 1)
    lam = pos - i0.astype(np.float32)
    return i0, i1, lam


def axis_matrix(out, inp, align, dtype=torch.float64):
    """[out, in]: row o holds 1 - lambda at i0 and lambda at i1 (their sum where the border clamps both onto one pixel),
    accumulated in `dtype`"""
    i0, i1, lam = axis_taps(out, inp, align)
    npdt = np.float64 if dtype == torch.float64 else np.float32
    A = np.zeros((out, inp), dtype=npdt)
    r = np.arange(out)
    np.add.at(A, (r, i0), npdt(1) - lam.astype(npdt))
    np.add.at(A, (r, i1), lam.astype(npdt))
    return torch.from_numpy(A)


def frame_mask(H, W, t):
    """bool [H, W]: within t of the border (t <= 0: everything)"""
    if t <= 0:
        return torch.ones(H, W, dtype=torch.bool)
    y, x = torch.arange(H)[:, None], torch.arange(W)[None, :]
    return (y < t) | (y >= H - t) | (x < t) | (x >= W - t)


def _apply(Ay, Ax, x):
    """out[n, o, p, c] = sum_h sum_w Ay[o, h] Ax[p, w] x[n, h, w, c]: columns first, then rows (the kernels' order)"""
    t = torch.einsum("pw,nhwc->nhpc", Ax, x)
    return torch.einsum("oh,nhpc->nopc", Ay, t)


def resize_fwd_ref(x, Ho, Wo, align, dtype=torch.float64):
    """x [N, Hi, Wi, C] -> (out, mass), both [N, Ho, Wo, C] in `dtype`"""
    Hi, Wi = x.shape[1:3]
    Ay, Ax = axis_matrix(Ho, Hi, align, dtype), axis_matrix(Wo, Wi, align, dtype)
    x = x.to(dtype)
    return _apply(Ay, Ax, x), _apply(Ay, Ax, x.abs())


def resize_bwd_ref(dy, Hi, Wi, align, frame=0, dtype=torch.float64):
    """dy [N, Ho, Wo, C] (taken as zero off the frame) -> (dx, mass [N, Hi, Wi, C], terms [Hi, Wi])"""
    Ho, Wo = dy.shape[1:3]
    Ay, Ax = axis_matrix(Ho, Hi, align, dtype), axis_matrix(Wo, Wi, align, dtype)
    M = frame_mask(Ho, Wo, frame)
    g = torch.where(M[None, :, :, None], dy.to(dtype), torch.zeros((), dtype=dtype))
    dx, mass = _apply(Ay.t(), Ax.t(), g), _apply(Ay.t(), Ax.t(), g.abs())
    By, Bx = (Ay != 0).double(), (Ax != 0).double()
    terms = By.t() @ M.double() @ Bx
    return dx, mass, terms.round().long()


def half_ulp(ref, dt):
    """half an ulp of the 16-bit storage type dt at |ref| (float64 tensor); 0 for fp32 storage"""
    if dt == "f32":
        return torch.zeros_like(ref)
    _, e = torch.frexp(ref.abs().clamp_min(1e-300))              # |ref| = m 2^e, m in [0.5, 1)
    e = (e - 1).clamp_min(EMIN[dt])
    return 0.5 * torch.exp2((e - MANT[dt]).double())


def elem_margin(got, ref, bound):
    """worst |got - ref| / bound over the elements; an error under a zero bound, or a NaN anywhere, gives inf"""
    d = (got.double() - ref.double()).abs()
    if bool(torch.isnan(d).any()):
        return float("inf")
    if not d.numel():
        return 0.0
    r = d / bound
    r = torch.where(d == 0, torch.zeros_like(r), r)               # 0 / 0: no error under a zero bound
    return float(r.max())


def image_margin(got, ref, floor, mask=None):
    """worst over the images of max |got - ref| / (floor * max |ref|), over the masked [H, W] pixels"""
    d, r = (got.double() - ref.double()).abs(), ref.double().abs()
    if mask is not None:
        d, r = d[:, mask], r[:, mask]
    d, r = d.reshape(d.shape[0], -1), r.reshape(r.shape[0], -1)
    if bool(torch.isnan(d).any()):
        return float("inf")
    return float((d.amax(1) / (floor * r.amax(1)).clamp_min(1e-300)).max())


def fwd_bound(mass, ref, dt):
    return 16 * U32 * mass + half_ulp(ref, dt)


def bwd_bound(mass, terms, ref, dt):
    return (16 + terms[None, :, :, None].double()) * U32 * mass + half_ulp(ref, dt)


def floor_of(dt):
    return FLOOR_F32 if dt == "f32" else FLOOR_H16


# ====================================================================================================== resize: the cases
@dataclasses.dataclass(frozen=True)
class Resize:
    name: str
    N: int
    Hi: int
    Wi: int
    Ho: int
    Wo: int
    C: int
    align: bool = False
    frames: tuple = (0,)
    variants: tuple = (("f32", 0),)          # (storage, pitch): pitch 0 = contiguous, else the slice [..., 8:8 + C] of a buffer this wide
    betas: tuple = (0, 1)
    seed: int = 0
    smooth: bool = False                     # inputs: a smooth field under 5 % noise instead of plain noise (see smooth_field)

    @property
    def exact(self):
        return axis_exact(self.Hi, self.Ho, self.align) and axis_exact(self.Wi, self.Wo, self.align)

    @property
    def bytes(self):
        """fp32 bytes of the larger pair (input + output) of a run"""
        return 4 * self.N * self.C * (self.Hi * self.Wi + self.Ho * self.Wo)


def pow2(n):
    return n >= 1 and n & (n - 1) == 0


def axis_exact(inp, out, align):
    if align:
        return out == 1 or inp == 1 or pow2((out - 1) // math.gcd(inp - 1, out - 1))
    return pow2(out // math.gcd(inp, out))


F32, BF16, F16 = ("f32", 0), ("bf16", 0), ("f16", 0)
RESIZE = [
    # ---- exact 2x (resize2x_{fwd,bwd}_kernel), C in {4, 20, 24, 64}
    Resize("x2_c4", 2, 4, 8, 8, 16, 4, variants=(F32, BF16), seed=301),                       # one channel vector per pixel; bf16 V = 4
    Resize("x2_c64", 1, 8, 16, 16, 32, 64, variants=(F32, BF16), seed=302),                   # Wi CV = 256 (fp32): exactly one block per row
    Resize("x2_c20_wide", 1, 2, 64, 4, 128, 20, variants=(F32, BF16), seed=303),              # Wi CV = 320: a second block with a tail; C % 8 == 4
    Resize("x2_c24_pitched", 2, 8, 8, 16, 16, 24, variants=(("f32", 40), ("bf16", 40), ("bf16", 36), ("f16", 40)), seed=304),
    Resize("x2_odd", 2, 7, 9, 14, 18, 4, seed=305),                                           # odd sizes: the last 2 x 2 input block is cut
    # ---- the border frame of an exact 2x: ts <= 7 up to frame 14 (forward), tb <= 3 up to frame 7 (backward, accumulating)
    Resize("x2_frame", 2, 16, 32, 32, 64, 4, frames=(1, 2, 7, 8, 14, 15), variants=(F32,), seed=306),
    Resize("x2_frame_c24", 1, 16, 16, 32, 32, 24, frames=(2, 7), variants=(BF16, ("bf16", 36)), seed=307),
    Resize("x2_frame_odd", 1, 15, 17, 30, 34, 4, frames=(1, 3, 5), seed=308),                 # odd sizes: the + 1 of tb
    # ---- the rows kernels
    Resize("x2_general", 2, 8, 8, 16, 16, 4, frames=(-1,), variants=(F32, BF16), seed=309),   # an exact 2x on the general kernel
    Resize("up4_c64", 1, 4, 4, 16, 16, 64, variants=(F32, BF16, F16), seed=310),              # Wo CV = 256 (fp32), 128 at V = 8
    Resize("up4_wide", 1, 2, 16, 8, 64, 20, variants=(F32, BF16), seed=311),                  # Wo CV = 320: tail of the second block
    Resize("up_down", 2, 8, 16, 16, 4, 4, seed=312),                                          # rows 2x up, columns 4x down
    Resize("down_up", 2, 16, 4, 4, 16, 24, variants=(F32, BF16), seed=313),
    Resize("shrink_1p5", 2, 12, 24, 8, 16, 4, frames=(0, 1, 3), seed=314),                    # ratio 1.5, exact; the MAXC fast path
    Resize("row_2x", 2, 1, 8, 2, 16, 4, seed=315),                                            # Hi == 1 under an exact 2x
    Resize("col_2x", 2, 8, 1, 16, 2, 4, seed=316),                                            # Wi == 1 under an exact 2x
    Resize("align_exact", 2, 5, 9, 9, 17, 20, align=True, frames=(0, 2), variants=(F32, BF16), seed=317),
    Resize("align_one_row", 2, 5, 9, 1, 17, 4, align=True, seed=318),                         # Ho == 1: scale 0, every row is a candidate
    Resize("align_one_col", 2, 5, 9, 9, 1, 4, align=True, seed=319),                          # Wo == 1
    Resize("align_from_one_row", 2, 1, 9, 5, 17, 4, align=True, seed=330),                   # Hi == 1: scale 0 the other way round
    Resize("up_inexact", 3, 7, 9, 20, 31, 4, frames=(0, 3), variants=(F32, BF16), seed=320),
    Resize("down_inexact", 3, 20, 31, 7, 9, 24, variants=(F32, BF16), seed=321),              # a ratio that is no integer, shrinking
    Resize("mix_inexact", 2, 9, 20, 20, 7, 4, align=True, seed=322),
    Resize("big_inexact", 1, 60, 107, 480, 854, 4, betas=(0,), seed=323, smooth=True),
    # ---- the grid-stride fallbacks: N * Ho > 65535 (forward), N * Hi > 65535 (backward)
    Resize("fb_up", 8192, 3, 3, 8, 8, 4, frames=(0, 1, 3), variants=(F32, BF16), seed=324),
    Resize("fb_up_c20", 8192, 3, 3, 8, 8, 20, betas=(0,), seed=325),                          # forward: 2.6 M items, the second trip (42 MB)
    Resize("fb_general_2x", 8192, 4, 4, 8, 8, 4, frames=(-1,), seed=326),                     # an exact 2x through the forward fallback
    Resize("fb_down", 8192, 8, 8, 4, 4, 4, frames=(0, 1), seed=327),                          # backward fallback, MAXC fast path
    Resize("fb_down_c20", 8192, 8, 7, 4, 4, 20, betas=(1,), seed=328),                        # backward: 2.3 M items, the second trip
    Resize("fb_align_frame", 4096, 16, 16, 17, 17, 4, align=True, frames=(1, 3, 4), seed=329),  # tc = 5, 7 and (too thick) 0
]
RESIZE_BY_NAME = {c.name: c for c in RESIZE}


def resize_runs():
    for c in RESIZE:
        for dt, pitch in c.variants:
            for frame in c.frames:
                yield c, dt, pitch, frame


def run_id(c, dt, pitch, frame, beta=None):
    s = f"{c.name}-{dt}" + (f"_p{pitch}" if pitch else "") + (f"-frame{frame}" if frame else "")
    return s if beta is None else s + f"-beta{beta}"


PARAMS_FWD = [pytest.param(c, dt, p, f, id=run_id(c, dt, p, f)) for c, dt, p, f in resize_runs()]
PARAMS_BWD = [pytest.param(c, dt, p, f, b, id=run_id(c, dt, p, f, b)) for c, dt, p, f in resize_runs() for b in c.betas]


# --------------------------------------------------------------------------------- dispatch restated (to choose inputs)
def vec_width(dt, C, pitch):
    return 8 if dt != "f32" and C % 8 == 0 and (pitch or C) % 8 == 0 else 4


def fwd_branch(c, dt, pitch, frame):
    """(kernel, frame kind, V) the forward dispatcher takes"""
    general = frame == -1
    fr = 0 if general else frame
    V = vec_width(dt, c.C, pitch)
    x2 = not general and not c.align and c.Ho == 2 * c.Hi and c.Wo == 2 * c.Wi
    if x2 and fr == 0 and c.Hi >= 2 and c.Wi >= 2 and c.N * c.Hi <= 65535:
        return "2x", "whole", V
    ts = (fr + 1) // 2
    if x2 and fr > 0 and 2 * ts < c.Hi and 2 * ts < c.Wi and c.N <= 65535:
        return "2x", "frame", V
    kind = "general" if general else ("frame" if fr > 0 else "whole")
    if c.N * c.Ho <= 65535:
        return "rows", kind, V
    return "fallback", kind, 4


def tc_of(c, frame, beta):
    f32 = np.float32
    if frame <= 0 or not beta:
        return 0
    smax = max(f32(c.Hi) / f32(c.Ho), f32(c.Wi) / f32(c.Wo))
    tc = int(np.ceil(f32(smax * f32(frame + 2)))) + 2
    return 0 if 2 * tc >= c.Hi or 2 * tc >= c.Wi else tc


def bwd_branch(c, dt, pitch, frame, beta):
    """(kernel, frame kind, V, tc) the backward dispatcher takes"""
    general = frame == -1
    fr = 0 if general else frame
    V = vec_width(dt, c.C, pitch)
    x2 = not general and not c.align and c.Ho == 2 * c.Hi and c.Wo == 2 * c.Wi
    Hh, Wh = (c.Hi + 1) // 2, (c.Wi + 1) // 2
    if x2 and fr == 0 and c.Hi >= 2 and c.Wi >= 2 and c.N * Hh <= 65535:
        return "2x", "whole", V, 0
    tb = (fr // 2 + 2) // 2 + 1
    if x2 and fr > 0 and beta and 2 * tb < Hh and 2 * tb < Wh and c.N <= 65535:
        return "2x", "frame", V, 0
    kind = "general" if general else ("frame" if fr > 0 else "whole")
    if c.N * c.Hi <= 65535:
        return "rows", kind, V, 0
    return "fallback", kind, 4, tc_of(c, fr, beta)


def bwd_fast_share(c):
    """share of the input pixels whose candidate ranges fit the MAXC = 6 fast path of the general backward kernels
    (cand_range restated in float32)"""
    f32 = np.float32

    def width(inp, out, scale):
        if scale <= 0:
            return np.full(inp, out - 1)
        inv = f32(1) / scale
        i = np.arange(inp, dtype=np.float32)
        if c.align:
            a, b = (i - f32(1)) * inv, (i + f32(1)) * inv
        else:
            a, b = (i - f32(0.5)) * inv - f32(0.5), (i + f32(1.5)) * inv - f32(0.5)
        lo = np.maximum(np.floor(a).astype(np.int64) - 1, 0)
        hi = np.minimum(np.ceil(b).astype(np.int64) + 1, out - 1)
        return hi - lo
    wy, wx = width(c.Hi, c.Ho, host_scale(c.Hi, c.Ho, c.align)), width(c.Wi, c.Wo, host_scale(c.Wi, c.Wo, c.align))
    return float(((wy[:, None] < 6) & (wx[None, :] < 6)).mean())


# ----------------------------------------------------------------------------------------------------------- resize inputs
def stored(t, dt):
    """the float64 of what a tensor of storage type dt holds"""
    return t.to(TORCH[dt]).double()


def smooth_field(N, H, W, C, g):
    """sin / cos waves of one to two periods per axis with a phase per (image, channel), under normal noise of 0.05.  For the
    60x107 -> 480x854 cases: at a position near 107 float32 resolves 8e-6, so its source positions differ from the float64 ones
    by up to 1e-5 of a pixel, and on plain noise (neighbours 5 sigma apart) that alone is half the 2e-5 floor -- a statement
    about float32 positions, not about any kernel.  On an image-like field it is a tenth of the floor."""
    y, x = torch.arange(H).double()[:, None] / H, torch.arange(W).double()[None, :] / W
    ph = 6.283 * torch.rand(N, 1, 1, C, generator=g).double()
    f = torch.sin(9.0 * y + 5.0 * x)[None, :, :, None] * torch.ones(N, 1, 1, C).double()
    f = torch.sin(7.0 * y[None, :, :, None] + ph) * torch.cos(11.0 * x[None, :, :, None] - ph) + 0.5 * f
    return (f + 0.05 * torch.randn(N, H, W, C, generator=g).double()).float()


@functools.lru_cache(maxsize=2)
def resize_inputs(name, dt):
    """x [N, Hi, Wi, C], dy [N, Ho, Wo, C], old [N, Hi, Wi, C] (what an accumulating backward finds): float64 tensors holding
    values the storage type represents; normal draws under per-channel scales 2^(2u).  Callers leave them unchanged."""
    c = RESIZE_BY_NAME[name]
    g = torch.Generator().manual_seed(c.seed)
    sc = lambda: torch.exp2(2 * torch.rand(c.C, generator=g))
    draw = (lambda *s: smooth_field(*s, g)) if c.smooth else (lambda *s: torch.randn(*s, generator=g))
    x = stored(draw(c.N, c.Hi, c.Wi, c.C) * sc(), dt)
    dy = stored(draw(c.N, c.Ho, c.Wo, c.C) * sc(), dt)
    old = stored(draw(c.N, c.Hi, c.Wi, c.C) * sc(), dt)
    return x, dy, old


@functools.lru_cache(maxsize=1)
def resize_fwd_truth(name, dt):
    c = RESIZE_BY_NAME[name]
    return resize_fwd_ref(resize_inputs(name, dt)[0], c.Ho, c.Wo, c.align)


@functools.lru_cache(maxsize=1)
def resize_bwd_truth(name, dt, frame):
    c = RESIZE_BY_NAME[name]
    return resize_bwd_ref(resize_inputs(name, dt)[1], c.Hi, c.Wi, c.align, max(frame, 0))


def with_beta(dx, mass, terms, old, beta):
    """the accumulating form: the prior value is one more term"""
    return (dx + old, mass + old.abs(), terms + 1) if beta else (dx, mass, terms)


def resize_margins(c, dt, got, ref, mass, terms=None, mask=None):
    """worst error / bound: per element on exact cases, per image against the floor otherwise (over `mask` [H, W] when given)"""
    if c.exact:
        bound = fwd_bound(mass, ref, dt) if terms is None else bwd_bound(mass, terms, ref, dt)
        if mask is not None:
            got, ref, bound = got[:, mask], ref[:, mask], bound[:, mask]
        return elem_margin(got, ref, bound)
    return image_margin(got, ref, floor_of(dt), mask)


# NCHW bilinear (fp32): planes, Hi, Wi, Ho, Wo, align
NCHW = [("exact", (2, 3), 6, 10, 16, 32, False), ("align", (2, 3), 5, 9, 9, 17, True), ("davis", (6,), 60, 107, 480, 854, False)]


def nchw_input(name, planes, Hi, Wi):
    """float32 [*planes, Hi, Wi]: plain noise, a smooth field for the 480x854 case (see smooth_field)"""
    g = torch.Generator().manual_seed(41)
    if name == "davis":
        return smooth_field(1, Hi, Wi, math.prod(planes), g).permute(0, 3, 1, 2).reshape(*planes, Hi, Wi).contiguous()
    return torch.randn(*planes, Hi, Wi, generator=g)


# ================================================================================================================ max-pool
def pool_out(n):
    return (n - 1) // 2 + 1


def maxpool_ref(x):
    """x [N, H, W, C] in any dtype -> (y float64 [N, Ho, Wo, C], code uint8 = 3 r + s of the winning tap)"""
    N, H, W, C = x.shape
    Ho, Wo = pool_out(H), pool_out(W)
    best = torch.full((N, Ho, Wo, C), -math.inf, dtype=torch.float64)
    code = torch.full((N, Ho, Wo, C), -1, dtype=torch.int16)
    for r in range(3):
        ys = 2 * torch.arange(Ho) - 1 + r
        vy = (ys >= 0) & (ys < H)
        for s in range(3):
            xs = 2 * torch.arange(Wo) - 1 + s
            vx = (xs >= 0) & (xs < W)
            v = x[:, ys.clamp(0, H - 1)][:, :, xs.clamp(0, W - 1)].double()
            valid = (vy[:, None] & vx[None, :])[None, :, :, None]
            take = valid & ((code < 0) | (v > best) | torch.isnan(v))
            best = torch.where(take, v, best)
            code = torch.where(take, torch.full((), 3 * r + s, dtype=torch.int16), code)
    assert int(code.min()) >= 0
    return best, code.to(torch.uint8)


def pool_flat_index(code, H, W):
    """winning input pixel y W + x per output element (torch's return_indices convention), int64 [N, Ho, Wo, C]"""
    N, Ho, Wo, C = code.shape
    r, s = (code // 3).long(), (code % 3).long()
    yi = 2 * torch.arange(Ho)[None, :, None, None] - 1 + r
    xi = 2 * torch.arange(Wo)[None, None, :, None] - 1 + s
    return yi * W + xi


def maxpool_bwd_ref(dy, code, H, W, dtype=torch.float64):
    """(dx, mass [N, H, W, C], terms [N, H, W, C]): dy scattered to the winning pixel"""
    N, Ho, Wo, C = dy.shape
    idx = pool_flat_index(code, H, W).reshape(N, Ho * Wo, C)
    g = dy.to(dtype).reshape(N, Ho * Wo, C)
    z = lambda dt: torch.zeros(N, H * W, C, dtype=dt)
    dx = z(dtype).scatter_add_(1, idx, g)
    mass = z(dtype).scatter_add_(1, idx, g.abs())
    terms = z(torch.int64).scatter_add_(1, idx, torch.ones_like(idx))
    return dx.reshape(N, H, W, C), mass.reshape(N, H, W, C), terms.reshape(N, H, W, C)


def pool_bwd_bound(mass, terms, ref, dt):
    """a float32 sum of `terms` addends: each addition rounds by at most 2^-24 of a partial sum that stays under mass (1 + terms 2^-24);
    one term is copied, not added"""
    return (terms - 1).clamp_min(0).double() * U32 * mass * (1 + 4 * U32) + half_ulp(ref, dt)


POOL_HW = [(1, 1), (1, 9), (8, 1), (7, 10), (15, 22)]
POOL_N, POOL_C = 2, 8
POOL_KINDS = ("normal", "relu_ties", "special")
# the second trip of the grid-stride loop: (what, N, H, W, C, storage)
POOL_BIG_BWD = (1, 182, 182, 256, "f32")
POOL_BIG_FWD = (1, 514, 514, 128, "bf16")


def pool_input(H, W, kind, dt, N=POOL_N, C=POOL_C, seed=0):
    """float64 [N, H, W, C] of values dt represents"""
    g = torch.Generator().manual_seed(1000 * H + 10 * W + seed)
    x = torch.randn(N, H, W, C, generator=g)
    if kind == "relu_ties":
        x = torch.relu((x * 2).round() / 2)                       # half of it zero, the rest on a grid of 0.5: ties in most windows
    if kind == "special":
        k = torch.rand(N, H, W, C, generator=g)
        x = torch.where(k < 0.06, torch.full((), math.nan), x)
        x = torch.where((k >= 0.06) & (k < 0.12), torch.full((), math.inf), x)
        x = torch.where((k >= 0.12) & (k < 0.3), torch.full((), -math.inf), x)
        x[:, : min(H, 4), : min(W, 4), 0] = -math.inf            # whole windows of -inf: the first valid tap stays
        x[:, H - 1, W - 1, 1] = math.nan                          # a NaN in the last tap of the last window
    return stored(x, dt)


# ================================================================================================ layout / copies / split
def nchw_to_nhwc_ref(x, cpad):
    N, C, H, W = x.shape
    out = torch.zeros(N, H, W, cpad, dtype=x.dtype)
    out[..., :C] = x.permute(0, 2, 3, 1)
    return out


def nhwc_to_nchw_ref(x, C):
    return x[..., :C].permute(0, 3, 1, 2).contiguous()


LAYOUT = [(2, 1, 5, 7, 4), (2, 3, 5, 7, 4), (2, 3, 5, 7, 8), (2, 5, 5, 7, 8)]           # N, C, H, W, Cpad
LAYOUT_BIG_TO = (1, 1, 1450, 1450, 4)                                                    # 2 102 500 pixels
LAYOUT_BIG_BACK = (1, 3, 840, 840, 4)                                                    # N, C, H, W, pitch: 2 116 800 elements

COPY_PAIRS = [("f32", "f32"), ("h16", "h16"), ("f32", "h16"), ("h16", "f32")]
COPY_SHAPES = [(37, 20, 28, 24), (1, 64, 64, 64), (1, 4, 12, 8)]                         # rows, C, spitch, dpitch
COPY_BIG = (8200, 1024)                                                                  # 2 099 200 items, 16-bit on both sides


def copy2d_ref(src, dst, beta, ddt):
    """src, dst float32 [rows, C] of stored values -> what dst holds after the call, in torch dtype ddt: one rounding"""
    return (dst + src if beta else src).to(ddt)


def batched_index(base, pitch, b0, b1, rows, C, n0, n1):
    """element offsets [n0, n1, rows, C] of copy2d_batched's operand"""
    a = lambda n: torch.arange(n, dtype=torch.int64)
    return (base + a(n0)[:, None, None, None] * b0 + a(n1)[None, :, None, None] * b1 + a(rows)[None, None, :, None] * pitch
            + a(C)[None, None, None, :])


@dataclasses.dataclass(frozen=True)
class Batched:
    name: str
    n0: int
    n1: int
    rows: int
    C: int
    src_len: int
    src: tuple                # base, pitch, b0, b1
    dst_len: int
    dst: tuple


def _pair_cases():
    """the frame-pair gather and scatter of layers.pair_concat: [B I, H, W, C] <-> [B, H, W, I C], frames in order or reversed"""
    B, I, H, W, C = 2, 3, 5, 7, 8
    HW = H * W
    n, out = B * I * HW * C, []
    for tag, first, step in (("", 0, 1), ("_reversed", I - 1, -1)):
        frames = (first * HW * C, C, I * HW * C, step * HW * C)
        pairs = (0, I * C, HW * I * C, C)
        out.append(Batched("gather" + tag, B, I, HW, C, n, frames, n, pairs))
        out.append(Batched("scatter" + tag, B, I, HW, C, n, pairs, n, frames))
    return out


# 4097 = 17 x 241 copies: the block cap 4096 / (n0 n1) yields one block per copy, 65 x 4 = 260 items > 256 threads
BATCHED = _pair_cases() + [Batched("cap_4097", 17, 241, 65, 16, 4097 * 65 * 16, (0, 16, 241 * 65 * 16, 65 * 16),
                                   4097 * 65 * 20, (4, 20, 241 * 65 * 20, 65 * 20))]


def batched_ref(src, dst, b, beta, ddt):
    """flat float32 src / dst -> flat dst after the call in torch dtype ddt"""
    si = batched_index(*b.src, b.rows, b.C, b.n0, b.n1).reshape(-1)
    di = batched_index(*b.dst, b.rows, b.C, b.n0, b.n1).reshape(-1)
    assert int(si.min()) >= 0 and int(si.max()) < b.src_len and int(di.min()) >= 0 and int(di.max()) < b.dst_len
    assert di.unique().numel() == di.numel()
    out = dst.clone()
    out[di] = (dst[di] + src[si]) if beta else src[si]
    return out.to(ddt)


def split_rect_ref(x, rect):
    """(inside, outside) of a [N, H, W, C] tensor; rect = (y0, x0, h, w)"""
    y0, x0, h, w = rect
    m = torch.zeros(x.shape[1], x.shape[2], dtype=torch.bool)
    m[y0:y0 + h, x0:x0 + w] = True
    m = m[None, :, :, None]
    z = torch.zeros((), dtype=x.dtype)
    return torch.where(m, x, z), torch.where(m, z, x)


SPLIT_SHAPE = (2, 6, 9, 8)                                                                # N, H, W, C
SPLIT_RECTS = [(0, 0, 2, 3), (0, 5, 3, 4), (4, 0, 2, 2), (4, 5, 2, 4), (3, 4, 1, 1), (0, 0, 6, 9), (1, 1, 4, 7)]
SPLIT_BIG = (2, 100, 165, 256, (17, 29, 50, 100))                                         # 2 112 000 items


# ========================================================================================================= exactness check
def positions_exact(out, inp, align):
    """the float32 positions of an axis equal the rational ones"""
    s = host_scale(inp, out, align)
    d = np.arange(out, dtype=np.float32)
    pos = s * d if align else np.maximum(s * (d + np.float32(0.5)) - np.float32(0.5), np.float32(0))
    for o in range(out):
        if align:
            want = Fraction(inp - 1, out - 1) * o if out > 1 else Fraction(0)
        else:
            want = max(Fraction(inp, out) * Fraction(2 * o + 1, 2) - Fraction(1, 2), Fraction(0))
        if Fraction(float(pos[o])) != want:
            return False
    return True
