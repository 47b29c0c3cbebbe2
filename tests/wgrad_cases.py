"""The cases of tests/test_wgrad_bits_gpu.py: shapes that reach every instantiation the dispatch can launch of the four weight-gradient kernels whose GEMM
columns are (tap, input channel) pairs (csrc/wgrad_cols.h: igemm_wgrad_h2t_kernel, igemm_wgrad_h2d_kernel, wgrad_bf16_kernel,
wgrad_bf16_dma_kernel), with the plan the library answers for each of them (tests/test_wgrad_cases_cpu.py holds the table to
rcf_conv_plan_of, so that it cannot silently stop reaching a kernel), their seeded operands, and to_planes.

A case is run in up to six variants:
    h2        fp32 operands with their ranges (igemm_wgrad_h2t_kernel), flags 0
    tile128   the same with RCF_CONV_WGRAD_TILE_128 (no 256 x 256 tile)
    noxcd     the same with RCF_CONV_NO_WGRAD_XCD (the plain work-item order); the plan of h2
    planes    both operands as fp16 pair planes (igemm_wgrad_h2d_kernel)
    bf16      16-bit operands, librcf_hip.so
    fp16      16-bit operands, librcf_hip_f16.so; the plan of bf16
The planners refuse no variant of a case listed here (pair planes need Cout >= 64: every fp32 case has it)."""
import ctypes
from collections import namedtuple

import numpy as np
import torch

import rcf_amd  # noqa: F401  (package alias)
from rcf_amd import _lib

H2T, H2D, H16, H16_DMA = _lib.KERNEL_WGRAD_H2T, _lib.KERNEL_WGRAD_H2D, _lib.KERNEL_WGRAD_BF16, _lib.KERNEL_WGRAD_BF16_DMA

# plan: {plan key: (kernel, tile rows, tile cols, split)}; the plan keys are h2, tile128, planes, h16
Case = namedtuple("Case", "name N H W Cin Cout k stride pad dil region plan seed")

F32_VARIANTS = ("h2", "tile128", "noxcd", "planes", "bf16", "fp16")
H16_VARIANTS = ("bf16", "fp16")
PLAN_KEY = {"h2": "h2", "tile128": "tile128", "noxcd": "h2", "planes": "planes", "bf16": "h16", "fp16": "h16"}


def _f32(rows, cols, splits=(1, 1, 1, 1), big=False, h16=None):
    """the four plans of an fp32 case: the same tile everywhere (big: 256 x 256 for h2 alone), h16 = another 16-bit (kernel, rows, cols)"""
    s = splits
    k16 = h16 or (H16_DMA, rows, cols)
    return {"h2": (H2T, 256 if big else rows, 256 if big else cols, s[0]), "tile128": (H2T, rows, cols, s[1]),
            "planes": (H2D, rows, cols, s[2]), "h16": k16 + (s[3],)}


def _h16(kernel, rows, cols, split=1):
    return {"h16": (kernel, rows, cols, split)}


_TABLE = [
    # name, (N, H, W, Cin, Cout, k, stride, pad, dil), region (y0, x0, h, w, band) or None, plan
    ("A", (1, 9, 11, 64, 64, 3, 1, 1, 1), None, _f32(128, 256)),               # several taps per tile, half-empty row tile, dividing walk
    ("X", (1, 3, 5, 64, 64, 3, 1, 1, 1), None, _f32(128, 256)),                # one K-step (M = 15)
    ("Y", (1, 5, 7, 128, 64, 1, 1, 0, 1), None, _f32(128, 128)),               # two to three K-steps, 128 x 128 one tap
    ("B", (2, 12, 17, 256, 256, 3, 1, 2, 2), None, _f32(128, 256, big=True)),  # 256 x 256; advance_rows on fp32 (Wo 17 >= 16), dividing on 16-bit
    ("P", (2, 12, 17, 256, 256, 3, 1, 2, 2), (1, 1, 9, 14, 0), _f32(128, 256, big=True)),     # rectangle, one tap
    ("C", (2, 13, 18, 256, 512, 3, 1, 3, 3), (0, 0, 13, 18, 3), _f32(128, 256, big=True)),    # frame, two row tiles, dilation 3
    ("D", (3, 19, 23, 64, 136, 3, 1, 1, 1), (2, 3, 11, 16, 0), _f32(128, 256)),               # region with several taps per tile, ragged Cout
    ("E", (2, 9, 21, 128, 64, 1, 1, 0, 1), None, _f32(128, 128)),              # 128 x 128, one tap
    ("F", (2, 9, 21, 64, 72, 1, 1, 0, 1), None, _f32(128, 128, h16=(H16, 128, 64))),          # 64 columns in a 128 tile (ragged columns)
    ("G", (2, 17, 35, 64, 128, 3, 2, 1, 1), None, _f32(128, 256)),             # stride 2
    ("H", (2, 9, 33, 192, 136, 1, 1, 0, 1), None, _f32(128, 128)),             # 192 % 128 != 0: ONETAP false; advance_rows on 16-bit (Wo 33)
    ("N", (1, 9, 40, 256, 72, 1, 1, 0, 1), None, _f32(128, 256)),              # ragged rows on the full-width tile, advance_rows everywhere
    ("I", (1, 24, 40, 8, 64, 7, 2, 3, 1), None, _h16(H16_DMA, 128, 256)),      # Cin = 8: per-thread taps in the DMA kernel, the stem
    ("J", (1, 9, 11, 64, 32, 3, 1, 1, 1), None, _h16(H16, 64, 256)),           # the four wgrad_bf16_kernel tiles
    ("K", (1, 9, 11, 128, 32, 1, 1, 0, 1), None, _h16(H16, 64, 128)),
    ("L", (1, 9, 11, 64, 32, 1, 1, 0, 1), None, _h16(H16, 64, 64)),
    ("M", (1, 9, 40, 64, 128, 1, 1, 0, 1), None, _h16(H16, 128, 64)),
    ("O", (4, 30, 40, 64, 64, 3, 1, 1, 1), None, _f32(128, 256, (4, 4, 4, 9))),               # split-K
    ("Q", (4, 24, 34, 256, 256, 3, 1, 2, 2), None, _f32(128, 256, (3, 3, 3, 6), big=True)),   # split-K on the 256 x 256 tile
    ("R", (4, 26, 36, 256, 512, 3, 1, 3, 3), (0, 0, 26, 36, 5), _f32(128, 256, (2, 2, 2, 4), big=True)),   # split-K over a frame
    ("S", (6, 30, 44, 64, 136, 3, 1, 1, 1), (2, 3, 25, 37, 0), _f32(128, 256, (5, 5, 5, 10))),             # split-K over a rectangle
    ("T", (8, 30, 44, 128, 64, 1, 1, 0, 1), None, _f32(128, 128, (10, 10, 10, 20))),          # many splits, few tiles
    ("U", (2, 48, 80, 8, 64, 7, 2, 3, 1), None, _h16(H16_DMA, 128, 256, 3)),   # split-K on the stem shape
    ("V", (4, 30, 44, 64, 32, 3, 1, 1, 1), None, _h16(H16, 64, 256, 10)),      # ... and on the register kernel
    ("W", (8, 30, 44, 64, 128, 1, 1, 0, 1), None, _h16(H16, 128, 64, 20)),
    # regions on the narrow 16-bit tiles (the fp32 planner sends a region on fewer than 256 columns to the tap-as-grid-row kernels):
    # the REGION instances of wgrad_bf16_kernel -- the per-pass dy walkers -- and of the 128 x 128 DMA tile, ONETAP and not
    ("Jr", (1, 9, 11, 64, 32, 3, 1, 1, 1), (1, 1, 6, 8, 0), _h16(H16, 64, 256)),
    ("Kr", (1, 9, 11, 128, 32, 1, 1, 0, 1), (0, 0, 9, 11, 2), _h16(H16, 64, 128)),
    ("Lr", (1, 9, 11, 64, 32, 1, 1, 0, 1), (2, 1, 5, 9, 0), _h16(H16, 64, 64)),
    ("Mr", (1, 9, 40, 64, 128, 1, 1, 0, 1), (0, 0, 9, 40, 1), _h16(H16, 128, 64)),
    ("Er", (2, 9, 21, 128, 64, 1, 1, 0, 1), (1, 2, 7, 17, 0), _h16(H16_DMA, 128, 128)),
    ("Hr", (2, 9, 33, 192, 136, 1, 1, 0, 1), (0, 0, 9, 33, 2), _h16(H16_DMA, 128, 128)),
]
CASES = [Case(name, *shape, region, plan, 7100 + i) for i, (name, shape, region, plan) in enumerate(_TABLE)]


def variants(c):
    return F32_VARIANTS if "h2" in c.plan else H16_VARIANTS


def out_size(n, k, stride, pad, dil):
    return (n + 2 * pad - dil * (k - 1) - 1) // stride + 1


def out_hw(c):
    return out_size(c.H, c.k, c.stride, c.pad, c.dil), out_size(c.W, c.k, c.stride, c.pad, c.dil)


_DUMMY = ctypes.create_string_buffer(64)                      # never read: the plan query launches nothing


def plan_of(c, variant):
    """(kernel, tile rows, tile cols, split) the library of this variant answers for the case"""
    ptr = (ctypes.addressof(_DUMMY) + 15) & ~15
    Ho, Wo = out_hw(c)
    h16 = variant in H16_VARIANTS
    flags = {"tile128": _lib.CONV_WGRAD_TILE_128, "noxcd": _lib.CONV_NO_WGRAD_XCD,
             "planes": _lib.CONV_X_PLANES | _lib.CONV_DY_PLANES}.get(variant, 0)
    ranges = [None] * 8 if h16 else [ptr, None, ptr] + [None] * 5                      # amax_x, amax_w, amax_dy, ...
    s = _lib.ConvShape(c.N, c.H, c.W, c.Cin, Ho, Wo, c.Cout, c.k, c.k, c.stride, c.pad, c.dil, c.Cin, c.Cout, *ranges, flags,
                       ctypes.sizeof(_lib.ConvShape))
    reg = None if c.region is None else ctypes.byref(_lib.ConvRegion(*c.region))
    plan = _lib.ConvPlan()
    lib = _lib.load("f16" if variant == "fp16" else "bf16")
    e = lib.rcf_conv_plan_of(ctypes.byref(s), reg, 2, _lib.BF16 if h16 else _lib.F32, ctypes.byref(plan))
    assert e == 0, f"case {c.name} {variant}: rcf_conv_plan_of refuses the shape ({e})"
    return (plan.kernel, plan.tile_rows, plan.tile_cols, plan.splitk)


def inputs(c):
    """x [N,H,W,Cin], dy [N,Ho,Wo,Cout], dw0 [Cout,k,k,Cin] (what beta = 1 adds to): fp32 CPU tensors of the case's seed"""
    g = torch.Generator().manual_seed(c.seed)
    Ho, Wo = out_hw(c)
    x = torch.randn(c.N, c.H, c.W, c.Cin, generator=g)
    dy = torch.randn(c.N, Ho, Wo, c.Cout, generator=g)
    dw0 = torch.randn(c.Cout, c.k, c.k, c.Cin, generator=g)
    return x, dy, dw0


def to_planes(x, bound_bits):
    """x [N,H,W,C] fp32 on the device -> the fp32-typed pair-plane buffer the kernels read, scaled like they scale: 2^k with
    k = 14 - floor(log2(bound))"""
    b = float(bound_bits.view(torch.float32))
    k = 14 - int(np.floor(np.log2(b)))
    t = x.double() * 2.0 ** k
    h = t.to(torch.float16)
    m = (t - h.double()).to(torch.float16)
    N, H, W, C = x.shape
    pl = torch.stack([h, m], dim=3).contiguous()                    # [N,H,W,2,C] fp16 = [pixel][h | m]
    return pl.view(torch.float32).reshape(N, H, W, C), k
