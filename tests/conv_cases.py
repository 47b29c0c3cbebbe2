"""The cases of tests/test_conv_bits_gpu.py: shapes that reach every instantiation the launchers can select of the forward and
data-gradient conv kernels (csrc/igemm_conv.hip launch_x3 / launch_h2d / launch_mfma and the conv_h2p_kernel pair,
csrc/igemm_bf16.hip launch_cfg), with the plan the library answers for each of them (tests/test_conv_cases_cpu.py holds the
table to rcf_conv_plan_of, directions 0 and 1, so that it cannot silently stop reaching a kernel) and their seeded operands.

A case runs the variants its row lists:
    x3        fp32 operands, no ranges: igemm_conv_x3_kernel on bf16 triples (NP 3)
    h2        both operand ranges: fp16 pairs, the forward splits its weights in the kernel (NP 2, PRE false); the data gradient
              splits them in its own pre-pass (PRE true: a data gradient has no other form)
    pre       ranges and weights split beforehand (ops.weight_pairs / weight_pairs_t): NP 2, PRE true
    natural   pre under RCF_CONV_KORDER_NATURAL (case C: 3x3 with 256 channels per tap, where the chunked order differs)
    nocolmap  pre under RCF_CONV_NO_COLMAP
    lean      pre, the data gradient's lean epilogue: bn_bwd (BST instances), addend, both
    band      pre, dy_band of rcf_conv2d_dgrad_region_band_f32 (the tap-list loop with its BAND term)
    planes    the activation operand as fp16 pair planes (wgrad_cases.to_planes): conv_h2d_kernel (whole K-steps inside a tap:
              channel counts in multiples of 16, so not the ragged cases D and E)
    leanp     planes, the lean epilogue (conv_h2d_kernel's BST instances)
    h2p       pre under RCF_CONV_H2P_ALWAYS: conv_h2p_kernel, forward with fused statistics and data gradient
    mfma0..3  RCF_CONV_FP32_MFMA(v): igemm_conv_kernel
    bf16      16-bit operands, librcf_hip.so: conv_bf16_kernel with 16-bit and fp32 output, bias, statistics, the affine forward
              (EP 1) and the masked data gradient from the tensor and from the forward's bits (EP 2, 3)
    fp16      the same in librcf_hip_f16.so; the plan of bf16

Which case reaches what (tile = rows x columns; forward columns = Cout, data-gradient columns = Cin):
    igemm_conv_x3_kernel, each in the three operand forms x3 / h2 / pre
        64 x 64      A (forward, data gradient), G (strided data gradient), Af (tap list, both directions), band on A
        128 x 64     L (forward, data gradient, lean), Ls (strided, lean strided), Lf (tap list, both directions)
        128 x 128    B (forward, data gradient), G2 (strided), Bf (tap list), band on B; ragged columns: E (Cout 72)
        128 x 256    C (forward, data gradient), G4 (strided), Cf (tap list), band on C and Cf; ragged columns: D (Cout 136)
        lean (BST)   A, B, C, L plain; G, G2, G4, Ls strided.  The BST tap-list instances are compiled, but no entry point
                     selects them: rcf_conv2d_dgrad_add_f32 passes neither a region nor a source band.
        pointwise    E (1x1, whole tensor); its negation Er (1x1 on a rectangle) and Ep (1x1 with a pitch wider than C)
        K order      C natural against C pre;  column map off: B nocolmap
        GEMM         GEMM (rcf_gemm_nt_f32: x3, h2, b_pairs, bias + GELU, amax_out), BGEMM (rcf_gemm_nt_batched_f32)
    conv_h2d_kernel  NR 1: A, Af, G (strided);  NR 2: B, Bf, G2 (strided);  NR 4: C, Cf, G4 (strided);  BST: leanp on
                     A, B, C plain and G, G2, G4 strided
    conv_h2p_kernel  C and Cr: forward with fused statistics, data gradient
    igemm_conv_kernel   narrow: A (forward, data gradient), G (strided);  wide: B (forward, data gradient), G2 (strided); v = 0..3
    conv_bf16_kernel (bf16 and fp16)   64 columns: A, Af, D (data gradient, rectangle), G (strided);  128: B, Bf, E, G2 (strided);
                     256: C, Cf, D (forward, ragged), G4 (strided);  EP 1 / 2 / 3: A, B, C

Every run is made at beta = 0 into a NaN-filled output and at beta = 1 onto a seeded one wherever its entry point takes beta."""
import ctypes
from collections import namedtuple

import torch

import rcf_amd  # noqa: F401  (package alias)
from rcf_amd import _lib

TILE, H2D, H2P, MFMA, H16 = _lib.KERNEL_TILE, _lib.KERNEL_H2D, _lib.KERNEL_H2P, _lib.KERNEL_MFMA, _lib.KERNEL_BF16

# plan: {plan key: ((kernel, rows, cols) forward, (kernel, rows, cols) data gradient)}
Case = namedtuple("Case", "name N H W Cin Cout k stride pad dil region pitch variants plan seed")

MFMAS = ("mfma0", "mfma1", "mfma2", "mfma3")
H16_VARIANTS = ("bf16", "fp16")
PLAN_KEY = {"x3": "tile", "h2": "tile", "pre": "tile", "natural": "tile", "nocolmap": "tile", "lean": "tile", "band": "tile",
            "planes": "h2d", "leanp": "h2d", "h2p": "h2p", "bf16": "h16", "fp16": "h16", **{m: "mfma" for m in MFMAS}}
FLAGS = {"natural": _lib.CONV_KORDER_NATURAL, "nocolmap": _lib.CONV_NO_COLMAP, "h2p": _lib.CONV_H2P_ALWAYS,
         **{m: _lib.CONV_FP32_MFMA(i) for i, m in enumerate(MFMAS)}}


def _plan(fwd, dgrad):
    """the plans of a case from the tile of igemm_conv_x3_kernel in each direction: conv_h2d_kernel and conv_bf16_kernel have 128
    rows and the same columns, igemm_conv_kernel 128 x 64 or 128 x 128, conv_h2p_kernel 32-row blocks x 256"""
    both = lambda f: (f(fwd), f(dgrad))
    return {"tile": both(lambda t: (TILE,) + t), "h2d": both(lambda t: (H2D, 128, t[1])), "h2p": both(lambda t: (H2P, 32, 256)),
            "mfma": both(lambda t: (MFMA, 128, min(t[1], 128))), "h16": both(lambda t: (H16, 128, t[1]))}


F32 = ("x3", "h2", "pre")
ALL = F32 + ("planes",) + H16_VARIANTS
S64, S128, S256, L64 = (64, 64), (128, 128), (128, 256), (128, 64)

_TABLE = [
    # name, (N, H, W, Cin, Cout, k, stride, pad, dil), region (y0, x0, h, w, band) or None, pitched, variants, plan
    ("A", (2, 9, 11, 64, 64, 3, 1, 1, 1), None, False, ALL + ("lean", "leanp", "band") + MFMAS, _plan(S64, S64)),      # rows cross an image, ragged last tile
    ("B", (2, 12, 17, 128, 128, 3, 1, 2, 2), None, False, ALL + ("lean", "leanp", "band", "nocolmap") + MFMAS, _plan(S128, S128)),   # dilation 2, rows past M
    ("C", (2, 13, 18, 256, 256, 3, 1, 3, 3), None, False, ALL + ("lean", "leanp", "band", "natural", "h2p"), _plan(S256, S256)),     # dilation 3, K = 2304
    ("Cr", (2, 13, 18, 256, 256, 3, 1, 3, 3), (1, 2, 10, 13, 0), False, ("pre", "h2p"), _plan(S256, S256)),            # rectangle on the persistent kernel
    ("Af", (2, 13, 18, 64, 64, 3, 1, 1, 1), (0, 0, 13, 18, 2), False, ALL, _plan(S64, S64)),                          # frames: the tap-list loop
    ("Bf", (2, 13, 18, 128, 128, 3, 1, 2, 2), (0, 0, 13, 18, 3), False, ALL, _plan(S128, S128)),
    ("Cf", (2, 13, 18, 256, 256, 3, 1, 3, 3), (0, 0, 13, 18, 3), False, ALL + ("band",), _plan(S256, S256)),
    ("D", (3, 19, 23, 64, 136, 3, 1, 1, 1), (2, 3, 11, 16, 0), False, F32 + H16_VARIANTS, _plan(S256, S64)),           # rectangle, ragged columns (136)
    ("E", (2, 9, 21, 128, 72, 1, 1, 0, 1), None, False, F32 + H16_VARIANTS, _plan(S128, S128)),                      # pointwise, ragged columns (72)
    ("Er", (2, 9, 21, 128, 72, 1, 1, 0, 1), (1, 2, 7, 17, 0), False, F32, _plan(S128, S128)),                         # 1x1 on a rectangle
    ("Ep", (2, 9, 21, 128, 72, 1, 1, 0, 1), None, True, F32 + H16_VARIANTS, _plan(S128, S128)),                       # 1x1, pitch wider than C
    ("G", (2, 17, 35, 64, 128, 3, 2, 1, 1), None, False, ALL + ("lean", "leanp") + MFMAS, _plan(S128, S64)),          # stride 2: strided data gradient
    ("G2", (2, 17, 35, 128, 256, 3, 2, 1, 1), None, False, ALL + ("lean", "leanp") + MFMAS, _plan(S256, S128)),
    ("G4", (1, 18, 22, 256, 64, 1, 2, 0, 1), None, False, ALL + ("lean", "leanp"), _plan(S64, S256)),
    # the fp32 128 x 64 tile: at least 512 row tiles of 128 on at most 64 columns (plan_conv takes 64 x 64 below that)
    ("L", (1, 256, 256, 64, 64, 1, 1, 0, 1), None, False, F32 + ("lean",), _plan(L64, L64)),
    ("Ls", (1, 256, 256, 64, 64, 3, 2, 1, 1), None, False, F32 + ("lean",), _plan(S64, L64)),
    ("Lf", (1, 320, 320, 16, 64, 3, 1, 1, 1), (0, 0, 320, 320, 64), False, F32, _plan(L64, L64)),
]
CASES = [Case(name, *shape, region, pitch, variants, plan, 8100 + i) for i, (name, shape, region, pitch, variants, plan) in enumerate(_TABLE)]

# the GEMM entry points (no rcf_conv_shape, so no plan query): M, N, K of rcf_gemm_nt_f32; batch, M, N, K of rcf_gemm_nt_batched_f32
GEMM = dict(M=300, N=136, K=96, seed=8201)
BGEMM = dict(batch=(2, 3), M=70, N=40, K=32, seed=8202)


def out_size(n, k, stride, pad, dil):
    return (n + 2 * pad - dil * (k - 1) - 1) // stride + 1


def out_hw(c):
    return out_size(c.H, c.k, c.stride, c.pad, c.dil), out_size(c.W, c.k, c.stride, c.pad, c.dil)


_DUMMY = ctypes.create_string_buffer(64)                      # never read: the plan query launches nothing


def plan_of(c, variant, direction):
    """(kernel, tile rows, tile cols) the library of this variant answers for the case; direction 0 forward, 1 data gradient"""
    ptr = (ctypes.addressof(_DUMMY) + 15) & ~15
    Ho, Wo = out_hw(c)
    h16 = variant in H16_VARIANTS
    flags = FLAGS.get(variant, 0)
    ranges = [None] * 8
    if not h16 and variant != "x3" and variant not in MFMAS:
        ranges[1] = ptr                                                                 # amax_w
        ranges[2 if direction else 0] = ptr                                             # amax_dy / amax_x
        if variant != "h2":
            ranges[6 if direction else 5] = ptr                                         # w_pairs2_t / w_pairs2
        if variant in ("planes", "leanp"):
            flags |= _lib.CONV_DY_PLANES if direction else _lib.CONV_X_PLANES
    s = _lib.ConvShape(c.N, c.H, c.W, c.Cin, Ho, Wo, c.Cout, c.k, c.k, c.stride, c.pad, c.dil, c.Cin, c.Cout, *ranges, flags,
                       ctypes.sizeof(_lib.ConvShape))
    reg = None if c.region is None else ctypes.byref(_lib.ConvRegion(*c.region))
    plan = _lib.ConvPlan()
    lib = _lib.load("f16" if variant == "fp16" else "bf16")
    e = lib.rcf_conv_plan_of(ctypes.byref(s), reg, direction, _lib.BF16 if h16 else _lib.F32, ctypes.byref(plan))
    assert e == 0, f"case {c.name} {variant} direction {direction}: rcf_conv_plan_of refuses the shape ({e})"
    return (plan.kernel, plan.tile_rows, plan.tile_cols)


PITCH_EXTRA = 32                                              # channels beside the operand's own in a pitched case


def inputs(c):
    """fp32 CPU tensors of the case's seed: x [N,H,W,Cin], w [Cout,Cin,k,k] (channels_last), dy and y0 [N,Ho,Wo,Cout], dx0
    [N,H,W,Cin] (y0 / dx0: what beta = 1 adds to), bias [Cout], chan [4][max(Cin, Cout)] (per-channel constants), and two
    ReLU bit masks over x's shape ([N H W Cin / 4] bytes, four channels per byte).  pitch: x and dy come PITCH_EXTRA channels
    wider; the operand is the slice [..., :Cin] / [..., :Cout] of the buffer once it is on the device."""
    g = torch.Generator().manual_seed(c.seed)
    Ho, Wo = out_hw(c)
    wide = PITCH_EXTRA if c.pitch else 0
    x = torch.randn(c.N, c.H, c.W, c.Cin + wide, generator=g)
    dy = torch.randn(c.N, Ho, Wo, c.Cout + wide, generator=g)
    w = (torch.randn(c.Cout, c.Cin, c.k, c.k, generator=g) / (c.Cin * c.k * c.k) ** 0.5).contiguous(memory_format=torch.channels_last)
    y0 = torch.randn(c.N, Ho, Wo, c.Cout, generator=g)
    dx0 = torch.randn(c.N, c.H, c.W, c.Cin, generator=g)
    bias = torch.randn(c.Cout, generator=g)
    chan = torch.rand(4, max(c.Cin, c.Cout), generator=g) + 0.5
    masks = torch.randint(0, 16, (2, c.N * c.H * c.W * c.Cin // 4), generator=g, dtype=torch.uint8)
    return dict(x=x, dy=dy, w=w, y0=y0, dx0=dx0, bias=bias, chan=chan, masks=masks)
