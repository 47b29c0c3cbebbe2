"""Edge-geometry cases of the ViT / soft-NCut family (csrc/attention.hip, csrc/vit.hip, the GEMM entry points of
csrc/igemm_conv.hip) and their references.

Shared by tests/test_vit_sweep_cpu.py (the tables reach the geometry they name; every reference's own float32 run sits within
a quarter of its floor) and tests/test_vit_sweep_gpu.py (the kernels against the float64 truth).  The references are plain
torch on the CPU, written once and run in float64 (truth) and float32 (conditioning); nothing of the HIP package enters this
module.

Kernel constants restated below to CHOOSE shapes (never as a reference for a value):
  attention_fwd_kernel   BQ = 128 queries per workgroup, 32 per wavefront, BKEY = 64 keys per tile, head dimension 64
  plan_conv              64x64 tiles when N <= 64 and cdiv(M, 128) * batches < 512, else 128 rows x (64 | 128 | 256) columns for
                         N <= 64 | N <= 128 | N > 128; K walked in steps of 16 (K % 4 == 0 is all the entry asks)
  softmax_rows_kernel    rows held in registers when pitch % 4 == 0 and pitch <= 256 * 4 * SM_QMAX = 8192, else three passes
  layernorm_kernel       one wavefront per row, four rows per workgroup, 8 float4 per lane: C <= 2048
  l2_normalize_rows      one wavefront per row, a lane walks columns lane, lane + 64, ..
  matvec / ncut          one workgroup (256 threads) per row; one workgroup for the value and the gradient

What the store epilogue of igemm_conv_x3_kernel does with N % 4 != 0 (read before the N = 97 case was written): the last
quad of a row is stored element by element, `if (c + e < p.Ncol)`, so columns [N, ldc) are NOT written.  include/rcf_hip.h
promises nothing about them; ncut.py and vit.py hand the GEMM padded matrices and overwrite the pad themselves
(rcf_softmax_rows_f32 zeroes it, rcf_affinity_threshold_f32 and the mat-vec never read it).  The sweep pins that behaviour:
every column from N on keeps its fill.

The pre-split GEMM case: h2p_eligible needs b_pairs2 (the plane-separated K-step blocks of rcf_conv_weight_pairs2_f32), and
rcf_gemm_nt_f32 never sets it -- conv_h2p_kernel (the persistent kernel) admits NO GEMM.  (40, 256, 32) pre-split therefore
runs the 128x256 tile kernel with PRE = true, and that is what its row of the table names.

Attention logit kinds (base magnitude |qkv| ~ 1.5; a case at magnitude m multiplies qkv by m / 1.5 and the scale by
(1.5 / m)^2, so the logits are the same numbers, as test_fused_attention_vs_float64 does):
  rand    normal q, k, v; scale 1/8
  ramp    q and k along one +-1 direction per head, k_j growing with j and stepping up at every 64th key: the logit rises with
          the key index and every tile raises every query's running maximum by more than a binade (alpha < 1/2 on every tile
          after the first, even a last tile of one key: the LDS row hand-off carries a real rescale)
  peak    rand at scale 1/2: a few keys carry a row
  first   the keys of tile 0 along the query direction, every later key against it: the maximum sits in tile 0 and every
          later tile is >= 100 lower in the log2 domain (exp2 underflows, alpha = 1, the tile adds nothing)
"""
import dataclasses
import functools
import math

import pytest
import torch

FILL = 7.0                       # what guard columns and untouched buffers hold
TAU, AFF_EPS = 0.2, 1e-5
LN_EPS = 1e-6

# floors: the project's own (tests/test_vit_gpu.py: 2e-5 attention / bf16-triple GEMM / layernorm / softmax, 2e-6 the fp16-pair
# linear with ranges, 1e-5 the NCut value).  FLOOR_NCUT_GRAD is derived: 4 x the float32 oracle's worst error over the final
# table (3.2e-6 of max |grad| at n = 257, profiles/vit_sweep_parity.txt: 1.3e-5), rounded up to one digit.
FLOOR, FLOOR_H2, FLOOR_NCUT, FLOOR_NCUT_GRAD = 2e-5, 2e-6, 1e-5, 2e-5

BQ, BKEY, HD = 128, 64, 64
SM_QMAX = 8
SM_FAST_CAP = 256 * 4 * SM_QMAX
KSTEP = 16


def cdiv(a, b):
    return -(-a // b)


def rel(got, ref):
    """max error / max |ref|, the measure of tests/test_vit_gpu.py; a NaN anywhere gives inf"""
    got, ref = got.double(), ref.double()
    e = (got - ref).abs().max() / ref.abs().max().clamp_min(1e-300)
    return float("inf") if bool(torch.isnan(e)) else float(e)


def _gen(*key):
    return torch.Generator().manual_seed(sum((i + 1) * 7919 * int(k) for i, k in enumerate(key)) % (2 ** 31))


# ------------------------------------------------------------------------------------------------------------ attention
KINDS = ("rand", "ramp", "peak", "first")
BASE_SCALE = {"rand": 0.125, "ramp": 0.125, "peak": 0.5, "first": 0.5}


@dataclasses.dataclass(frozen=True)
class Attn:
    T: int
    B: int
    nh: int
    kind: str
    why: str
    arith: str = "x3"         # "x3": bf16 triples; "h2": fp16 pairs (amax_qkv given)
    mag: float = 1.5          # |qkv|
    pitched: bool = False     # qkv = columns [4 : 4 + 3 dim] of a buffer 3 dim + 8 wide, out = [4 : 4 + dim] of one dim + 8 wide

    @property
    def name(self):
        return f"T{self.T}-b{self.B}h{self.nh}-{self.kind}-{self.arith}-{self.mag:g}" + ("-pitched" if self.pitched else "")

    @property
    def dim(self):
        return self.nh * HD

    @property
    def scale(self):
        return BASE_SCALE[self.kind] * (1.5 / self.mag) ** 2


ATTN = [
    Attn(1, 1, 1, "rand", "one token: softmax of one logit, 127 idle queries, 63 masked keys, B = nh = 1"),
    Attn(31, 2, 3, "rand", "fewer queries than one wavefront"),
    Attn(32, 1, 1, "rand", "exactly one wavefront of queries, half a key tile"),
    Attn(33, 2, 3, "rand", "the second wavefront has one query, the third and fourth none"),
    Attn(64, 2, 3, "rand", "one whole key tile: key < T is all-true, no key is masked"),
    Attn(64, 1, 1, "peak", "a whole key tile under sharp rows"),
    Attn(65, 2, 3, "rand", "one real key in the second tile"),
    Attn(65, 1, 1, "first", "the one key of the second tile underflows"),
    Attn(127, 1, 1, "rand", "one query short of a workgroup, one key short of two tiles"),
    Attn(128, 2, 3, "rand", "one whole workgroup of queries, two whole key tiles"),
    Attn(128, 1, 1, "ramp", "two whole tiles, the second raises every running maximum"),
    Attn(129, 2, 3, "ramp", "a second workgroup with one query; one real key in the third tile, and it is the largest"),
    Attn(129, 1, 1, "first", "two later tiles underflow, the last holds one key"),
    Attn(193, 2, 3, "ramp", "four tiles, the maximum rises in each; the last holds one key"),
    Attn(193, 1, 1, "peak", "four tiles, sharp rows"),
    Attn(193, 2, 3, "first", "three later tiles underflow"),
    Attn(64, 1, 1, "rand", "ld_qkv = 3 dim + 8, ld_out = dim + 8, whole tile", pitched=True),
    Attn(129, 2, 3, "rand", "pitched, two workgroups, three tiles, B and nh > 1", pitched=True),
    Attn(64, 2, 3, "rand", "fp16 pairs, whole tile", "h2"),
    Attn(65, 1, 1, "ramp", "fp16 pairs, the second tile's one key is the maximum", "h2"),
    Attn(193, 2, 3, "first", "fp16 pairs, later tiles underflow", "h2"),
    Attn(127, 2, 3, "rand", "fp16 pairs, pitched", "h2", pitched=True),
    Attn(33, 2, 3, "rand", "fp16 pairs at |qkv| ~ 3e-4", "h2", 3e-4),
    Attn(128, 1, 1, "ramp", "fp16 pairs at |qkv| ~ 3e-4, rising maximum", "h2", 3e-4),
    Attn(1, 1, 1, "rand", "fp16 pairs at |qkv| ~ 2e3, one token", "h2", 2e3),
    Attn(129, 2, 3, "peak", "fp16 pairs at |qkv| ~ 2e3, sharp rows", "h2", 2e3),
    Attn(193, 1, 1, "first", "fp16 pairs at |qkv| ~ 2e3, later tiles underflow", "h2", 2e3),
]
ATTN_PARAMS = [pytest.param(c, id=c.name) for c in ATTN]


@functools.lru_cache(maxsize=None)
def attn_qkv(c):
    """float32 [B T, 3 dim] (q | k | v, heads side by side): the stored values"""
    g = _gen(c.T, c.B, c.nh, KINDS.index(c.kind), c.arith == "h2", c.pitched, round(math.log10(c.mag) * 10) + 100)
    B, T, nh = c.B, c.T, c.nh
    rnd, uni = (lambda *s: torch.randn(*s, generator=g, dtype=torch.float64)), (lambda *s: torch.rand(*s, generator=g, dtype=torch.float64))
    q, k, v = 1.5 * rnd(B, nh, T, HD), 1.5 * rnd(B, nh, T, HD), 1.5 * rnd(B, nh, T, HD)
    if c.kind in ("ramp", "first"):
        u = torch.sign(rnd(B, nh, 1, HD))
        if c.kind == "ramp":
            q = 1.5 * u * (0.5 + uni(B, nh, T, 1)) + 0.1 * rnd(B, nh, T, HD)
            j = torch.arange(T, dtype=torch.float64)
            k = 1.5 * u * (0.4 * (j + 1) / T + 0.15 * (j // BKEY)).view(1, 1, T, 1) + 0.03 * rnd(B, nh, T, HD)    # a step up at every tile
        else:
            q = 1.5 * u * (0.8 + 0.4 * uni(B, nh, T, 1)) + 0.1 * rnd(B, nh, T, HD)
            late = -1.5 * u * (1.5 + 0.5 * uni(B, nh, T, 1))
            early = 1.5 * u * (0.1 + 0.05 * uni(B, nh, T, 1))
            k = torch.where((torch.arange(T) < BKEY).view(1, 1, T, 1), early, late) + 0.1 * rnd(B, nh, T, HD)
    x = torch.stack([q, k, v]).permute(1, 3, 0, 2, 4).reshape(B * T, 3 * c.dim)
    return (x * (c.mag / 1.5)).float()


def attn_logits(c, dtype=torch.float64):
    """[B, nh, T, T] scale q k^T"""
    x = attn_qkv(c).to(dtype).view(c.B, c.T, 3, c.nh, HD).permute(2, 0, 3, 1, 4)
    return x[0] @ x[1].transpose(-2, -1) * c.scale


def attn_ref(c, dtype):
    x = attn_qkv(c).to(dtype).view(c.B, c.T, 3, c.nh, HD).permute(2, 0, 3, 1, 4)
    p = torch.softmax(x[0] @ x[1].transpose(-2, -1) * c.scale, dim=-1)
    return (p @ x[2]).transpose(1, 2).reshape(c.B * c.T, c.dim)


# ----------------------------------------------------------------------------------------------------------------- GEMM
@dataclasses.dataclass(frozen=True)
class Gemm:
    name: str
    M: int
    N: int
    K: int
    tile: tuple               # what plan_conv picks (checked by the CPU test from the restated rule)
    why: str
    variants: tuple = ("x3", "h2", "pre")
    ldc: int = 0              # 0: the output is columns [4 : 4 + N] of a buffer roundup4(N) + 8 wide; else columns [0 : N] of one ldc wide
    pitched: bool = False     # a = columns [4 : 4 + K] of a buffer K + 8 wide, b likewise (pre: b dense, it needs ldb == K)
    bias: bool = False
    act: int = 0              # 2: GELU(erf)
    beta: int = 0


GEMM = [
    Gemm("smallest", 5, 4, 4, (64, 64), "K = 4: one partial K-step and nothing else"),
    Gemm("ktail12", 130, 36, 28, (64, 64), "64x64 tiles; the last row tile has 2 rows; K % 16 = 12"),
    Gemm("ktail4", 70, 68, 52, (128, 128), "128x128 tile; ragged columns; K % 16 = 4"),
    Gemm("wide", 129, 260, 32, (128, 256), "128x256 tiles; the second column tile is 4 wide, the second row tile has 1 row"),
    Gemm("odd_n", 33, 97, 64, (128, 128), "N % 4 != 0 with ldc = 100: the last quad is stored by element, columns 97..99 keep their fill", ldc=100),
    Gemm("presplit", 40, 256, 32, (128, 256), "whole 256-column tile: the lean epilogue (fp16 pairs); pre-split weights on the tile kernel -- "
         "conv_h2p_kernel admits no GEMM (no b_pairs2)"),
    Gemm("tall", 65409, 8, 4, (128, 64), "cdiv(M, 128) = 512: the 128x64 tile; the last row tile has 1 row", variants=("x3", "h2")),
    Gemm("pitched", 67, 72, 40, (128, 128), "every operand a pitched slice, bias + GELU, beta = 1, amax_out; K % 16 = 8", pitched=True,
         bias=True, act=2, beta=1),
]
GEMM_BY_NAME = {c.name: c for c in GEMM}
# (a, b) magnitudes; b is further divided by sqrt(K).  The fp16-pair variant with ranges also runs at 3e-4 and 2e3.
MAG_ONE, MAGS_H2 = (1.0, 1.0), ((3e-4, 3e-4), (2e3, 2e3))
GEMM_RUNS = [(c, v, MAG_ONE) for c in GEMM for v in c.variants] + [(c, "h2", m) for c in GEMM if c.name != "tall" for m in MAGS_H2]
GEMM_PARAMS = [pytest.param(c, v, m, id=f"{c.name}-{v}-{m[0]:g}") for c, v, m in GEMM_RUNS]


def gemm_tile(M, N, batches=1):
    """plan_conv's tile rule for the default kernels (to name a case's tile class)"""
    if N <= 64 and cdiv(M, 128) * batches < 512:
        return (64, 64)
    return (128, 64 if N <= 64 else (256 if N > 128 else 128))


def gemm_floor(variant):
    return FLOOR if variant == "x3" else FLOOR_H2


@functools.lru_cache(maxsize=4)
def gemm_inputs(name, mag):
    c = GEMM_BY_NAME[name]
    g = _gen(c.M, c.N, c.K, 17)
    ma, mb = mag
    a = ((torch.randn(c.M, c.K, generator=g) + 0.5) * ma).float()                      # the offsets: a mean of sqrt(K) / 4 under the noise,
    b = ((torch.randn(c.N, c.K, generator=g) + 0.5) * (mb / c.K ** 0.5)).float()       # which halves the float32 oracle's share of max |ref|
    bias = (torch.randn(c.N, generator=g) * (ma * mb)).float()
    c0 = (torch.randn(c.M, c.N, generator=g) * (ma * mb)).float()
    return a, b, bias, c0


def gemm_ref(c, mag, dtype):
    a, b, bias, c0 = (t.to(dtype) for t in gemm_inputs(c.name, mag))
    y = a @ b.T
    if c.bias:
        y = y + bias
    if c.act == 2:
        y = torch.nn.functional.gelu(y)
    return y + c0 if c.beta else y


# the batched entry.  "vit": the ViT's own two products at T = 37, nh = 2, B = 2 out of one [B T, 3 dim] buffer -- S = q k^T (head
# stride 64, N = 37 into rows of pitch Tp = 40) and P V from transpose2d's [dim][Tp] output (K = Tp = 40: K % 16 = 8, the pad
# columns of P and V^T are zero).  "beta": a (3, 2) batch with K = 20 (K % 16 = 4) accumulating into its output.
BG_VIT = dict(T=37, nh=2, B=2, Tp=40)
BG_BETA = dict(batch=(3, 2), M=33, N=36, K=20)


@functools.lru_cache(maxsize=1)
def bg_vit_inputs():
    q = BG_VIT
    g = _gen(q["T"], q["nh"], q["B"], 23)
    qkv = torch.randn(q["B"] * q["T"], 3 * q["nh"] * HD, generator=g).float()
    x = qkv.double().view(q["B"], q["T"], 3, q["nh"], HD).permute(2, 0, 3, 1, 4)            # [3][B][nh][T][64]
    P = torch.softmax(x[0] @ x[1].transpose(-2, -1) * 0.125, dim=-1).float()                  # the stored probabilities
    return qkv, P


def bg_vit_ref(dtype):
    qkv, P = bg_vit_inputs()
    q = BG_VIT
    x = qkv.to(dtype).view(q["B"], q["T"], 3, q["nh"], HD).permute(2, 0, 3, 1, 4)
    S = x[0] @ x[1].transpose(-2, -1)                                                         # [B][nh][T][T]
    O = (P.to(dtype) @ x[2]).transpose(1, 2).reshape(q["B"] * q["T"], q["nh"] * HD)
    return S, O


@functools.lru_cache(maxsize=1)
def bg_beta_inputs():
    q = BG_BETA
    (b0, b1), M, N, K = q["batch"], q["M"], q["N"], q["K"]
    g = _gen(b0, b1, M, N, K)
    return (torch.randn(b0, b1, M, K, generator=g).float(), (torch.randn(b0, b1, N, K, generator=g) / K ** 0.5).float(),
            torch.randn(b0, b1, M, N, generator=g).float())


def bg_beta_ref(dtype):
    a, b, c0 = (t.to(dtype) for t in bg_beta_inputs())
    return a @ b.transpose(-2, -1) + c0


# ------------------------------------------------------------------------------------------------------------ layernorm
# (rows, C).  Rows 1 and 2 of a case with >= 5 rows are special: row 1 is constant (variance 0: the output is beta, exactly),
# row 2 is LN_BIG_MEAN + 1e-2 normal.  LN_BIG_MEAN: at 1000 the float32 oracle is 3.4e-3 of max |y| off its float64 run (one
# ulp of the stored values is 6e-5 against a spread of 1e-2, and the float32 mean is no better), at 100 3.0e-4, at 10 3.5e-5;
# at 1 3.8e-6 -- inside the quarter floor, with little left for another host's summation order; the mean was reduced to 0.5 (1.2e-6,
# worst of the table).
LN_BIG_MEAN = 0.5
LN = [(1, 4), (5, 4), (5, 252), (8, 256), (1, 260), (5, 260), (5, 384), (8, 384), (1, 2048), (5, 2048)]
LN_WHY = {4: "one quad: lane 0 alone holds data", 252: "63 quads: one idle lane", 256: "exactly 64 quads: one per lane",
          260: "65 quads: lane 0 holds two", 384: "the ViT-S width", 2048: "the cap: 8 quads on every lane"}
LN_PARAMS = [pytest.param(r, C, id=f"{r}x{C}") for r, C in LN]
LN_CONST = 3.25


@functools.lru_cache(maxsize=None)
def ln_inputs(rows, C):
    g = _gen(rows, C, 31)
    x = torch.randn(rows, C, generator=g) * torch.exp2(4 * torch.rand(rows, 1, generator=g) - 2) + torch.randn(rows, 1, generator=g)
    if rows >= 5:
        x[1] = LN_CONST
        x[2] = LN_BIG_MEAN + 1e-2 * torch.randn(C, generator=g)
    return x.float(), torch.randn(C, generator=g).float(), torch.randn(C, generator=g).float()


def ln_ref(rows, C, dtype):
    x, gamma, beta = (t.to(dtype) for t in ln_inputs(rows, C))
    mean = x.mean(-1, keepdim=True)
    d = x - mean
    var = (d * d).mean(-1, keepdim=True)                               # biased, like nn.LayerNorm
    return d / torch.sqrt(var + LN_EPS) * gamma + beta


# -------------------------------------------------------------------------------------------------------------- softmax
# (pitch, n), three rows each: row 0 normal, row 1 all equal, row 2 spread over +-80 after scaling (both ends present)
SM = [(4, 1), (4, 3), (100, 97), (1028, 1025), (8192, 8190), (8196, 8193), (99, 97), (1030, 1027)]
SM_SCALES = (0.125, -0.125)
SM_PARAMS = [pytest.param(p, n, s, id=f"{p}-{n}-{s:g}") for p, n in SM for s in SM_SCALES]
SM_EQUAL = 5.0


def sm_fast(pitch):
    return pitch % 4 == 0 and pitch <= SM_FAST_CAP


@functools.lru_cache(maxsize=None)
def sm_inputs(n):
    g = _gen(n, 41)
    x = torch.empty(3, n)
    x[0] = 16 * torch.randn(n, generator=g)
    x[1] = SM_EQUAL
    x[2] = 1280 * torch.rand(n, generator=g) - 640
    x[2, 0] = 640.0
    if n > 1:
        x[2, 1] = -640.0
    return x.float()


def sm_ref(n, scale, dtype):
    return torch.softmax(sm_inputs(n).to(dtype) * scale, dim=-1)


# ------------------------------------------------------------------------------------------------------------ transpose
TR = [(1, 1, 1), (32, 32, 32), (31, 33, 31), (33, 31, 40), (97, 64, 100), (65, 5, 200)]        # (rows, cols, dpitch)
TR_PARAMS = [pytest.param(*t, id="x".join(map(str, t))) for t in TR]

# ------------------------------------------------------------------------------------------------------- l2_normalize_rows
# six rows (the second workgroup holds two): 0 normal, 1 zero (-> zeros), 2 of norm 1e-20 (-> divided by 1e-12), 3 at 1e3, 4 and 5 normal
L2_C = (1, 63, 64, 65, 384)
L2_ROWS, L2_TINY = 6, 1e-20


@functools.lru_cache(maxsize=None)
def l2_inputs(C):
    g = _gen(C, 53)
    x = torch.randn(L2_ROWS, C, generator=g, dtype=torch.float64)
    x[1] = 0.0
    x[2] = x[2] / x[2].norm() * L2_TINY
    x[3] *= 1e3
    return x.float()


def l2_ref(C, dtype):
    x = l2_inputs(C).to(dtype)
    return x / torch.sqrt((x * x).sum(-1, keepdim=True)).clamp_min(1e-12)


def row_rel(got, ref):
    """worst per-row max error / max |ref row|; a row whose reference is all zero must be all zero"""
    got, ref = got.double(), ref.double()
    worst = 0.0
    for a, b in zip(got, ref):
        m = float(b.abs().max())
        e = float((a - b).abs().max())
        worst = max(worst, (0.0 if e == 0.0 else float("inf")) if m == 0.0 else e / m) if e == e else float("inf")
    return worst


# ------------------------------------------------------------------------------------------------------- affinity_threshold
AFF = [(n, n + d) for n in (1, 5, 257) for d in (0, 3)]                                       # (n, pitch)
AFF_PARAMS = [pytest.param(n, p, id=f"{n}-{p}") for n, p in AFF]


def aff_inputs(n):
    """float32 [n, n] in [-1, 1] with the edge values planted (n >= 5: tau, its two float32 neighbours, NaN, +inf in row 0, -inf
    below; n = 1: tau itself), and what the threshold makes of it (strict >, a NaN is not greater)"""
    g = _gen(n, 61)
    x = (2 * torch.rand(n, n, generator=g) - 1).float()
    tau = torch.tensor(TAU, dtype=torch.float32)
    x[0, 0] = tau
    if n >= 5:
        x[0, 1], x[0, 2] = torch.nextafter(tau, torch.tensor(math.inf)), torch.nextafter(tau, torch.tensor(-math.inf))
        x[0, 3], x[0, 4], x[1, 0] = math.nan, math.inf, -math.inf
    want = torch.where(x > tau, torch.tensor(1.0), torch.tensor(AFF_EPS, dtype=torch.float32))
    return x, want


# ---------------------------------------------------------------------------------------------------------- ncut_value_grad
NCUT = [(n, n + d) for n in (2, 63, 64, 257, 1030) for d in (0, 2)]                           # (n, pitch)
NCUT_WHY = {2: "254 idle threads in every reduction", 63: "one lane short of a wavefront", 64: "exactly one wavefront",
            257: "the stride loops' second trip holds one element", 1030: "five trips, the last with 6 elements"}
NCUT_PARAMS = [pytest.param(n, p, id=f"{n}-{p}") for n, p in NCUT]


@functools.lru_cache(maxsize=None)
def ncut_inputs(n):
    """symmetric affinity of {1, eps} with a unit diagonal (float32 [n, n]), x uniform in (0.05, 0.95)"""
    g = _gen(n, 71)
    up = torch.triu(torch.rand(n, n, generator=g) > 0.7, 1)
    A = torch.where(up | up.T | torch.eye(n, dtype=torch.bool), torch.tensor(1.0), torch.tensor(AFF_EPS, dtype=torch.float32))
    return A, (0.05 + 0.9 * torch.rand(n, generator=g)).float()


def ncut_ref(n, dtype):
    """autograd of the closed form in vit.hip's comment: u = A x, s = A 1, a = s.x, cut = a - x.u, NCut = cut / a + cut / (S - a)"""
    A, x = ncut_inputs(n)
    A, x = A.to(dtype), x.to(dtype).requires_grad_(True)
    u, s = A @ x, A.sum(1)
    a = s @ x
    cut = a - x @ u
    val = cut / a + cut / (s.sum() - a)
    val.backward()
    return val.detach(), x.grad.detach(), u.detach(), s
