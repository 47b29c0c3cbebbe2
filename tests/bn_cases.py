"""Edge-geometry cases of the batch-norm family (csrc/bn.hip) and their reference.

Shared by tests/test_bn_sweep_cpu.py (the table really reaches the geometry it names; the reference's own float32 error)
and tests/test_bn_sweep_gpu.py (the kernels against the float64 truth).  The reference is plain torch on the CPU, written
out term by term in the dtype asked for (F.batch_norm refuses one value per channel and its ReLU pattern cannot be fixed);
nothing of the HIP package enters this module.

Both runs of the reference ADD in float64 (`colsum`): the column sums are float64 accumulations of addends formed in the
run's dtype.  That is the kernels' contract too (fp32 addends, fp64 accumulation), and it is what lets the float32 run be
held to the 5e-7 floor of the raw sums at all: a float32 accumulation of 32 773 addends is no statement about any kernel.

Geometry constants restated below to CHOOSE inputs (never as a reference for a value):
  col_geom            cvB = min(CV, 64) channel vectors per block, RG = 256 / cvB row groups, chunks <= 1024 / cgroups,
                      at least 8 RG rows per chunk, the chunk count re-derived from the rounded-up rows per chunk
  ew_geom             cvt = min(CV, 256), rpb = 256 / cvt rows per block, grid.x = row blocks / 8
  launch_partial_sum  32 -> 16 -> 8 columns while a thread would walk more than 32 rows or fewer than 64 workgroups ran
  vec_width           8 only for bf16 on both sides with C and every pitch divisible by 8

What each case is for:
  one_row        1 row: var = 0, invstd = eps^-1/2, the unscaled running_var branch, only the tail trip of the two-in-flight loop,
                 dx == 0
  idle_threads   CV = 12: RG = rpb = 21 (252 of 256 threads), 3 chunks of 143 rows (6 full trips of the 21 row groups and one
                 of 17), 2 row blocks, 143 rows per image straddling the row groups under dropout
  single_vector  CV = 1: RG = rpb = 256
  ragged_cgroup  CV = 80: the second column group holds 16 of 64 vectors, rpb = 3 (240 threads), H = 1, prime row count
  ragged_cchunk  CV = 320: the second channel chunk of the element-wise grid holds 64 of 256
  chains_128     128 chunks = exactly one four-chain trip of partial_sum_kernel<8>, no tail
  chains_129     129 chunks: the tail loop for slice 0 only
  cols16         n = 2C = 1024 -> partial_sum_kernel<16>
  cols32_cap     fp32: the cap of 256 chunks binds, the count re-derives to 249, 32 columns; bf16: the 8-wide geometry cuts 257
                 chunks, so the workspace rule "larger of the two" decides
  cap_1024       the 1024-chunk cap binds (994 after re-deriving), 1024 row blocks; >= 8192 rows: also under BN_SWEEP_ALWAYS
  v8_idle        8-wide vectors with CV = 3: RG = rpb = 85 (255 threads)
  v4_bf16        C % 8 == 4: bf16 storage on the 4-wide path
  pitched        every operand a channel slice [..., 8:136] of a wider buffer; pitch 140 forces bf16 down to 4-wide vectors
"""
import dataclasses
import functools
import types

import pytest
import torch

EPS, MOMENTUM, KEEP_P = 1e-5, 0.1, 0.7
REF_THREADS = 16

# floors: the project's own (tests/test_kernels_gpu.py test_batchnorm_train / test_conv_fwd_fused_bn_stats,
# tests/test_bf16_gpu.py test_batchnorm_mixed_precision)
FLOOR_F32, FLOOR_F32_SUMS, FLOOR_BF16, FLOOR_BF16_SUMS = 2e-5, 5e-7, 5e-3, 1e-6
TIE_MARGIN, TIE_SHARE = 1e-5, 2e-4
FILL = 7.0                                           # what guard channels and untouched buffers hold


@dataclasses.dataclass(frozen=True)
class Variant:
    tag: str
    xdt: str                  # storage of the conv-output side (x, dx): "f32" | "bf16"
    ydt: str                  # storage of the activation side (y, dy, residual, dres)
    pitch: int = 0            # 0: contiguous; else every operand is the slice [..., 8:8 + C] of a buffer this wide


F32, MIXED, BF16 = Variant("f32", "f32", "f32"), Variant("mixed", "f32", "bf16"), Variant("bf16", "bf16", "bf16")


@dataclasses.dataclass(frozen=True)
class Case:
    name: str
    N: int
    H: int
    W: int
    C: int
    variants: tuple
    res: bool = False         # a residual is added before the ReLU (and dres comes back)
    drop: bool = False        # Dropout2d scale per (image, channel)
    res_beta: int = 0         # dres accumulates
    seed: int = 0

    @property
    def rows(self):
        return self.N * self.H * self.W


CASES = [
    Case("one_row", 1, 1, 1, 48, (F32,), res=True, seed=101),
    Case("idle_threads", 3, 11, 13, 48, (F32, MIXED), res=True, drop=True, res_beta=1, seed=102),
    Case("single_vector", 2, 25, 82, 4, (F32,), drop=True, seed=103),
    Case("ragged_cgroup", 1, 1, 337, 320, (F32, MIXED), res=True, seed=104),
    Case("ragged_cchunk", 3, 7, 9, 1280, (F32,), res=True, drop=True, res_beta=1, seed=205),
    Case("chains_128", 1, 128, 128, 64, (F32,), seed=106),
    Case("chains_129", 1, 37, 443, 64, (F32,), seed=107),
    Case("cols16", 1, 17, 241, 512, (F32,), seed=208),
    Case("cols32_cap", 1, 40, 205, 1024, (F32, BF16), res=True, res_beta=1, seed=109),
    Case("cap_1024", 1, 13, 2521, 256, (F32,), res=True, drop=True, seed=110),
    Case("v8_idle", 2, 100, 100, 24, (BF16,), res=True, drop=True, res_beta=1, seed=111),
    Case("v4_bf16", 1, 25, 41, 20, (BF16,), res=True, seed=112),
    Case("pitched", 3, 9, 11, 128, (Variant("f32_p144", "f32", "f32", 144), Variant("bf16_p144", "bf16", "bf16", 144),
                                    Variant("bf16_p140", "bf16", "bf16", 140)), res=True, drop=True, res_beta=1, seed=113),
]
# pair planes (fp32 only, C % 8 == 0): CV = 2 -> rpb = 128; CV = 66 -> rpb = 3 (198 threads)
PLANE_CASES = [Case("planes_cv2", 2, 25, 82, 8, (F32,), seed=121), Case("planes_cv66", 1, 1, 337, 264, (F32,), res=True, seed=122)]
BY_NAME = {c.name: c for c in CASES + PLANE_CASES}
RUNS = [(c, v) for c in CASES for v in c.variants]
PARAMS_RUNS = [pytest.param(c, v, id=f"{c.name}-{v.tag}") for c, v in RUNS]
PARAMS_CASES = [pytest.param(c, id=c.name) for c in CASES]


def variant(case, tag):
    """a case's own variant of that name, else the contiguous storage variant of that name"""
    return next(v for v in case.variants + (F32, MIXED, BF16) if v.tag == tag)


# ------------------------------------------------------------------------------------------- geometry (to choose inputs)
def cdiv(a, b):
    return -(-a // b)


def col_geom(rows, C, V=4):
    CV = C // V
    cvB = min(CV, 64)
    RG = 256 // cvB
    cgroups = cdiv(CV, cvB)
    cap, want = 1024 // cgroups, cdiv(rows, RG * 8)
    first = max(min(cap, want), 1)
    rows_per_chunk = cdiv(rows, first)
    return types.SimpleNamespace(CV=CV, cvB=cvB, RG=RG, cgroups=cgroups, cap=cap, want=want, first=first,
                                 rows_per_chunk=rows_per_chunk, chunks=cdiv(rows, rows_per_chunk),
                                 last_group=CV - (cgroups - 1) * cvB)


def ew_geom(rows, CV):
    cvt = min(CV, 256)
    rpb = 256 // cvt
    cchunks = cdiv(CV, cvt)
    bx = min(max(cdiv(rows, rpb) // 8, 1), max(4096 // cchunks, 1))
    return types.SimpleNamespace(CV=CV, cvt=cvt, rpb=rpb, cchunks=cchunks, bx=bx, last_chunk=CV - (cchunks - 1) * cvt)


def partial_cols(chunks, n):
    cols = 32
    while cols > 8 and (chunks // (256 // cols) > 32 or cdiv(n, cols) < 64):
        cols >>= 1
    return cols


def vec_width(var, C):
    pitch = var.pitch or C
    return 8 if (var.xdt == "bf16" and var.ydt == "bf16" and C % 8 == 0 and pitch % 8 == 0) else 4


def workspace_chunks(rows, C):
    """rcf_bn_stats_workspace_bytes / (2 C doubles): the larger of the 4-wide and the 8-wide geometry's chunk counts"""
    c = col_geom(rows, C).chunks
    return max(c, col_geom(rows, C, 8).chunks) if C % 8 == 0 else c


def geometry(case, var):
    V = vec_width(var, case.C)
    g, e = col_geom(case.rows, case.C, V), ew_geom(case.rows, case.C // V)
    return types.SimpleNamespace(V=V, col=g, ew=e, cols=partial_cols(g.chunks, 2 * case.C))


# ------------------------------------------------------------------------------------------------------------ inputs
TORCH = {"f32": torch.float32, "bf16": torch.bfloat16}


def _store(t, dt):
    """the float64 of what a tensor of storage type dt holds"""
    return t.to(TORCH[dt]).double()


def make_inputs(case, var):
    """float64 [rows, C] matrices and [C] vectors holding exactly the stored values: per-channel scales 2^(3u), offsets
    3 * normal, gamma in [0.5, 1.5], beta normal, keep in {0, 1 / 0.7} per (image, channel).  One stream of draws per case:
    every variant of a case rounds the SAME draws to its storage types."""
    g = torch.Generator().manual_seed(case.seed)
    rows, C, N = case.rows, case.C, case.N
    rnd, uni = (lambda *s: torch.randn(*s, generator=g)), (lambda *s: torch.rand(*s, generator=g))
    i = types.SimpleNamespace(rows=rows, C=C, n=float(rows), per_image=case.H * case.W)
    i.x = _store(rnd(rows, C) * torch.exp2(3 * uni(C)) + 3 * rnd(C), var.xdt)
    i.r = _store(rnd(rows, C) * torch.exp2(3 * uni(C)) * 0.5, var.ydt)
    i.dy = _store(rnd(rows, C) * torch.exp2(3 * uni(C)), var.ydt)
    i.dres0 = _store(rnd(rows, C), var.ydt)
    i.gamma, i.beta = (uni(C) + 0.5).double(), rnd(C).double()
    i.keep = ((uni(N, C) > 1 - KEEP_P).float() / KEEP_P).double()               # [N, C]
    i.rm0, i.rv0 = rnd(C).double(), (uni(C) + 0.5).double()
    i.dgamma0, i.dbeta0 = rnd(C).double(), rnd(C).double()
    # a second norm on a second conv output: the residual normalised on the fly, and the downsample norm of the shared backward
    i.x2 = _store(rnd(rows, C) * torch.exp2(3 * uni(C)) + 3 * rnd(C), var.xdt)
    i.gamma2, i.beta2 = (uni(C) + 0.5).double(), rnd(C).double()
    i.dgamma20, i.dbeta20 = rnd(C).double(), rnd(C).double()
    i.mask4 = torch.randint(0, 16, (rows * C // 4,), generator=g, dtype=torch.uint8)
    if not case.drop:
        i.keep = None
    if not case.res:
        i.r = None
    return i


def keep_rows(i, dtype):
    """[rows, C] Dropout2d scale, or None"""
    return None if i.keep is None else i.keep.to(dtype).repeat_interleave(i.per_image, dim=0)


def mask_to_pattern(mask, rows, C):
    """uint8 [rows * C / 4] sign bits (bit e of byte j = channel 4 j + e) -> bool [rows, C]"""
    m = mask.reshape(rows, C // 4, 1).to(torch.int32)
    return ((m >> torch.arange(4, dtype=torch.int32, device=mask.device)) & 1).bool().reshape(rows, C)


# --------------------------------------------------------------------------------------------------------- reference
def colsum(t):
    return t.double().sum(0)


def stats(x, n, dtype):
    mean = (colsum(x) / n).to(dtype)
    d = x - mean
    var = (colsum(d * d) / n).to(dtype)
    return mean, var, 1.0 / torch.sqrt(var + EPS), d


def forward(i, dtype, res_norm=False):
    """training-mode batch norm of x (+ residual, or + the second norm of x2 with res_norm) with and without ReLU, and the
    running statistics"""
    t = lambda v: None if v is None else v.to(dtype)
    x, n = t(i.x), i.n
    f = types.SimpleNamespace()
    f.sum, f.sumsq = colsum(x), colsum(x * x)
    f.mean, f.var, f.invstd, d = stats(x, n, dtype)
    f.xhat = d * f.invstd
    f.pre = f.xhat * t(i.gamma) + t(i.beta)
    if res_norm:
        f.mean2, f.var2, f.invstd2, d2 = stats(t(i.x2), n, dtype)
        f.pre = f.pre + (d2 * f.invstd2 * t(i.gamma2) + t(i.beta2))
    elif i.r is not None:
        f.pre = f.pre + t(i.r)
    f.keep = keep_rows(i, dtype)
    k = 1.0 if f.keep is None else f.keep
    f.y, f.y_lin = torch.relu(f.pre) * k, f.pre * k
    f.rm = (1 - MOMENTUM) * t(i.rm0) + MOMENTUM * f.mean
    f.rv = (1 - MOMENTUM) * t(i.rv0) + MOMENTUM * (f.var * (n / (n - 1)) if n > 1 else f.var)
    return f


def backward(i, f, pattern, dtype, xhat=None, gamma=None, invstd=None, keep="own"):
    """pattern: bool [rows, C] (None: no ReLU).  xhat / gamma / invstd: another norm under the same masked gradient."""
    t = lambda v: None if v is None else v.to(dtype)
    n = i.n
    xhat = f.xhat if xhat is None else xhat
    gamma, invstd = t(i.gamma if gamma is None else gamma), f.invstd if invstd is None else invstd
    b = types.SimpleNamespace()
    g = t(i.dy)
    kr = f.keep if keep == "own" else None
    if kr is not None:
        g = g * kr
    if pattern is not None:
        g = g * pattern.to(dtype)
    b.g, b.gx = g, g * xhat
    b.sg, b.sgx = colsum(b.g), colsum(b.gx)
    b.abs_sg, b.abs_sgx = colsum(b.g.abs()), colsum(b.gx.abs())
    sg, sgx = (b.sg / n).to(dtype), (b.sgx / n).to(dtype)
    b.dx = gamma * invstd * (g - sg - xhat * sgx)
    b.dres = g
    return b


def margin_of(pre):
    """per channel, from the float64 run: TIE_MARGIN of the largest pre-activation"""
    return TIE_MARGIN * pre.abs().amax(0)


def near_zero(pre64):
    return pre64.abs() < margin_of(pre64)


def pattern_with_ties(pre64, kernel_pattern):
    """the float64 sign pattern outside the margin, the kernel's own bit inside it"""
    return torch.where(near_zero(pre64), kernel_pattern, pre64 > 0)


# ------------------------------------------------------------------------------------------------------- error measure
TINY = 1e-300


def chan_err(got, ref, scale):
    """worst per-channel |got - ref| / scale_c; got / ref are [rows, C] or [C], scale is [C] float64.  A NaN anywhere gives inf."""
    d = (got.double() - ref.double()).abs()
    if d.dim() == 2:
        d = d.amax(0)
    e = d / scale.clamp_min(TINY)
    return float("inf") if bool(torch.isnan(e).any()) else float(e.max())


def scales(i, f, b=None, res_beta=0):
    """the float64 scales per channel, from the float64 run: y by the largest pre-activation, dx by |gamma| invstd max |dy|,
    dres by max |dy| (+ max |old| when it accumulates), the sums by the sums of the addends' magnitudes, mean by mean |x|,
    running_mean by mean |x| + |old| (the three fp32 roundings of its update), invstd and running_var relative"""
    kmax = 1.0 if i.keep is None else float(i.keep.max())
    s = types.SimpleNamespace()
    s.y = f.pre.abs().amax(0) * kmax
    s.y_lin = s.y
    s.mean = i.x.abs().mean(0)
    s.sum, s.sumsq = colsum(i.x.abs()), colsum(i.x * i.x)
    s.invstd, s.rv, s.rm = f.invstd.abs(), f.rv.abs(), s.mean + i.rm0.abs()
    dymax = i.dy.abs().amax(0)
    s.dx = i.gamma.abs() * f.invstd * dymax * kmax
    s.dres = dymax * kmax + (i.dres0.abs().amax() if res_beta else 0.0)
    if b is not None:
        s.sg, s.sgx = b.abs_sg, b.abs_sgx
    return s


def floors(var):
    """floor per quantity for a storage variant"""
    xb, yb = var.xdt == "bf16", var.ydt == "bf16"
    any_b = xb or yb
    return dict(sum=FLOOR_BF16_SUMS if xb else FLOOR_F32_SUMS, sumsq=FLOOR_BF16_SUMS if xb else FLOOR_F32_SUMS,
                mean=FLOOR_F32, invstd=FLOOR_F32, rm=FLOOR_F32, rv=FLOOR_F32,
                y=FLOOR_BF16 if yb else FLOOR_F32, y_lin=FLOOR_BF16 if yb else FLOOR_F32,
                sg=FLOOR_BF16_SUMS if any_b else FLOOR_F32_SUMS, sgx=FLOOR_BF16_SUMS if any_b else FLOOR_F32_SUMS,
                dx=FLOOR_BF16 if xb else FLOOR_F32, dres=FLOOR_BF16 if yb else FLOOR_F32,
                dgamma=FLOOR_BF16_SUMS if any_b else FLOOR_F32, dbeta=FLOOR_BF16_SUMS if any_b else FLOOR_F32)


# ----------------------------------------------------------------------------------------------------------- caches
@functools.lru_cache(maxsize=6)
def inputs(name, tag):
    c = BY_NAME[name]
    return make_inputs(c, variant(c, tag))


@functools.lru_cache(maxsize=6)
def truth(name, tag, res_norm=False):
    """the float64 forward of a run, computed once and shared (callers leave it unchanged)"""
    old = torch.get_num_threads()
    torch.set_num_threads(min(REF_THREADS, old))
    try:
        return forward(inputs(name, tag), torch.float64, res_norm)
    finally:
        torch.set_num_threads(old)


def ref32_errors(case, var):
    """the reference's own float32 run against its float64 run, per channel, with the float64 ReLU pattern: (errors by
    quantity, near-zero share, number of sign bits the float32 run would have set differently)"""
    i, f = inputs(case.name, var.tag), truth(case.name, var.tag)
    pat = f.pre > 0
    b = backward(i, f, pat, torch.float64)
    s = scales(i, f, b)
    f32 = forward(i, torch.float32)
    b32 = backward(i, f32, pat, torch.float32)
    e = {k: chan_err(getattr(f32, k), getattr(f, k), getattr(s, k)) for k in ("sum", "sumsq", "mean", "invstd", "rm", "rv", "y", "y_lin")}
    e.update(sg=chan_err(b32.sg, b.sg, s.sg), sgx=chan_err(b32.sgx, b.sgx, s.sgx), dx=chan_err(b32.dx, b.dx, s.dx),
             dres=chan_err(b32.dres, b.dres, s.dres),
             dgamma=chan_err((i.dgamma0.float() + b32.sgx.float()), i.dgamma0 + b.sgx, s.sgx),
             dbeta=chan_err((i.dbeta0.float() + b32.sg.float()), i.dbeta0 + b.sg, s.sg))
    share = float(near_zero(f.pre).double().mean())
    flips = int((((f32.pre > 0) != pat) & ~near_zero(f.pre)).sum())
    return e, share, flips
