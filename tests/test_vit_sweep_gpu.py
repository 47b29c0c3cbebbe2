"""The ViT / soft-NCut kernels (csrc/attention.hip, csrc/vit.hip, rcf_gemm_nt_f32 / rcf_gemm_nt_batched_f32) against float64
restatements at the edges of their launch geometry (tests/vit_cases.py; conditioning of every case and the derived floor of the
NCut gradient: tests/test_vit_sweep_cpu.py).  Errors are max error / max |ref|, the measure and the floors of
tests/test_vit_gpu.py: 2e-5 (attention, bf16-triple GEMM, layernorm, softmax), 2e-6 (fp16-pair GEMM with ranges), 1e-5 (NCut
value).  Every call runs twice on fresh outputs and the two runs are bit-equal; pitched operands sit inside buffers whose guard
columns are checked afterwards."""
from ctypes import c_void_p

import pytest
import torch

import rcf_amd  # noqa: F401  (package alias)
import vit_cases as vc
from rcf_amd import _lib, ops

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
NAN = float("nan")
EINVAL = dict(match="status -1")
P = lambda t: c_void_p(t.data_ptr())


class Slice:
    """columns [c0 : c0 + cols] of a FILL-ed [rows, width] device buffer"""

    def __init__(self, rows, cols, width, c0, init=None):
        self.big = torch.full((rows, width), vc.FILL, dtype=torch.float32, device=DEV)
        self.v, self.c0, self.cols = self.big[:, c0:c0 + cols], c0, cols
        if init is None:
            self.v.fill_(NAN)
        else:
            self.v.copy_(init)

    def guards_intact(self):
        return bool((self.big[:, :self.c0] == vc.FILL).all()) and bool((self.big[:, self.c0 + self.cols:] == vc.FILL).all())


def same(a, b):
    """bit-equal, NaN == NaN"""
    return a.dtype == b.dtype and a.shape == b.shape and torch.equal(a.contiguous().view(torch.uint8), b.contiguous().view(torch.uint8))


def bits_of_max(t):
    return int(t.float().abs().max().view(torch.int32))


def amax_slot(bits=0):
    return torch.full((1,), bits, dtype=torch.int32, device=DEV)


def above(t):
    """the bits of a range well above max |t|"""
    return int((t.float().abs().max() * 2 + 1).view(torch.int32))


def check_amax(run, what):
    """run(slot) -> (buffer, output view).  Twice from a zeroed slot: bit-equal, and the slot holds the bits of max |out|; once from a
    slot preset above it: the slot is unchanged and the output is the same"""
    s1, s2 = amax_slot(), amax_slot()
    (b1, o1), (b2, o2) = run(s1), run(s2)
    assert same(b1, b2) and int(s1) == int(s2), f"{what}: two runs of the same call differ"
    assert int(s1) == bits_of_max(o1), f"{what}: amax_out is not the range of the kernel's own output"
    hi = above(o1)
    s3 = amax_slot(hi)
    b3, _ = run(s3)
    assert int(s3) == hi and same(b3, b1), f"{what}: a larger preset amax_out was changed"
    return b1, o1


# ------------------------------------------------------------------------------------------------------------ attention
@pytest.mark.parametrize("c", vc.ATTN_PARAMS)
def test_attention_sweep_vs_float64(c, report):
    qkv = vc.attn_qkv(c)
    rows, dim = c.B * c.T, c.dim
    q = Slice(rows, 3 * dim, 3 * dim + 8, 4, qkv) if c.pitched else Slice(rows, 3 * dim, 3 * dim, 0, qkv)
    amax = ops.absmax(qkv.to(DEV)) if c.arith == "h2" else None
    outs = []

    def run(slot):
        o = Slice(rows, dim, dim + 8, 4) if c.pitched else Slice(rows, dim, dim, 0)
        ops.attention(q.v, c.B, c.T, c.nh, c.scale, out=o.v, amax=amax, amax_out=slot)
        outs.append(o)
        return o.big, o.v
    _, out = check_amax(run, c.name)
    assert q.guards_intact() and all(o.guards_intact() for o in outs), "a guard column of a pitched buffer was written"
    assert same(q.v.cpu(), qkv), "qkv was written"
    e = vc.rel(out.cpu(), vc.attn_ref(c, torch.float64))
    report(f"vit sweep attention {c.name}: {e:.2e} ({c.why})")
    assert e < vc.FLOOR


def test_attention_refuses_what_it_cannot_do():
    """head_dim != 64, a pitch that is no multiple of 4, more than 65535 (image, head) pairs: a status before any launch"""
    T, nh = 5, 2
    dim = nh * vc.HD
    qkv, out = torch.zeros(T, 3 * dim + 2, device=DEV), torch.full((T, dim + 2), vc.FILL, device=DEV)
    st = ops._stream()
    with pytest.raises(_lib.RcfHipError, **EINVAL):
        ops.call("rcf_attention_fwd_f32", P(qkv), 3 * dim, P(out), dim, 1, T, 4, 32, 0.125, None, None, st)             # head_dim = 32
    with pytest.raises(_lib.RcfHipError, **EINVAL):
        ops.call("rcf_attention_fwd_f32", P(qkv), 3 * dim + 2, P(out), dim, 1, T, nh, vc.HD, 0.125, None, None, st)     # ld_qkv % 4
    with pytest.raises(_lib.RcfHipError, **EINVAL):
        ops.call("rcf_attention_fwd_f32", P(qkv), 3 * dim, P(out), dim + 2, 1, T, nh, vc.HD, 0.125, None, None, st)     # ld_out % 4
    B = 65536
    big, bout = torch.zeros(B, 3 * vc.HD, device=DEV), torch.full((B, vc.HD), vc.FILL, device=DEV)
    with pytest.raises(_lib.RcfHipError, **EINVAL):
        ops.attention(big, B, 1, 1, 0.125, out=bout)                                                                    # B nh > 65535
    torch.cuda.synchronize()
    assert bool((out == vc.FILL).all()) and bool((bout == vc.FILL).all()), "a refused call wrote to its output"


# ----------------------------------------------------------------------------------------------------------------- GEMM
@pytest.mark.parametrize("c,v,mag", vc.GEMM_PARAMS)
def test_gemm_sweep_vs_float64(c, v, mag, report):
    a, b, bias, c0 = vc.gemm_inputs(c.name, mag)
    M, N, K = c.M, c.N, c.K
    A = Slice(M, K, K + 8, 4, a) if c.pitched else Slice(M, K, K, 0, a)
    B = Slice(N, K, K + 8, 4, b) if c.pitched and v != "pre" else Slice(N, K, K, 0, b)      # pre-split weights need ldb == K
    amax = (ops.absmax(a.to(DEV)), ops.absmax(b.to(DEV))) if v != "x3" else None
    pairs = ops.weight_pairs_2d(B.v, amax[1]) if v == "pre" else None
    bg = bias.to(DEV) if c.bias else None
    width, col0 = (c.ldc, 0) if c.ldc else (vc.cdiv(N, 4) * 4 + 8, 4)
    outs = []

    def run(slot, pairs=pairs):
        o = Slice(M, N, width, col0, c0 if c.beta else None)
        ops.gemm_nt(A.v, B.v, bg, out=o.v, act=c.act, beta=c.beta, amax=amax, b_pairs=pairs, amax_out=slot)
        outs.append(o)
        return o.big, o.v
    big, out = check_amax(run, f"{c.name}-{v}")
    if v == "pre":                                        # weights split beforehand: the bits of the launch that splits them itself
        assert same(run(amax_slot(), None)[0], big), "pre-split weights give other bits than the fp16-pair launch that splits them"
    assert all(o.guards_intact() for o in outs), "a column outside [0, N) of the output buffer was written"
    assert A.guards_intact() and B.guards_intact() and same(A.v.cpu(), a) and same(B.v.cpu(), b)
    e = vc.rel(out.cpu(), vc.gemm_ref(c, mag, torch.float64))
    report(f"vit sweep gemm {c.name}-{v} |a| {mag[0]:g} |b| {mag[1]:g} ({M}, {N}, {K}) tile {c.tile[0]}x{c.tile[1]}: {e:.2e} ({c.why})")
    assert e < vc.gemm_floor(v)


def test_batched_gemm_vit_pattern_vs_float64(report):
    """the un-fused attention's two launches (vit.py) at T = 37: S = q k^T out of the qkv buffer (head stride 64, rows of pitch Tp =
    40 whose last three columns keep their fill), then P V from transpose2d's zero-tailed [dim][Tp] (K = 40)"""
    q = vc.BG_VIT
    T, nh, Bn, Tp = q["T"], q["nh"], q["B"], q["Tp"]
    dim, hd = nh * vc.HD, vc.HD
    qkv, Pm = vc.bg_vit_inputs()
    S_ref, O_ref = vc.bg_vit_ref(torch.float64)
    rows = qkv.to(DEV)

    def scores():
        S = torch.full((Bn, nh, T, Tp), vc.FILL, dtype=torch.float32, device=DEV)
        ops.gemm_nt_batched(rows, 3 * dim, (T * 3 * dim, hd), rows[:, dim:], 3 * dim, (T * 3 * dim, hd), S, Tp, (nh * T * Tp, T * Tp),
                            (Bn, nh), T, T, hd)
        return S
    S, S2 = scores(), scores()
    assert same(S, S2) and bool((S[..., T:] == vc.FILL).all()), "two runs differ, or a column from N on was written"
    e_s = vc.rel(S[..., :T].cpu(), S_ref)
    Pg = torch.zeros((Bn, nh, T, Tp), dtype=torch.float32, device=DEV)
    Pg[..., :T] = Pm.to(DEV)
    Vt = torch.stack([ops.transpose2d(rows[i * T:(i + 1) * T, 2 * dim:], Tp) for i in range(Bn)])      # [B, dim, Tp]
    assert torch.equal(Vt[..., :T].cpu(), qkv.view(Bn, T, 3 * dim)[:, :, 2 * dim:].transpose(1, 2)) and not Vt[..., T:].any()

    def pv():
        o = Slice(Bn * T, dim, dim + 8, 4)
        ops.gemm_nt_batched(Pg, Tp, (nh * T * Tp, T * Tp), Vt, Tp, (dim * Tp, hd * Tp), o.v, dim + 8, (T * (dim + 8), hd), (Bn, nh), T, hd, Tp)
        return o
    o, o2 = pv(), pv()
    assert same(o.big, o2.big) and o.guards_intact()
    e_o = vc.rel(o.v.cpu(), O_ref)
    report(f"vit sweep batched gemm T={T} nh={nh} B={Bn}: q k^T {e_s:.2e} (N = 37 into pitch 40), P V {e_o:.2e} (K = 40, pitched out)")
    assert max(e_s, e_o) < vc.FLOOR


def test_batched_gemm_accumulating_vs_float64(report):
    q = vc.BG_BETA
    (b0, b1), M, N, K = q["batch"], q["M"], q["N"], q["K"]
    a, b, c0 = vc.bg_beta_inputs()
    ag, bg = a.to(DEV), b.to(DEV)

    def run():
        out = c0.to(DEV).clone()
        ops.gemm_nt_batched(ag, K, (b1 * M * K, M * K), bg, K, (b1 * N * K, N * K), out, N, (b1 * M * N, M * N), (b0, b1), M, N, K, beta=1)
        return out
    out, out2 = run(), run()
    assert same(out, out2)
    e = vc.rel(out.cpu(), vc.bg_beta_ref(torch.float64))
    report(f"vit sweep batched gemm ({b0}, {b1}) x ({M}, {N}, {K}) beta 1: {e:.2e}")
    assert e < vc.FLOOR


def test_gemm_refuses_what_it_cannot_do():
    a, b = torch.zeros(8, 8, device=DEV), torch.zeros(8, 8, device=DEV)
    out = torch.full((8, 8), vc.FILL, device=DEV)
    with pytest.raises(_lib.RcfHipError, **EINVAL):
        ops.gemm_nt(a[:, :6], b[:, :6], out=out)                                      # K % 4
    with pytest.raises(_lib.RcfHipError, **EINVAL):
        ops.gemm_nt(a, b, out=torch.full((8, 10), vc.FILL, device=DEV)[:, :8])          # ldc % 4
    amax = (ops.absmax(a), ops.absmax(b))
    wide = torch.zeros(8, 12, device=DEV)
    with pytest.raises(_lib.RcfHipError, **EINVAL):
        ops.gemm_nt(a, wide[:, :8], out=out, amax=amax, b_pairs=ops.weight_pairs_2d(b, amax[1]))      # pre-split weights with ldb != K
    with pytest.raises(_lib.RcfHipError, **EINVAL):
        ops.gemm_nt_batched(a, 8, (2, 0), b, 8, (0, 0), out, 8, (0, 0), (1, 1), 8, 8, 8)              # a batch stride that is no multiple of 4
    torch.cuda.synchronize()
    assert bool((out == vc.FILL).all())


# ------------------------------------------------------------------------------------------------------------ layernorm
@pytest.mark.parametrize("rows,C", vc.LN_PARAMS)
def test_layernorm_sweep_vs_float64(rows, C, report):
    x, gamma, beta = vc.ln_inputs(rows, C)
    X = Slice(rows, C, C + 8, 4, x)
    gam, bet = gamma.to(DEV), beta.to(DEV)
    outs = []

    def run(slot):
        o = Slice(rows, C, C + 8, 4)
        ops.layernorm(X.v, gam, bet, vc.LN_EPS, out=o.v, amax_out=slot)
        outs.append(o)
        return o.big, o.v
    _, y = check_amax(run, f"{rows}x{C}")
    assert X.guards_intact() and all(o.guards_intact() for o in outs) and same(X.v.cpu(), x)
    y = y.cpu()
    ref = vc.ln_ref(rows, C, torch.float64)
    e = vc.rel(y, ref)
    e_big = float((y[2].double() - ref[2]).abs().max() / ref.abs().max()) if rows >= 5 else 0.0
    report(f"vit sweep layernorm {rows}x{C}: {e:.2e}, the row of mean {vc.LN_BIG_MEAN:g} and spread 1e-2 {e_big:.2e} ({vc.LN_WHY[C]})")
    assert e < vc.FLOOR
    if rows >= 5:
        assert torch.equal(y[1], beta), "a constant row does not give beta exactly"


def test_layernorm_refuses_what_it_cannot_do():
    for C in (6, 2052):
        x, out = torch.zeros(2, C, device=DEV), torch.full((2, C), vc.FILL, device=DEV)
        with pytest.raises(_lib.RcfHipError, **EINVAL):
            ops.layernorm(x, torch.ones(C, device=DEV), torch.zeros(C, device=DEV), vc.LN_EPS, out=out)
        torch.cuda.synchronize()
        assert bool((out == vc.FILL).all())


# -------------------------------------------------------------------------------------------------------------- softmax
@pytest.mark.parametrize("pitch,n,scale", vc.SM_PARAMS)
def test_softmax_rows_sweep_vs_float64(pitch, n, scale, report):
    x = vc.sm_inputs(n)

    def run():
        buf = torch.full((4, pitch), NAN, dtype=torch.float32, device=DEV)              # the pad holds NaN: it is replaced, not scaled
        buf[3] = vc.FILL                                                                # a fourth row the call does not own
        buf[:3, :n] = x.to(DEV)
        ops.softmax_rows_(buf[:3], n, scale)
        return buf
    buf, buf2 = run(), run()
    assert same(buf, buf2)
    assert bool((buf[3] == vc.FILL).all()), "a row beyond `rows` was written"
    assert bool((buf[:3, n:] == 0).all()), "columns [n, pitch) are not exactly 0"
    y = buf[:3, :n].cpu()
    e, s = vc.rel(y, vc.sm_ref(n, scale, torch.float64)), float((y.double().sum(-1) - 1).abs().max())
    report(f"vit sweep softmax pitch {pitch} n {n} scale {scale:g} ({'registers' if vc.sm_fast(pitch) else 'three passes'}): {e:.2e}, "
           f"row sums off 1 by {s:.2e}")
    assert e < vc.FLOOR and s < vc.FLOOR
    assert float(y[1].min()) == float(y[1].max()), "a row of equal logits does not give equal probabilities"


# ---------------------------------------------------------------------------------------- transpose2d, l2_normalize_rows
@pytest.mark.parametrize("rows,cols,dpitch", vc.TR_PARAMS)
def test_transpose2d_sweep_exact(rows, cols, dpitch):
    g = torch.Generator().manual_seed(rows * 1000 + cols)
    x = torch.randn(rows, cols, generator=g)
    X = Slice(rows, cols, cols + 8, 4, x)
    d1, d2 = ops.transpose2d(X.v, dpitch), ops.transpose2d(X.v, dpitch)
    assert same(d1, d2) and tuple(d1.shape) == (cols, dpitch)
    assert torch.equal(d1[:, :rows].cpu(), x.T.contiguous()) and not d1[:, rows:].any() and not torch.isnan(d1).any()
    assert X.guards_intact() and same(X.v.cpu(), x)


@pytest.mark.parametrize("C", vc.L2_C)
def test_l2_normalize_rows_sweep_vs_float64(C, report):
    x = vc.l2_inputs(C)
    X = Slice(vc.L2_ROWS, C, C + 8, 4, x)
    y, y2 = ops.l2_normalize_rows(X.v), ops.l2_normalize_rows(X.v)
    assert same(y, y2) and X.guards_intact()
    y = y.cpu()
    ref = vc.l2_ref(C, torch.float64)
    e = vc.row_rel(y, ref)
    e_tiny = vc.rel(y[2], x[2].double() / 1e-12)
    report(f"vit sweep l2_normalize C={C}: worst row {e:.2e}; the row of norm 1e-20 against x / 1e-12 {e_tiny:.2e}")
    assert e < vc.FLOOR and e_tiny < vc.FLOOR
    assert not y[1].any(), "a zero row does not give zeros"


# ------------------------------------------------------------------------------------------------------- soft-NCut pieces
@pytest.mark.parametrize("n,pitch", vc.AFF_PARAMS)
def test_affinity_threshold_sweep_exact(n, pitch):
    x, want = vc.aff_inputs(n)

    def run():
        G = Slice(n, n, pitch, 0, x)
        ops.call("rcf_affinity_threshold_f32", P(G.big), pitch, n, vc.TAU, vc.AFF_EPS, ops._stream())
        return G
    G, G2 = run(), run()
    assert same(G.big, G2.big) and G.guards_intact(), "two runs differ, or a pad column was written"
    assert torch.equal(G.v.cpu(), want)


@pytest.mark.parametrize("n,pitch", vc.NCUT_PARAMS)
def test_ncut_value_grad_sweep_vs_float64(n, pitch, report):
    A, x = vc.ncut_inputs(n)
    G = Slice(n, n, pitch, 0, A)
    xg = x.to(DEV)
    s = torch.full((n,), NAN, dtype=torch.float64, device=DEV)

    def run(compute_rowsum):
        u = torch.full((n,), NAN, dtype=torch.float64, device=DEV)
        grad, val = torch.full((n + 8,), vc.FILL, dtype=torch.float32, device=DEV), torch.full((2,), vc.FILL, dtype=torch.float32, device=DEV)
        grad[:n] = NAN
        ops.call("rcf_ncut_value_grad_f32", P(G.big), pitch, n, P(xg), P(u), P(s), compute_rowsum, P(grad), P(val), ops._stream())
        return u, grad, val
    u, grad, val = run(1)
    s1 = s.clone()
    u2, grad2, val2 = run(0)                                # the row sums are kept: the same bits
    assert same(u, u2) and same(grad, grad2) and same(val, val2) and same(s, s1)
    assert bool((grad[n:] == vc.FILL).all()) and float(val[1]) == vc.FILL and G.guards_intact() and same(G.v.cpu(), A)
    v64, g64, u64, s64 = vc.ncut_ref(n, torch.float64)
    e_v, e_g = abs(float(val[0]) - float(v64)) / abs(float(v64)), vc.rel(grad[:n].cpu(), g64)
    e_u, e_s = vc.rel(u.cpu(), u64), vc.rel(s.cpu(), s64)
    report(f"vit sweep ncut n={n} pitch {pitch}: value {e_v:.2e} gradient {e_g:.2e} (floor {vc.FLOOR_NCUT_GRAD:g}); fp64 mat-vec u {e_u:.1e} "
           f"row sums {e_s:.1e} ({vc.NCUT_WHY[n]})")
    assert e_v < vc.FLOOR_NCUT and e_g < vc.FLOOR_NCUT_GRAD
    assert e_u < 1e-12 and e_s < 1e-12                       # float64 accumulations of float32 operands
