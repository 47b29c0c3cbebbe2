"""Conditioning of the ViT / soft-NCut sweep (tests/vit_cases.py): the case tables reach the geometry they name, and every
reference's own float32 run sits within a quarter of its floor of the float64 run.  Then a kernel that misses a floor in
tests/test_vit_sweep_gpu.py is wrong, not unlucky.  A case that cannot meet this gets other inputs, never a looser limit."""
import math

import pytest
import torch

import vit_cases as vc


def test_attention_table_covers_the_kernel_limits():
    Ts = {c.T for c in vc.ATTN}
    assert Ts == {1, 31, 32, 33, 64, 65, 127, 128, 129, 193}
    assert any(T % vc.BKEY == 0 for T in Ts) and any(T % vc.BKEY == 1 and T > 1 for T in Ts)          # whole tiles; one key in the last
    assert any(T < 32 for T in Ts) and any(32 < T < 64 for T in Ts)                                    # a short wavefront; an idle one
    assert any(T % vc.BQ == 0 for T in Ts) and any(T % vc.BQ == 1 and T > vc.BQ for T in Ts)           # whole workgroups; one query in the last
    assert {(c.B, c.nh) for c in vc.ATTN} == {(1, 1), (2, 3)}
    assert {c.kind for c in vc.ATTN} == set(vc.KINDS)
    assert {(c.arith, c.mag) for c in vc.ATTN} == {("x3", 1.5), ("h2", 1.5), ("h2", 3e-4), ("h2", 2e3)}
    assert {c.arith for c in vc.ATTN if c.pitched} == {"x3", "h2"}
    assert any(c.T % vc.BKEY == 0 and c.kind == "rand" and not c.pitched for c in vc.ATTN)
    assert len({c.name for c in vc.ATTN}) == len(vc.ATTN) and all(c.why for c in vc.ATTN)
    for c in vc.ATTN:
        if c.kind in ("ramp", "first"):
            assert c.T > vc.BKEY, c.name
        s2 = vc.attn_logits(c) * math.log2(math.e)                                                     # the kernel's log2 domain
        tiles = [s2[..., k0:k0 + vc.BKEY].amax(-1) for k0 in range(0, c.T, vc.BKEY)]
        if c.kind == "ramp":                      # every tile raises every query's running maximum, by at least one binade
            assert all(bool((b >= a + 1).all()) for a, b in zip(tiles, tiles[1:])), c.name
        if c.kind == "first":                     # the maximum sits in tile 0; every later key is >= 100 lower
            assert all(bool((t <= tiles[0] - 100).all()) for t in tiles[1:]), c.name
            assert float(tiles[0].max()) < 40                                                          # and the logits that count stay small
        assert abs(float(vc.attn_qkv(c).abs().max()) / c.mag - 4) < 3                                  # the magnitude the case names


@pytest.mark.parametrize("c", vc.ATTN_PARAMS)
def test_attention_reference_float32_error_is_a_quarter_of_the_floor(c):
    e = vc.rel(vc.attn_ref(c, torch.float32), vc.attn_ref(c, torch.float64))
    print(f"vit sweep attention {c.name}: reference fp32 vs fp64 {e:.2e}")
    assert e <= 0.25 * vc.FLOOR


def test_gemm_table_covers_the_kernel_limits():
    assert {c.K % vc.KSTEP for c in vc.GEMM} >= {0, 4, 8, 12} and any(c.K < vc.KSTEP for c in vc.GEMM)
    assert {vc.gemm_tile(c.M, c.N) for c in vc.GEMM} == {(64, 64), (128, 64), (128, 128), (128, 256)}  # every tile class of plan_conv
    for c in vc.GEMM:
        assert vc.gemm_tile(c.M, c.N) == c.tile and c.why, c.name
        assert c.K % 4 == 0 and (c.ldc == 0 or (c.ldc % 4 == 0 and c.ldc >= c.N))
    by = vc.GEMM_BY_NAME
    assert by["ktail12"].M % 64 == 2 and by["wide"].N % 256 == 4 and by["wide"].M % 128 == 1
    assert by["odd_n"].N % 4 and by["odd_n"].ldc == 100
    assert by["presplit"].N % 256 == 0 and "pre" in by["presplit"].variants
    assert vc.cdiv(by["tall"].M, 128) == 512 and by["tall"].M % 128 == 1
    c = by["pitched"]
    assert c.pitched and c.bias and c.act == 2 and c.beta == 1
    assert sum(v == "h2" and m != vc.MAG_ONE for _, v, m in vc.GEMM_RUNS) == 2 * (len(vc.GEMM) - 1)
    q = vc.BG_VIT
    assert q["Tp"] == vc.cdiv(q["T"], 4) * 4 and q["T"] % 4 and q["Tp"] % vc.KSTEP == 8
    assert vc.BG_BETA["K"] % vc.KSTEP == 4 and vc.BG_BETA["batch"] == (3, 2)
    assert max(c.M * max(c.K + 8, c.N + 16) for c in vc.GEMM) * 4 < 8.5e6                              # nothing above the 8 MB of the Adam sweep


@pytest.mark.parametrize("c,v,mag", vc.GEMM_PARAMS)
def test_gemm_reference_float32_error_is_a_quarter_of_the_floor(c, v, mag):
    e = vc.rel(vc.gemm_ref(c, mag, torch.float32), vc.gemm_ref(c, mag, torch.float64))
    print(f"vit sweep gemm {c.name}-{v}-{mag[0]:g}: reference fp32 vs fp64 {e:.2e}")
    assert e <= 0.25 * vc.gemm_floor(v)


def test_batched_gemm_reference_float32_error_is_a_quarter_of_the_floor():
    (S32, O32), (S64, O64) = vc.bg_vit_ref(torch.float32), vc.bg_vit_ref(torch.float64)
    e = {"S": vc.rel(S32, S64), "PV": vc.rel(O32, O64), "beta": vc.rel(vc.bg_beta_ref(torch.float32), vc.bg_beta_ref(torch.float64))}
    print("vit sweep batched gemm: reference fp32 vs fp64 " + " ".join(f"{k} {v:.2e}" for k, v in e.items()))
    assert max(e.values()) <= 0.25 * vc.FLOOR


def test_small_kernel_tables_cover_the_kernel_limits():
    assert {C for _, C in vc.LN} == {4, 252, 256, 260, 384, 2048} == set(vc.LN_WHY) and {r for r, _ in vc.LN} == {1, 5, 8}
    assert all(C % 4 == 0 and C <= 2048 for _, C in vc.LN) and any(r < 4 for r, _ in vc.LN) and any(r % 4 == 0 for r, _ in vc.LN)
    assert {C // 4 for _, C in vc.LN} >= {1, 63, 64, 65, 512}
    # both softmax paths, the fast one at its cap, the slow one through each of its two conditions
    assert [(p, n) for p, n in vc.SM if vc.sm_fast(p)] == [(4, 1), (4, 3), (100, 97), (1028, 1025), (8192, 8190)]
    assert (vc.SM_FAST_CAP, 8190) in vc.SM and (vc.SM_FAST_CAP + 4, 8193) in vc.SM
    assert any(p % 4 and p <= vc.SM_FAST_CAP for p, _ in vc.SM) and all(p >= n for p, n in vc.SM)
    assert any(p // 4 > 256 and vc.sm_fast(p) for p, _ in vc.SM)                                       # a second float4 per thread
    for _, n in vc.SM:
        x = vc.sm_inputs(n)
        assert float(x[1].min()) == float(x[1].max()) == vc.SM_EQUAL
        assert float(x[2].max()) * 0.125 == 80 and (n == 1 or float(x[2].min()) * 0.125 == -80)
    assert any(r % 32 == 0 and c % 32 == 0 for r, c, _ in vc.TR) and any(r % 32 and c % 32 and d > r for r, c, d in vc.TR)
    assert all(d >= r for r, _, d in vc.TR) and any(d >= r + 64 for r, _, d in vc.TR)                  # whole tiles of nothing but tail
    assert {C % 64 for C in vc.L2_C} >= {0, 1, 63} and vc.L2_ROWS % 4
    for C in vc.L2_C:
        x = vc.l2_inputs(C).double()
        assert not x[1].any() and abs(float(x[2].norm()) / vc.L2_TINY - 1) < 1e-6
    assert {n for n, _ in vc.AFF} == {1, 5, 257} and {p - n for n, p in vc.AFF} == {0, 3}
    x, want = vc.aff_inputs(5)
    assert want[0, :5].tolist() == [vc.aff_inputs(1)[1][0, 0].item(), 1.0] + [want[0, 0].item()] * 2 + [1.0] and want[1, 0] == want[0, 0]
    assert bool(torch.isnan(x[0, 3])) and float(want[0, 0]) == float(torch.tensor(vc.AFF_EPS, dtype=torch.float32))
    assert {n for n, _ in vc.NCUT} == {2, 63, 64, 257, 1030} == set(vc.NCUT_WHY) and {p - n for n, p in vc.NCUT} == {0, 2}
    for n, _ in vc.NCUT:
        A, x = vc.ncut_inputs(n)
        assert torch.equal(A, A.T) and set(A.unique().tolist()) <= {1.0, float(torch.tensor(vc.AFF_EPS, dtype=torch.float32))}
        assert 0.05 <= float(x.min()) and float(x.max()) <= 0.95


@pytest.mark.parametrize("rows,C", vc.LN_PARAMS)
def test_layernorm_reference_float32_error_is_a_quarter_of_the_floor(rows, C):
    ref = vc.ln_ref(rows, C, torch.float64)
    y32 = vc.ln_ref(rows, C, torch.float32)
    e = vc.rel(y32, ref)
    rows_e = [float((y32[r].double() - ref[r]).abs().max() / ref.abs().max()) for r in range(rows)]
    print(f"vit sweep layernorm {rows}x{C}: reference fp32 vs fp64 {e:.2e}; per row " + " ".join(f"{v:.1e}" for v in rows_e))
    assert e <= 0.25 * vc.FLOOR
    if rows >= 5:                                                      # a constant row gives beta, exactly, in both runs
        beta = vc.ln_inputs(rows, C)[2]
        assert torch.equal(y32[1], beta) and torch.equal(ref[1], beta.double())


@pytest.mark.parametrize("pitch,n,scale", vc.SM_PARAMS)
def test_softmax_reference_float32_error_is_a_quarter_of_the_floor(pitch, n, scale):
    ref, y32 = vc.sm_ref(n, scale, torch.float64), vc.sm_ref(n, scale, torch.float32)
    e, s = vc.rel(y32, ref), float((y32.double().sum(-1) - 1).abs().max())
    print(f"vit sweep softmax {pitch}-{n} scale {scale:g}: reference fp32 vs fp64 {e:.2e}, row sums off 1 by {s:.2e}")
    assert e <= 0.25 * vc.FLOOR and s <= 0.25 * vc.FLOOR
    assert float((ref[1] * n - 1).abs().max()) < 1e-12


@pytest.mark.parametrize("C", vc.L2_C)
def test_l2_normalize_reference_float32_error_is_a_quarter_of_the_floor(C):
    ref, y32 = vc.l2_ref(C, torch.float64), vc.l2_ref(C, torch.float32)
    e = vc.row_rel(y32, ref)
    print(f"vit sweep l2_normalize C={C}: reference fp32 vs fp64 (per row) {e:.2e}")
    assert e <= 0.25 * vc.FLOOR
    assert not ref[1].any() and vc.rel(ref[2], vc.l2_inputs(C)[2].double() / 1e-12) < 1e-12            # the tiny row is divided by the clamp


@pytest.mark.parametrize("n", sorted({n for n, _ in vc.NCUT}))
def test_ncut_reference_float32_error_is_a_quarter_of_the_floor(n):
    v64, g64, _, _ = vc.ncut_ref(n, torch.float64)
    v32, g32, _, _ = vc.ncut_ref(n, torch.float32)
    e_v, e_g = abs(float(v32) - float(v64)) / abs(float(v64)), vc.rel(g32, g64)
    print(f"vit sweep ncut n={n}: reference fp32 vs fp64 value {e_v:.2e} gradient {e_g:.2e}")
    assert e_v <= 0.25 * vc.FLOOR_NCUT and e_g <= 0.25 * vc.FLOOR_NCUT_GRAD
