"""Conditioning of the batch-norm sweep (tests/bn_cases.py): the case table reaches the launch geometry it names, and the
reference's own float32 run sits within a quarter of each fp32 floor of its float64 run, per channel, with next to no
pre-activation close enough to zero for float32 to turn its sign.  Then a kernel that misses a floor in
tests/test_bn_sweep_gpu.py is wrong, not unlucky.  A case that cannot meet this gets other inputs, never a looser limit."""
import pytest

import bn_cases as bc


def test_case_table_covers_the_kernel_limits():
    """col_geom, ew_geom, the column choice of launch_partial_sum and vec_width restated from their constants (to choose inputs,
    not as a reference for any value): every entry of bn_cases' "what each case is for" holds"""
    by = bc.BY_NAME
    geo = {(c.name, v.tag): bc.geometry(c, v) for c, v in bc.RUNS}
    for (name, tag), g in geo.items():
        print(f"bn sweep geometry {name}-{tag}: V {g.V} col cvB {g.col.cvB} RG {g.col.RG} cgroups {g.col.cgroups} chunks "
              f"{g.col.first}->{g.col.chunks} x {g.col.rows_per_chunk} rows, {g.cols} columns; ew cvt {g.ew.cvt} rpb {g.ew.rpb} grid "
              f"{g.ew.bx} x {g.ew.cchunks}")

    g = geo["one_row", "f32"]                                                   # rows = 1: one chunk, one row block, tail trip only
    assert by["one_row"].rows == 1 and g.col.chunks == 1 and g.ew.bx == 1 and g.ew.bx * g.ew.rpb >= 1

    c, g = by["idle_threads"], geo["idle_threads", "f32"]
    assert g.col.cvB == 12 and g.col.RG == g.ew.rpb == 21 and 21 * 12 == 252 < 256
    assert g.col.chunks == 3 and g.col.rows_per_chunk == 143 and 143 % g.col.RG == 17          # a short last trip of the row groups
    assert g.ew.bx == 2 and c.drop and (c.H * c.W) % g.ew.rpb and (c.H * c.W) % g.col.RG       # images straddle the row groups
    assert {v.tag for v in c.variants} == {"f32", "mixed"}

    g = geo["single_vector", "f32"]
    assert g.col.CV == 1 and g.col.RG == g.ew.rpb == 256

    c, g = by["ragged_cgroup"], geo["ragged_cgroup", "f32"]
    assert g.col.CV == 80 and g.col.cgroups == 2 and g.col.last_group == 16 < g.col.cvB == 64   # c0 < C cuts the last column group
    assert g.ew.rpb == 3 and g.ew.rpb * g.ew.cvt == 240 and c.H == 1
    assert all(c.rows % k for k in range(2, 19))                                                # 337 is prime
    assert {v.tag for v in c.variants} == {"f32", "mixed"}

    g = geo["ragged_cchunk", "f32"]
    assert g.ew.CV == 320 and g.ew.cchunks == 2 and g.ew.last_chunk == 64 < g.ew.cvt == 256     # cv < CV cuts the last channel chunk

    # partial_sum_kernel<8>: 32 row slices, four chains -> trips of 128 partial rows
    g = geo["chains_128", "f32"]
    assert g.col.chunks == 128 and g.cols == 8
    g = geo["chains_129", "f32"]
    assert g.col.chunks == 129 and g.cols == 8
    assert geo["cols16", "f32"].cols == 16 and 2 * by["cols16"].C == 1024
    assert geo["cols32_cap", "f32"].cols == 32 and geo["cols32_cap", "bf16"].cols == 32

    # the cap 1024 / cgroups binds, and the count re-derived from the rounded-up rows per chunk is smaller
    g = geo["cols32_cap", "f32"]
    assert g.col.cgroups == 4 and g.col.want == 257 > g.col.cap == 256 == g.col.first and g.col.chunks == 249
    g8 = geo["cols32_cap", "bf16"]
    assert g8.V == 8 and g8.col.chunks == 257 > g.col.chunks                   # the 8-wide geometry cuts MORE chunks than the 4-wide
    assert bc.workspace_chunks(by["cols32_cap"].rows, 1024) == 257
    g = geo["cap_1024", "f32"]
    assert g.col.cgroups == 1 and g.col.want == 1025 > g.col.cap == 1024 == g.col.first and g.col.chunks == 994
    assert g.ew.bx == 1024 and g.cols == 8 and by["cap_1024"].rows >= 8192     # >= 8192 rows: make_sweep takes the banded orders

    # a cvB and a cvt that do not divide 256, on both vector widths
    assert any(256 % g.col.cvB and 256 % g.ew.cvt for g in geo.values() if g.V == 4)
    g = geo["v8_idle", "bf16"]
    assert g.V == 8 and g.col.CV == 3 and g.col.RG == g.ew.rpb == 85 and 85 * 3 == 255
    assert any(256 % g.col.cvB and 256 % g.ew.cvt for g in geo.values() if g.V == 8)

    # bf16 on each vector width
    c, g = by["v4_bf16"], geo["v4_bf16", "bf16"]
    assert c.C % 8 == 4 and g.V == 4
    assert {g.V for (n, t), g in geo.items() if t.startswith("bf16")} == {4, 8}

    c = by["pitched"]
    assert [(v.tag, v.pitch, bc.vec_width(v, c.C)) for v in c.variants] == [("f32_p144", 144, 4), ("bf16_p144", 144, 8),
                                                                          ("bf16_p140", 140, 4)]
    assert all(v.pitch >= 8 + c.C for v in c.variants)
    # the largest case: 32 773 x 256 fp32
    assert max(c.rows * c.C for c in bc.CASES) * 4 < 34e6


@pytest.mark.parametrize("case,var", bc.PARAMS_RUNS)
def test_reference_float32_error_is_a_quarter_of_the_floor(case, var):
    err, share, flips = bc.ref32_errors(case, var)
    print(f"bn sweep {case.name}-{var.tag}: reference fp32 vs fp64 " + " ".join(f"{k} {v:.2e}" for k, v in err.items()) +
          f"; near-zero share {share:.2e}, sign bits float32 turns outside the margin {flips}")
    assert share <= bc.TIE_SHARE
    assert flips == 0
    fl = bc.floors(bc.F32)                                  # the fp32 floors, whatever the variant stores
    bad = {k: v for k, v in err.items() if not v <= 0.25 * fl[k]}
    assert not bad, bad
    f = bc.truth(case.name, var.tag)
    if case.rows == 1:
        assert not f.var.any() and not f.xhat.any() and float((f.invstd - bc.EPS ** -0.5).abs().max()) < 1e-9
