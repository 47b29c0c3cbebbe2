"""CPU: every case and variant of tests/conv_cases.py takes the kernel and the tile its table says, forward and data gradient
(rcf_conv_plan_of, the library's own answer), so the bit fixture of tests/test_conv_bits_gpu.py cannot silently stop reaching an
instantiation of the forward / data-gradient conv kernels."""
import pytest

import conv_cases as cc


@pytest.mark.parametrize("c", cc.CASES, ids=lambda c: c.name)
def test_conv_case_takes_the_planned_kernel(c):
    for v in c.variants:
        for direction in (0, 1):
            want = c.plan[cc.PLAN_KEY[v]][direction]
            got = cc.plan_of(c, v, direction)
            assert got == want, f"case {c.name} {v} direction {direction}: plan (kernel, rows, cols) {got}, the table says {want}"


def test_conv_cases_reach_every_kernel_and_tile():
    """kernel x tile x direction (forward, data gradient, strided data gradient), with and without a region where an instance
    exists: igemm_conv_kernel takes no region (fwd_params / dgrad_params refuse it), a strided launch walks no tap list and the
    table's strided cases are whole tensors; conv_h2p_kernel has no strided form (h2p_eligible)"""
    seen = set()
    for c in cc.CASES:
        for v in c.variants:
            for direction in (0, 1):
                way = ("fwd", "strided" if c.stride > 1 else "dgrad")[direction]
                seen.add((c.plan[cc.PLAN_KEY[v]][direction], way, c.region is not None, v))
    reach = lambda kernel, tile, way, region, variants: all(((kernel,) + tile, way, region, v) in seen for v in variants)
    for tile in (cc.S64, cc.L64, cc.S128, cc.S256):
        for way in ("fwd", "dgrad"):
            assert reach(cc.TILE, tile, way, False, cc.F32) and reach(cc.TILE, tile, way, True, cc.F32), (tile, way)
        assert reach(cc.TILE, tile, "strided", False, cc.F32 + ("lean",)), tile
        assert reach(cc.TILE, tile, "dgrad", False, ("lean",)), tile
    for tile in (cc.L64, cc.S128, cc.S256):                           # conv_h2d_kernel NR 1, 2, 4; conv_bf16_kernel's column tiles
        for way in ("fwd", "dgrad"):
            assert reach(cc.H2D, tile, way, False, ("planes",)) and reach(cc.H2D, tile, way, True, ("planes",)), (tile, way)
            assert reach(cc.H16, tile, way, False, cc.H16_VARIANTS) and reach(cc.H16, tile, way, True, cc.H16_VARIANTS), (tile, way)
        assert reach(cc.H2D, tile, "strided", False, ("planes", "leanp")) and reach(cc.H2D, tile, "dgrad", False, ("leanp",)), tile
        assert reach(cc.H16, tile, "strided", False, cc.H16_VARIANTS), tile
    for way in ("fwd", "dgrad"):
        assert reach(cc.H2P, (32, 256), way, False, ("h2p",)) and reach(cc.H2P, (32, 256), way, True, ("h2p",)), way
    for tile in (cc.L64, cc.S128):                                    # igemm_conv_kernel narrow and wide
        for way in ("fwd", "dgrad", "strided"):
            assert reach(cc.MFMA, tile, way, False, cc.MFMAS), (tile, way)
    # the switches and the tap-list loop's source frame, on the tiles the module's docstring names
    by_name = {c.name: c for c in cc.CASES}
    assert "natural" in by_name["C"].variants and by_name["C"].Cin >= 256 and by_name["C"].k == 3
    assert "nocolmap" in by_name["B"].variants
    assert {"A", "B", "C", "Cf"} <= {c.name for c in cc.CASES if "band" in c.variants}
