"""CPU: every case and variant of tests/wgrad_cases.py takes the kernel, the tile and the split-K factor its table says
(rcf_conv_plan_of, the library's own answer), so the bit fixture of tests/test_wgrad_bits_gpu.py cannot silently stop reaching an
instantiation of the tap-column weight-gradient kernels."""
import pytest

import wgrad_cases as wg


@pytest.mark.parametrize("c", wg.CASES, ids=lambda c: c.name)
def test_wgrad_case_takes_the_planned_kernel(c):
    for v in wg.variants(c):
        want = c.plan[wg.PLAN_KEY[v]]
        got = wg.plan_of(c, v)
        assert got == want, f"case {c.name} {v}: plan (kernel, rows, cols, split) {got}, the table says {want}"


def test_wgrad_cases_reach_every_instantiation():
    """kernel x tile x region x split, as planned: the four kernels, every tile each of them has, with and without a region
    (the fp32 planner gives a region on fewer than 256 columns to the tap-as-grid-row kernels: the 128 x 128 tiles of the fp32
    kernels have no region instance), with and without split-K"""
    seen = {(c.plan[wg.PLAN_KEY[v]][:3], c.region is not None) for c in wg.CASES for v in wg.variants(c)}
    for tile in ((wg.H2T, 256, 256), (wg.H2T, 128, 256), (wg.H2D, 128, 256), (wg.H16_DMA, 128, 256), (wg.H16_DMA, 128, 128),
                 (wg.H16, 64, 256), (wg.H16, 64, 128), (wg.H16, 64, 64), (wg.H16, 128, 64)):
        assert (tile, False) in seen and (tile, True) in seen, tile
    for tile in ((wg.H2T, 128, 128), (wg.H2D, 128, 128)):           # no region instance exists: igemm_conv.hip plan_wgrad
        assert (tile, False) in seen, tile
    for key in ("h2", "tile128", "planes", "h16"):
        splits = {c.plan[key][3] for c in wg.CASES if key in c.plan}
        assert 1 in splits and max(splits) > 1, key
