"""Conditioning of the flow-head sweep (tests/flowhead_cases.py): the oracle's own float32 run must sit within a quarter
of each tolerance floor of its float64 run, on every loss term, flow map and gradient of every case.  Then a kernel
that misses a floor in tests/test_flowhead_sweep_gpu.py is wrong, not unlucky.  A case that cannot meet this is badly
conditioned (near-singular S_ww, a hinge or |.| tie within float32 rounding) and gets other inputs, never a looser limit."""
import pytest

import flowhead_cases as fc


def test_case_table_covers_the_kernel_limits():
    """the table itself: the limits of make_cfg and the launch geometry it is there to reach"""
    by = fc.BY_NAME
    D = {"free": 0, "affine": 2, "quadratic": 5}
    assert max(2 * c.B * c.C for c in fc.CASES) == 256                          # one-block kernels, 256 threads
    assert max((2 + 2 * D[c.mode]) * c.C for c in fc.CASES) == 96                # PARTW
    assert sum(c.h * c.w > 512 * 4 * 64 for c in fc.CASES) >= 2                  # second trip of bwd_pixel_kernel
    assert any(c.h * c.w < 64 for c in fc.CASES) and any(c.h == 1 for c in fc.CASES)
    assert {1, 2, 3, 5, 8} <= {c.C for c in fc.CASES}                            # pitch > C four ways, and CMAX
    assert all((c.h * c.w) % 64 for c in fc.CASES)                               # every last 64-pixel group is partial
    assert 2 * sum(c.w_seg == 2.0 for c in fc.CASES) >= len(fc.CASES)
    assert by["row_linear"].res_scale == -1.0 and by["quad_kl"].res_size == (7, 9)


@pytest.mark.parametrize("case", fc.PARAMS_CASES)
def test_oracle_float32_error_is_a_quarter_of_the_floor(case):
    err = fc.ref32_errors(case)
    print(f"flow head sweep {case.name}: oracle fp32 vs fp64 " + " ".join(f"{k} {v:.2e}" for k, v in err.items()))
    truth = fc.cached_reference(case.name, True)
    expect = {"loss", "loss_warp_seg"}
    expect |= {"loss_sharpen"} if case.w_sharpen > 0 else ({"loss_entropy"} if case.w_entropy > 0 else set())
    expect |= {"loss_compactness"} if case.compact_channel is not None else set()
    expect |= {"loss_pl", "loss_crf"} if case.targets else set()
    assert set(truth["losses"]) == expect
    assert ("aff" in truth["flows"]) == (case.mode != "free")
    assert truth["tie"] > 0.9 * fc.TIE_MARGIN                                    # no |.| tie within float32's reach
    if case.C == 1:
        assert not truth["dlogits"].any()                                        # softmax of one channel is constant
    bad = {k: v for k, v in err.items() if not v <= 0.25 * fc.floor_of(case, k)}
    assert not bad, bad
