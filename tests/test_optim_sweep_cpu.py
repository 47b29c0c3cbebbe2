"""Conditioning of the optimiser sweep (tests/optim_cases.py): the table reaches the stride loops' second and third trips and the
inputs hold what they name, and the reference's own float32 run sits within a quarter of each floor of its float64 run, after
every one of the four calls.  Then a kernel that misses a floor in tests/test_optim_sweep_gpu.py is wrong, not unlucky."""
import math

import pytest
import torch

import optim_cases as oc


def test_table_reaches_what_it_names():
    assert oc.NS == (1, 255, 257, 4096 * 256 - 1, 4096 * 256 + 5, 2 * 4096 * 256 + 3)
    trips = [-(-n // oc.GRID) for n in oc.NS]                                       # trips of the busiest thread's stride loop
    assert trips == [1, 1, 1, 1, 2, 3] and max(oc.NS) * 4 < 8.5e6                   # a second and a third trip; 8 MB at the most
    assert oc.STEPS == (1, 2, 3, 1000) and {(r.wd > 0, r.gs) for r in oc.RUNS} == {(False, 1.0), (True, 1.0 / 1024)}
    assert len(oc.RUNS) == 12 and math.log2(1 / oc.HYPER[1][1]) == 10
    # the bound test_adam_and_ema holds p to would pass a kernel without the bias correction of v at step 3: not this one
    assert 1 / math.sqrt(1 - oc.B2 ** 3) > 10
    for r in (oc.RUNS[3], oc.RUNS[4]):                                              # n = 255: both hyper-parameter sets
        p0, grads = oc.inputs(r)
        assert 3e-3 < float(p0.abs().mean()) < 3e-2 and oc.LR > 1e4 * float(p0.abs().max()) * 2.0 ** -23
        for g in grads:
            eff = g.double() * r.gs
            nz = eff[eff != 0].abs()
            assert float(nz.min()) >= 0.99e-6 and float(nz.max()) <= 1.01e2 and float(nz.min()) < 1e-5 and float(nz.max()) > 10
            assert bool((eff[3::10] == 0).all()) and 0.1 < float((eff == 0).double().mean()) < 0.3
            assert bool((eff > 0).any()) and bool((eff < 0).any())
    # a zero gradient without weight decay: both moments stay 0, the denominator is eps, p stays where it was -- exactly
    r = oc.RUNS[2]
    assert r.n == 255 and r.wd == 0
    p0, _ = oc.inputs(r)
    for p, m, v in oc.truth(r):
        assert torch.equal(p[3::10], p0.double()[3::10]) and not m[3::10].any() and not v[3::10].any()


@pytest.mark.parametrize("run", oc.PARAMS)
def test_reference_float32_error_is_a_quarter_of_the_floor(run):
    worst = {k: 0.0 for k in oc.FLOORS}
    before = (oc.inputs(run)[0], torch.zeros(run.n), torch.zeros(run.n))
    for call, got in enumerate(oc.trajectory(run, torch.float32), 1):
        e = oc.call_errors(before, got, run, call)
        print(f"optim sweep {run.name} call {call} (step {oc.STEPS[call - 1]}): reference fp32 vs fp64 " + " ".join(f"{k} {v:.2e}" for k, v in e.items()))
        worst = {k: max(worst[k], v) for k, v in e.items()}
        before = got
    bad = {k: v for k, v in worst.items() if not v <= 0.25 * oc.FLOORS[k]}
    assert not bad, bad
    assert oc.FLOOR_P <= 5e-3 and oc.FLOOR_P_TRAJ <= 5e-3                            # never looser than test_adam_and_ema's bound


def test_ema_formula_edges():
    d, s = oc.ema_inputs(257)
    assert torch.equal(oc.ema_ref(d, s, 0.0), s) and torch.equal(oc.ema_ref(d, s, 1.0), d)
    y = oc.ema_ref(d, s, 0.999)
    assert y.dtype == torch.float32 and float((y.double() - (0.999 * d.double() + 0.001 * s.double())).abs().max()) < 1e-3
