"""The optimiser passes (csrc/optim.hip) against a float64 restatement of torch.optim.Adam and against the float32 formulas of the
EMA and fill kernels, at sizes on both sides of the 4096 x 256 thread grid (tests/optim_cases.py; conditioning and the derived
floors: tests/test_optim_sweep_cpu.py).  p, exp_avg and exp_avg_sq are each compared, per element, after every call."""
import pytest
import torch

import optim_cases as oc
import rcf_amd  # noqa: F401  (package alias)
from rcf_amd import ops

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
GUARD, TAIL = 7.0, 64


def guarded(t):
    """t on the device as the head of a buffer TAIL elements longer, the tail holding GUARD"""
    buf = torch.full((t.numel() + TAIL,), GUARD, dtype=torch.float32, device=DEV)
    buf[:t.numel()].copy_(t)
    return buf


def same(a, b):
    return torch.equal(a.view(torch.int32), b.view(torch.int32))


@pytest.mark.parametrize("run", oc.PARAMS)
def test_adam_sweep_vs_float64(run, report):
    """four calls on one state (steps 1, 2, 3, 1000); every call twice from the same state (bit-equal), p / exp_avg / exp_avg_sq
    against one float64 update of the state the call started from, p also against the float64 trajectory"""
    n = run.n
    p0, grads = oc.inputs(run)
    st = [guarded(p0), guarded(torch.zeros(n)), guarded(torch.zeros(n))]
    worst = {k: 0.0 for k in oc.FLOORS}
    lines = []
    for call, (step, graw) in enumerate(zip(oc.STEPS, grads), 1):
        g = guarded(graw)
        before = tuple(t[:n].cpu() for t in st)
        alt = [t.clone() for t in st]
        for s in (st, alt):
            ops.adam_step(s[0][:n], g[:n], s[1][:n], s[2][:n], oc.LR, step, betas=(oc.B1, oc.B2), eps=oc.EPS, weight_decay=run.wd,
                          grad_scale=run.gs)
        assert all(same(a, b) for a, b in zip(st, alt)), f"call {call}: two runs from the same state differ"
        assert all(bool((t[n:] == GUARD).all()) for t in st), f"call {call}: an element beyond n was written"
        assert torch.equal(g[:n].cpu(), graw) and bool((g[n:] == GUARD).all()), f"call {call}: the gradient buffer was written"
        e = oc.call_errors(before, tuple(t[:n].cpu() for t in st), run, call)
        lines.append(f"call {call} (step {step}) " + " ".join(f"{k} {v:.2e}" for k, v in e.items()))
        worst = {k: max(worst[k], v) for k, v in e.items()}
    report(f"optim sweep {run.name}: " + "; ".join(lines) + "; worst error / floor " + f"{max(v / oc.FLOORS[k] for k, v in worst.items()):.3f}")
    bad = {k: v for k, v in worst.items() if not v < oc.FLOORS[k]}
    assert not bad, f"{run.name}: over the floor {bad}"
    if run.wd == 0:                       # a gradient that is zero in every call: moments 0, denominator eps, p where it was
        p, m, v = (t[:n].cpu() for t in st)
        assert torch.equal(p[3::10], p0[3::10]) and not m[3::10].any() and not v[3::10].any()


@pytest.mark.parametrize("n", oc.NS)
def test_ema_and_fill_sweep_exact(n, report):
    """rcf_ema_update_f32 at m = 0, 0.999 and 1 and rcf_fill_f32: the float32 formula d m + s (1 - m), bit for bit (the library is
    built without contraction), nothing beyond n written, the source untouched"""
    d, s = oc.ema_inputs(n)
    sg = guarded(s)
    for m in oc.EMA_M:
        def run():
            dg = guarded(d)
            ops.ema_update(dg[:n], sg[:n], m)
            return dg
        a, b = run(), run()
        assert same(a, b), f"m = {m}: two runs differ"
        assert bool((a[n:] == GUARD).all()), f"m = {m}: an element beyond n was written"
        assert torch.equal(a[:n].cpu(), oc.ema_ref(d, s, m)), f"m = {m}: not the float32 formula"
    assert torch.equal(sg[:n].cpu(), s) and bool((sg[n:] == GUARD).all())
    f = guarded(d)
    ops.fill(f[:n], oc.FILL_V)
    assert bool((f[:n] == oc.FILL_V).all()) and bool((f[n:] == GUARD).all())
    report(f"optim sweep n={n}: ema_update exact at m = {oc.EMA_M}, fill exact, guards intact")


def test_optimiser_refuses_what_it_cannot_do():
    """n = 0 and step = 0 are answered with a status before anything is launched"""
    from rcf_amd import _lib
    from rcf_amd.ops import _p, _stream
    t = [torch.full((8,), GUARD, dtype=torch.float32, device=DEV) for _ in range(4)]
    with pytest.raises(_lib.RcfHipError, match="status -1"):
        ops.call("rcf_adam_step_f32", _p(t[0]), _p(t[1]), _p(t[2]), _p(t[3]), 0, 1e-3, 0.9, 0.999, 1e-8, 0.0, 1, 1.0, _stream())
    with pytest.raises(_lib.RcfHipError, match="status -1"):
        ops.adam_step(t[0], t[1], t[2], t[3], 1e-3, 0)
    with pytest.raises(_lib.RcfHipError, match="status -1"):
        ops.call("rcf_ema_update_f32", _p(t[0]), _p(t[1]), 0, 0.5, _stream())
    with pytest.raises(_lib.RcfHipError, match="status -1"):
        ops.call("rcf_fill_f32", _p(t[0]), 0, 1.0, _stream())
    torch.cuda.synchronize()
    assert all(bool((x == GUARD).all()) for x in t)
