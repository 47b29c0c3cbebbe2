"""The cost-volume kernels (csrc/correlation.hip) against the float64 restatement of tests/correlation_cases.py (its conditioning:
tests/test_correlation_cpu.py).  Errors are taken PER ELEMENT against (C + 2) u mass (forward) and (D^2 + 2) u mass (each
gradient), u = 2^-24; non-finite elements must be the restatement's; the exact case is bit-equal; every call is made twice and
must repeat its bits; outputs start as a sentinel, so an element the kernel leaves alone, or adds into, shows.  The last test
reports the worst error / bound per family; those lines are what profiles/correlation_sweep_parity.txt keeps."""
import os
from ctypes import c_void_p

import numpy as np
import pytest
import torch

import correlation_cases as cc
import rcf_amd
from rcf_amd import ops

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
SENTINEL = -777.25
ALL = [pytest.param(c, id=c.name) for c in cc.CASES]
WORST = {}


def P(t):
    return None if t is None else c_void_p(t.data_ptr())


def G(a):
    return torch.from_numpy(np.ascontiguousarray(a)).to(DEV)


def N(t):
    return t.cpu().numpy()


def same(a, b):
    """bit-equal, NaN == NaN"""
    return a.shape == b.shape and torch.equal(a.contiguous().view(torch.uint8), b.contiguous().view(torch.uint8))


def fwd(x1, x2, d, slope):
    B, C, H, W = x1.shape
    out = torch.full((B, (2 * d + 1) ** 2, H, W), SENTINEL, device=DEV)
    ops.call("rcf_correlation_fwd_f32", P(x1), P(x2), P(out), B, C, H, W, d, slope, ops._stream())
    return out


def bwd(x1, x2, dout, out, d, slope, want1=True, want2=True):
    B, C, H, W = x1.shape
    dx1 = torch.full_like(x1, SENTINEL) if want1 else None
    dx2 = torch.full_like(x2, SENTINEL) if want2 else None
    ops.call("rcf_correlation_bwd_f32", P(x1), P(x2), P(dout), P(out), P(dx1), P(dx2), B, C, H, W, d, slope, ops._stream())
    return dx1, dx2


def note(family, name, m):
    if m >= WORST.get(family, (-1.0, ""))[0]:
        WORST[family] = (m, name)


# ================================================================================================================ forward
@pytest.mark.parametrize("c", ALL)
def test_forward_vs_float64(c, report):
    d = cc.inputs(c)
    x1, x2 = G(d["x1"]), G(d["x2"])
    ref, mass = cc.fwd_truth(c)
    out, again = fwd(x1, x2, c.d, c.slope), fwd(x1, x2, c.d, c.slope)
    m = cc.margin(N(out), ref, cc.fwd_bound(mass, c.C))
    report(f"correlation sweep forward {c.name}: worst error / bound {m:.3f}; second call bit-equal {same(out, again)}")
    note(f"forward {c.kind}" + (" leaky" if c.slope != 1.0 else ""), c.name, m)
    assert m <= 1.0, c.name
    assert same(out, again), "the forward does not repeat its bits"
    if c.kind == "exact":
        want = torch.from_numpy(ref.astype(np.float32))
        assert np.array_equal(want.numpy().astype(np.float64), ref) and same(out.cpu(), want), "out is not x2z bit for bit"
    if c.slope != 1.0:                                   # the fused activation is leaky_relu of the plain result, bit for bit
        plain = fwd(x1, x2, c.d, 1.0)
        assert same(out, torch.nn.functional.leaky_relu(plain, c.slope))


# =============================================================================================================== backward
@pytest.mark.parametrize("c", ALL)
def test_backward_vs_float64(c, report):
    d = cc.inputs(c)
    x1, x2, dout = G(d["x1"]), G(d["x2"]), G(d["dout"])
    act = G(d["mask_out"]) if c.slope != 1.0 else None
    r1, m1, r2, m2 = cc.bwd_truth(c)
    dx1, dx2 = bwd(x1, x2, dout, act, c.d, c.slope)
    e1, e2 = cc.margin(N(dx1), r1, cc.grad_bound(m1, c.d)), cc.margin(N(dx2), r2, cc.grad_bound(m2, c.d))
    a1, a2 = bwd(x1, x2, dout, act, c.d, c.slope)
    only1, none2 = bwd(x1, x2, dout, act, c.d, c.slope, want2=False)
    none1, only2 = bwd(x1, x2, dout, act, c.d, c.slope, want1=False)
    rep = same(dx1, a1) and same(dx2, a2)
    alone = none1 is None and none2 is None and same(dx1, only1) and same(dx2, only2)
    report(f"correlation sweep backward {c.name}: worst error / bound dx1 {e1:.3f} dx2 {e2:.3f}; second call bit-equal {rep}; "
           f"each gradient alone bit-equal {alone}")
    tag = f" {c.kind}" + (" leaky" if c.slope != 1.0 else "")
    note("dx1" + tag, c.name, e1)
    note("dx2" + tag, c.name, e2)
    assert e1 <= 1.0 and e2 <= 1.0, c.name
    assert rep, "the backward does not repeat its bits"
    assert alone, "a gradient changes when the other is not asked for"
    if c.slope == 1.0:                                   # `out` is not read when slope == 1
        junk = torch.full((c.B, c.D ** 2, c.H, c.W), float("nan"), device=DEV)
        j1, j2 = bwd(x1, x2, dout, junk, c.d, 1.0)
        assert same(dx1, j1) and same(dx2, j2)


# ================================================================================================== module and autograd
@pytest.mark.parametrize("c", [pytest.param(c, id=c.name) for c in cc.CASES if c.kind == "gauss"][::4])
def test_module_backward_gives_the_bits_of_the_ops(c):
    d = cc.inputs(c)
    x1, x2, dout = G(d["x1"]).requires_grad_(True), G(d["x2"]).requires_grad_(True), G(d["dout"])
    mod = rcf_amd.Correlation(c.d, 1, stride1=1, slope=c.slope)
    out = mod(x1, x2)
    out.backward(dout)
    o = ops.correlation(x1.detach(), x2.detach(), c.d, c.slope)
    g1, g2 = ops.correlation_bwd(x1.detach(), x2.detach(), dout, o if c.slope != 1.0 else None, c.d, c.slope)
    assert same(out.detach(), o) and same(out.detach(), fwd(x1.detach(), x2.detach(), c.d, c.slope))
    assert same(x1.grad, g1) and same(x2.grad, g2)
    # needs_input_grad: only the asked-for gradient is made, and it is the same one
    a, b = G(d["x1"]).requires_grad_(True), G(d["x2"])
    mod(a, b).backward(dout)
    assert same(a.grad, g1) and b.grad is None
    a, b = G(d["x1"]), G(d["x2"]).requires_grad_(True)
    mod(a, b).backward(dout)
    assert same(b.grad, g2) and a.grad is None
    assert not mod(G(d["x1"]), G(d["x2"])).requires_grad
    # a non-contiguous view goes through .contiguous()
    xt = G(np.ascontiguousarray(d["x1"].transpose(0, 1, 3, 2))).transpose(2, 3)
    assert not xt.is_contiguous() or min(c.H, c.W) == 1
    assert same(ops.correlation(xt, x2.detach(), c.d, c.slope), o)


@pytest.mark.parametrize("slope", [1.0, 0.1])
def test_against_the_torch_composition_in_float64(slope, report):
    """the reference's 81-slice composition restated in torch, float64, on the device, with autograd"""
    B, C, H, W, d = cc.COMPOSITION_SHAPE
    g = torch.Generator().manual_seed(3309)
    x1, x2 = torch.randn(B, C, H, W, generator=g), torch.randn(B, C, H, W, generator=g)
    dout = torch.randn(B, 81, H, W, generator=g)
    a, b = x1.to(DEV).double().requires_grad_(True), x2.to(DEV).double().requires_grad_(True)
    o64 = cc.torch_composition(a, b, d, float(np.float32(slope)))
    o64.backward(dout.to(DEV).double())
    p, q = x1.to(DEV).requires_grad_(True), x2.to(DEV).requires_grad_(True)
    out = rcf_amd.Correlation(d, slope=slope)(p, q)
    out.backward(dout.to(DEV))
    _, mass = cc.corr_ref(x1.numpy(), x2.numpy(), d)
    # the gradient masks are the kernel's own output's: elements where it and the float64 run disagree in sign would be a tie set
    flips = int(((out.detach() > 0) != (o64.detach() > 0)).sum()) if slope != 1.0 else 0
    _, m1, _, m2 = cc.corr_bwd_ref(x1.numpy(), x2.numpy(), dout.numpy(), d, slope, N(out.detach()))
    e = (cc.margin(N(out.detach()), N(o64.detach()), cc.fwd_bound(mass, C)), cc.margin(N(p.grad), N(a.grad), cc.grad_bound(m1, d)),
         cc.margin(N(q.grad), N(b.grad), cc.grad_bound(m2, d)))
    report(f"correlation vs the float64 torch composition {cc.COMPOSITION_SHAPE} slope {slope}: error / bound out {e[0]:.3f} dx1 {e[1]:.3f} "
           f"dx2 {e[2]:.3f}; activation sign flips {flips}")
    note("torch composition float64", f"slope {slope}", max(e))
    assert flips == 0 and max(e) <= 1.0


# ================================================================================================================ golden
@pytest.mark.parametrize("k", range(len(cc.GOLDEN_SHAPES)))
def test_golden_cases_on_the_device(k, golden_dir, report):
    z = np.load(os.path.join(golden_dir, "correlation.npz"))
    B, C, H, W, d = cc.GOLDEN_SHAPES[k]
    x1, x2, dout = z[f"x1_{k}"], z[f"x2_{k}"], z[f"dout_{k}"]
    _, mass = cc.corr_ref(x1, x2, d)
    _, m1, _, m2 = cc.corr_bwd_ref(x1, x2, dout, d)
    out = fwd(G(x1), G(x2), d, 1.0)
    dx1, dx2 = bwd(G(x1), G(x2), G(dout), None, d, 1.0)
    e = (cc.margin(N(out), z[f"out64_{k}"], cc.fwd_bound(mass, C)), cc.margin(N(dx1), z[f"dx1_64_{k}"], cc.grad_bound(m1, d)),
         cc.margin(N(dx2), z[f"dx2_64_{k}"], cc.grad_bound(m2, d)))
    report(f"correlation golden {cc.GOLDEN_SHAPES[k]} against the reference's float64 run: error / bound out {e[0]:.3f} dx1 {e[1]:.3f} dx2 {e[2]:.3f}")
    note("golden (reference float64)", str(cc.GOLDEN_SHAPES[k]), max(e))
    assert max(e) <= 1.0


# ============================================================================================================== refusals
def test_entries_refuse_and_write_nothing():
    x = torch.randn(1, 2, 3, 4, device=DEV)
    outs = [torch.full((1, 81, 3, 4), 7.0, device=DEV), torch.full((1, 2, 3, 4), 7.0, device=DEV), torch.full((1, 2, 3, 4), 7.0, device=DEV)]
    o, g1, g2 = outs
    st = ops._stream()

    def refused(name, *args):
        with pytest.raises(rcf_amd._lib.RcfHipError, match="status -1"):
            ops.call(name, *args)
    for d in (0, 5):
        refused("rcf_correlation_fwd_f32", P(x), P(x), P(o), 1, 2, 3, 4, d, 1.0, st)
        refused("rcf_correlation_bwd_f32", P(x), P(x), P(o), P(o), P(g1), P(g2), 1, 2, 3, 4, d, 1.0, st)
    for dims in ((0, 2, 3, 4), (1, 0, 3, 4), (1, 2, 0, 4), (1, 2, 3, 0), (1, 1, 5155, 5155)):
        refused("rcf_correlation_fwd_f32", P(x), P(x), P(o), *dims, 4, 1.0, st)
        refused("rcf_correlation_bwd_f32", P(x), P(x), P(o), P(o), P(g1), P(g2), *dims, 4, 1.0, st)
    for k in range(3):
        a = [P(x), P(x), P(o)]
        a[k] = None
        refused("rcf_correlation_fwd_f32", *a, 1, 2, 3, 4, 4, 1.0, st)
        refused("rcf_correlation_bwd_f32", *a, P(o), P(g1), P(g2), 1, 2, 3, 4, 4, 1.0, st)
    refused("rcf_correlation_bwd_f32", P(x), P(x), P(o), P(o), None, None, 1, 2, 3, 4, 4, 1.0, st)
    refused("rcf_correlation_bwd_f32", P(x), P(x), P(o), None, P(g1), P(g2), 1, 2, 3, 4, 4, 0.1, st)
    with pytest.raises(rcf_amd._lib.RcfHipError):
        ops.correlation(x.cpu(), x.cpu())
    with pytest.raises(rcf_amd._lib.RcfHipError):
        ops.correlation(x.half(), x.half())
    torch.cuda.synchronize()
    assert all(bool((v == 7.0).all()) for v in outs), "a refused call wrote to an output"


# =============================================================================================================== summary
def test_worst_margins_per_family(report):
    """last in the file: what the tests above noted, one line per family (empty when they were deselected)"""
    TH, TW, CK = cc.geometry()
    if WORST:
        report(f"correlation sweep summary: {len(cc.CASES)} cases, tile {TH} x {TW}, {CK} channels per trip; worst error / bound per family")
    for fam in sorted(WORST):
        report(f"correlation sweep worst {fam}: {WORST[fam][0]:.3f}  ({WORST[fam][1]})")
        assert WORST[fam][0] <= 1.0
