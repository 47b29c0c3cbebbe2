"""The flow-loss kernels (csrc/unflow.hip) and rcf_amd.unFlowLoss against the float64 restatement of tests/unflow_cases.py (its
conditioning: tests/test_unflow_cpu.py) and the reference-made fixture.

Scalars (every loss term and the total): relative error <= 1e-4 against float64, NaN equal to NaN.  Gradients, per tensor:
max |err| <= max(6 e32, 16 u max |g64|) outside the tie set of the non-smooth points, e32 being the worst error of the SAME
arithmetic run in float32 by torch on the CPU (computed here, never taken from the kernels); the fixture cases use the
reference's own float32 run.  Area outputs: (n + 2) u mass per element.  Every call is made twice and must repeat its bits;
gradient buffers start as a sentinel.  The last test reports the worst error / bound per group; those lines are what
profiles/unflow_sweep_parity.txt keeps."""
import os
from ctypes import c_void_p

import numpy as np
import pytest
import torch

import unflow_cases as uc
import rcf_amd
from rcf_amd import ops

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
SENTINEL = -777.25
WORST = {}


def P(t):
    return None if t is None else c_void_p(t.data_ptr())


def G(a):
    return torch.from_numpy(np.ascontiguousarray(a)).to(DEV)


def N(t):
    return t.detach().cpu().numpy()


def same(a, b):
    """bit-equal, NaN == NaN"""
    return a.shape == b.shape and torch.equal(a.reshape(-1).contiguous().view(torch.uint8), b.reshape(-1).contiguous().view(torch.uint8))


def note(group, name, m):
    if m >= WORST.get(group, (-1.0, ""))[0]:
        WORST[group] = (m, name)


def ratio(err, bound):
    return 0.0 if err == 0 else (err / bound if bound > 0 else float("inf"))


def photo_bwd(im, other, flow, occ, stats, c):
    """the entry point itself, dflow starting as a sentinel; flow is a channel slice of a [B, 4, h, w] tensor"""
    B, _, h, w = flow.shape
    dflow = torch.full((B, 2, h, w), SENTINEL, device=DEV)
    one = torch.ones(1, device=DEV)
    ops.call("rcf_unflow_photo_bwd_f32", P(im), P(other), P(flow), flow.stride(0), P(occ), occ.shape[2], occ.shape[3], c.md,
             *[float(v) for v in c.weights], P(one), P(stats), P(dflow), B, h, w, ops._stream())
    return dflow


# ============================================================================================================ photometric
@pytest.mark.parametrize("c", [pytest.param(c, id=c.name) for c in uc.CASES])
def test_photometric_vs_float64(c, report):
    d = uc.inputs(c)
    p, e32, _ = uc.photo_truth(c)
    im, other, occ = G(d["im"]), G(d["other"]), G(d["occ"])
    wide = torch.full((c.B, 4, c.h, c.w), float("nan"), device=DEV)
    wide[:, 2:] = G(d["flow"])
    flow = wide[:, 2:]                                    # read in place: batch stride 4 h w, offset 2 h w
    loss, stats = ops.unflow_photo(im, other, flow, occ, c.md, *c.weights)
    loss2, stats2 = ops.unflow_photo(im, other, G(d["flow"]), occ, c.md, *c.weights)
    got = [float(v) for v in N(stats)]
    want = [p.loss, p.l1, p.ssim, p.tern, p.occ_mean]
    on = [True, c.weights[0] > 0, c.weights[1] > 0, c.weights[2] > 0, True]
    rels = [uc.rel_err(g, r) if k else 0.0 for g, r, k in zip(got, want, on)]
    line = f"unflow photo {c.name}: relative error loss {rels[0]:.1e} L1 {rels[1]:.1e} SSIM {rels[2]:.1e} ternary {rels[3]:.1e} mask mean {rels[4]:.1e}"
    note(f"photo forward md{c.md}", c.name, max(rels) / uc.SCALAR_RTOL)
    assert same(stats, stats2) and same(loss, stats[0]), "the forward does not repeat its bits (or reads a strided flow differently)"
    if c.grad:
        dflow, again = photo_bwd(im, other, flow, occ, stats, c), photo_bwd(im, other, flow, occ, stats, c)
        err, bound = uc.max_err(N(dflow), p.dflow, p.tie[:, None]), uc.grad_bound(e32, p.dflow)
        line += f"; dflow max error {err:.2e}, bound {bound:.2e} (e32 {e32:.1e}, max |g| {np.abs(p.dflow).max():.1e}), error / bound {ratio(err, bound):.3f}"
        note(f"photo dflow md{c.md}" + (" ternary" if c.weights[2] > 0 else ""), c.name, ratio(err, bound))
    report(line)
    assert max(rels) <= uc.SCALAR_RTOL, line
    if c.grad:
        assert same(dflow, again), "the backward does not repeat its bits"
        assert not bool((dflow == SENTINEL).any()), "an element of dflow was left alone"
        assert err <= bound, line
        via_op = ops.unflow_photo_bwd(im, other, flow, occ, stats, torch.ones((), device=DEV), c.md, *c.weights)
        assert same(via_op, dflow)
        twice = ops.unflow_photo_bwd(im, other, flow, occ, stats, torch.full((), 2.0, device=DEV), c.md, *c.weights)
        assert np.abs(N(twice) - 2 * N(dflow)).max() <= 4 * uc.U * np.abs(N(dflow)).max()     # the upstream gradient comes from the device
    else:
        assert np.isnan(got[0]) == np.isnan(p.loss)


# ============================================================================================================= smoothness
@pytest.mark.parametrize("h,w,second", uc.SMOOTH_CASES)
def test_smoothness_vs_float64(h, w, second, report):
    im, fl = uc.smooth_inputs(h, w, second)
    s = float(min(h, w))
    T = torch.from_numpy
    ref, g64, tie = uc.smooth_analytic(T(fl).double(), T(im).double(), 10.0, s, second)
    _, g32 = uc.smooth_autograd(T(fl), T(im), 10.0, s, second)
    e32 = uc.max_err(g32, g64, tie)
    wide = torch.full((2, 4, h, w), float("nan"), device=DEV)
    wide[:, :2] = G(fl)
    out, out2 = ops.unflow_smooth(wide[:, :2], G(im), 10.0, s, second), ops.unflow_smooth(G(fl), G(im), 10.0, s, second)
    rel = uc.rel_err(float(out), ref)
    one = torch.ones((), device=DEV)
    g, again = ops.unflow_smooth_bwd(wide[:, :2], G(im), one, 10.0, s, second), ops.unflow_smooth_bwd(G(fl), G(im), one, 10.0, s, second)
    err, bound = uc.max_err(N(g), g64, tie), uc.grad_bound(e32, g64)
    order = "second" if second else "first"
    report(f"unflow smooth {order} {h}x{w}: relative error {rel:.1e}; dflow max error {err:.2e}, bound {bound:.2e}, error / bound {ratio(err, bound):.3f}")
    note(f"smooth {order} forward", f"{h}x{w}", rel / uc.SCALAR_RTOL)
    note(f"smooth {order} dflow", f"{h}x{w}", ratio(err, bound))
    assert same(out, out2) and same(g, again)
    assert rel <= uc.SCALAR_RTOL and err <= bound
    if h * w > 20:                               # the planted zero differences were compared: sign(0) = 0
        assert not tie[0, 0, 1, :3].any()


# =================================================================================================================== area
@pytest.mark.parametrize("H,W,h,w", uc.AREA_CASES)
def test_area_resize_vs_float64(H, W, h, w, report):
    g = torch.Generator().manual_seed(H * W + h)
    pair = torch.rand(2, 6, H, W, generator=g)
    dev = pair.to(DEV)
    worst = 0.0
    for k in (0, 3):
        ref, mass, n = uc.area_ref(pair[:, k:k + 3].numpy(), h, w)
        out = ops.area_resize(dev[:, k:k + 3], (h, w))           # a channel slice read in place
        assert same(out, ops.area_resize(dev[:, k:k + 3].contiguous(), (h, w)))
        d = np.abs(N(out) - ref)
        worst = max(worst, float((d / uc.area_bound(mass, n)).max()))
        if (H, W) == (h, w):
            assert same(out, dev[:, k:k + 3])
    report(f"unflow area {H}x{W} -> {h}x{w}: worst error / bound {worst:.3f}")
    note("area", f"{H}x{W}->{h}x{w}", worst)
    assert worst <= 1.0


# ================================================================================================================= module
def run_module(cfg, flows, target, mod=None):
    mod = mod or rcf_amd.unFlowLoss(cfg)
    leaves = [G(f).requires_grad_(True) for f in flows]
    out = mod(leaves, target if torch.is_tensor(target) else G(target))
    assert all(torch.is_tensor(v) and v.dim() == 0 and v.is_cuda for v in out)
    out[0].backward()
    return mod, out, leaves


def check_module(name, cfg, flows, target, ref, e32s, report, group):
    mod, out, leaves = run_module(cfg, flows, target)
    _, out2, leaves2 = run_module(cfg, flows, target)
    got = [float(v.detach()) for v in out]
    want = [ref["total"], ref["warp"], ref["smooth"], ref["absmean"]]
    rels = [uc.rel_err(g, r) for g, r in zip(got, want)]
    lines = [f"unflow module {name}: relative error total {rels[0]:.1e} warp {rels[1]:.1e} smooth {rels[2]:.1e} |flow| {rels[3]:.1e}"]
    worst = 0.0
    for l, (leaf, g64, tie, e32) in enumerate(zip(leaves, ref["grads"], ref["ties"], e32s)):
        if g64 is None:
            assert leaf.grad is None or not bool(leaf.grad.any())
            continue
        err, bound = uc.max_err(N(leaf.grad), g64, tie), uc.grad_bound(e32, g64)
        worst = max(worst, ratio(err, bound))
        lines.append(f"unflow module {name} level {l}: dflow max error {err:.2e}, bound {bound:.2e} (e32 {e32:.1e}), error / bound {ratio(err, bound):.3f}")
        assert same(leaf.grad, leaves2[l].grad), "the module's backward does not repeat its bits"
    for line in lines:
        report(line)
    note(f"{group} values", name, max(rels) / uc.SCALAR_RTOL)
    note(f"{group} dflow", name, worst)
    assert all(same(a, b) for a, b in zip(out, out2))
    assert same(mod.pyramid_occu_mask1[0].cpu(), torch.from_numpy(ref["mask1"]).float()), "mask 1 differs"
    assert same(mod.pyramid_occu_mask2[0].cpu(), torch.from_numpy(ref["mask2"]).float()), "mask 2 differs"
    live = [f for i, f in enumerate(flows) if cfg.w_scales[i] != 0]
    assert [tuple(m.shape[2:]) for m in mod.pyramid_occu_mask1] == [f.shape[2:] for f in live]
    for m, f in zip(mod.pyramid_occu_mask2, live):
        assert same(m.cpu(), torch.from_numpy(uc.nearest_mask(ref["mask2"], *f.shape[2:])).float())
    assert max(rels) <= uc.SCALAR_RTOL and worst <= 1.0, "\n".join(lines)


@pytest.mark.parametrize("k", range(len(uc.module_cases())))
def test_module_vs_float64(k, report):
    name, cfg, (B, H, W), levels = uc.module_cases()[k]
    flows, target, _ = uc.pyramid_inputs(B, H, W, levels, 4100 + k)
    ref = uc.loss_ref(cfg, flows, target)
    r32 = uc.loss_ref(cfg, flows, target, dt=torch.float32, analytic=False)
    e32s = [None if g is None else uc.max_err(g32, g, t) for g, g32, t in zip(ref["grads"], r32["grads"], ref["ties"])]
    check_module(name, cfg, flows, target, ref, e32s, report, "module")


@pytest.mark.parametrize("k", range(len(uc.golden_cfgs())))
def test_module_vs_the_reference_fixture(k, golden_dir, report):
    z = np.load(os.path.join(golden_dir, "unflow.npz"))
    name, cfg, levels = uc.golden_cfgs()[k]
    flows, target = [z[f"flow_{l}"] for l in range(levels)], z["target"]
    mine = uc.loss_ref(cfg, flows, target)                       # for the tie set alone
    v = z[f"vals64_{k}"]
    sub = lambda a: a.reshape(-1)[::uc.GOLDEN_STRIDE]
    mod, out, leaves = run_module(cfg, flows, target)
    rels = [uc.rel_err(float(g.detach()), float(r)) for g, r in zip(out, v)]
    lines = [f"unflow golden {name} against the reference's float64 run: relative error total {rels[0]:.1e} warp {rels[1]:.1e} smooth {rels[2]:.1e} |flow| {rels[3]:.1e}"]
    worst = 0.0
    for l in range(levels):
        if cfg.w_scales[l] == 0:
            continue
        g64, g32, tie = z[f"g64_{k}_{l}"], z[f"g32_{k}_{l}"], sub(mine["ties"][l])
        e32 = uc.max_err(g32, g64, tie)
        err, bound = uc.max_err(sub(N(leaves[l].grad)), g64, tie), uc.grad_bound(e32, g64)
        worst = max(worst, ratio(err, bound))
        lines.append(f"unflow golden {name} level {l}: dflow max error {err:.2e}, bound {bound:.2e} (the reference's float32 run {e32:.1e}), error / bound {ratio(err, bound):.3f}")
    for line in lines:
        report(line)
    note("golden values", name, max(rels) / uc.SCALAR_RTOL)
    note("golden dflow", name, worst)
    assert same(mod.pyramid_occu_mask1[0].cpu(), torch.from_numpy(z[f"mask1_{k}"]).float())
    assert same(mod.pyramid_occu_mask2[0].cpu(), torch.from_numpy(z[f"mask2_{k}"]).float())
    assert max(rels) <= uc.SCALAR_RTOL and worst <= 1.0, "\n".join(lines)


def test_pyramid_cache_survives_an_in_place_edit_of_target():
    name, cfg, (B, H, W), levels = uc.module_cases()[0]
    flows, target, _ = uc.pyramid_inputs(B, H, W, levels, 4100)
    tgt = G(target)
    mod, out, leaves = run_module(cfg, flows, tgt)
    cached = mod._pyramid[2][(H, W)][0]
    _, again, _ = run_module(cfg, flows, tgt, mod)                   # the second call of a step: the same images, not rebuilt
    assert mod._pyramid[2][(H, W)][0] is cached and same(out[0], again[0])
    with torch.no_grad():
        tgt[:, :, : H // 2] *= 0.5                                   # in place: same tensor, new version
    _, edited, l_edit = run_module(cfg, flows, tgt, mod)
    _, fresh, l_fresh = run_module(cfg, flows, tgt.clone())
    assert mod._pyramid[2][(H, W)][0] is not cached
    assert same(edited[0], fresh[0]) and not same(edited[0], out[0])
    assert all(same(a.grad, b.grad) for a, b in zip(l_edit[:-1], l_fresh[:-1]))
    ref = uc.loss_ref(cfg, flows, N(tgt))
    assert uc.rel_err(float(edited[0]), ref["total"]) <= uc.SCALAR_RTOL
    _, other, _ = run_module(cfg, flows, G(target), mod)             # another tensor: rebuilt again
    assert same(other[0], out[0])


def test_module_leaves_flows_without_grad_alone_and_needs_level_0():
    name, cfg, (B, H, W), levels = uc.module_cases()[0]
    flows, target, _ = uc.pyramid_inputs(B, H, W, levels, 4100)
    out = rcf_amd.unFlowLoss(cfg)([G(f) for f in flows], G(target))
    assert not out[0].requires_grad
    with pytest.raises(rcf_amd._lib.RcfHipError):
        rcf_amd.unFlowLoss(uc.fcn_cfg(w_scales=[0.0, 1.0, 1.0, 1.0, 0.0]))([G(f) for f in flows], G(target))
    with pytest.raises(rcf_amd._lib.RcfHipError):
        rcf_amd.unFlowLoss(cfg)([G(f).half() for f in flows], G(target))


# =============================================================================================================== summary
def test_worst_margins_per_group(report):
    """last in the file: what the tests above noted, one line per group (empty when they were deselected)"""
    TH, TW, MD = uc.geometry()
    if WORST:
        report(f"unflow sweep summary: {len(uc.CASES)} photometric cases, tile {TH} x {TW}, md up to {MD}; worst error / bound per group")
    for grp in sorted(WORST):
        report(f"unflow sweep worst {grp}: {WORST[grp][0]:.3f}  ({WORST[grp][1]})")
        assert WORST[grp][0] <= 1.0
