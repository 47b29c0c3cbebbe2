"""The warp, occlusion and photometric kernels (csrc/warp.hip) against the float64 restatement of tests/warp_cases.py (its
conditioning: tests/test_warp_sweep_cpu.py).  Errors are taken PER ELEMENT against 16 u mass (warped pixels, dflow) and
(16 + n) u mass (dx), u = 2^-24; masks must equal the restatement outside its tie set; the fused L1 sum stays within the sum of
its pixels' bounds and its mask sum is exact; the photometric loss keeps the suite's 1e-4.  The tile kernels must give the bits of
the per-pixel kernels.  Outputs start as NaN, dx as zeros (the kernel accumulates into it)."""
from ctypes import c_void_p

import numpy as np
import pytest
import torch

import rcf_amd  # noqa: F401  (package alias)
import rcf_torch as orc
import warp_cases as wc
from rcf_amd import _lib, ops

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
NAN = float("nan")
PP = _lib.WARP_PER_PIXEL
PAD = {"border": 0, "zeros": 1}
ALL = [pytest.param(c, id=c.name) for c in wc.CASES]


def P(t):
    return None if t is None else c_void_p(t.data_ptr())


def G(a):
    return torch.from_numpy(np.ascontiguousarray(a)).to(DEV)


def N(t):
    return t.cpu().numpy()


def same(a, b):
    """bit-equal, NaN == NaN"""
    return a.shape == b.shape and torch.equal(a.contiguous().view(torch.uint8), b.contiguous().view(torch.uint8))


def warp(x, fl, mode):
    B, C, H, W = x.shape
    out = torch.full_like(x, NAN)
    ops.call("rcf_flow_warp_f32", P(x), P(fl), P(out), B, C, H, W, mode, ops._stream())
    return out


def warp_bwd(x, fl, dout, mode, want_dx=True, want_dflow=True):
    B, C, H, W = x.shape
    dx = torch.zeros_like(x) if want_dx else None
    dfl = torch.full_like(fl, NAN) if want_dflow else None
    ops.call("rcf_flow_warp_bwd_f32", P(x), P(fl), P(dout), P(dx), P(dfl), B, C, H, W, mode, ops._stream())
    return dx, dfl


def l1(im1, im2, fl, occ, mode):
    B, C, H, W = im1.shape
    out = torch.full((2,), NAN, dtype=torch.float64, device=DEV)
    ops.call("rcf_warp_l1_residual_f32", P(im1), P(im2), P(fl), P(occ), P(out), B, C, H, W, mode, ops._stream())
    return [float(v) for v in out.cpu()]


def occ_backward(f21, th=0.2):
    B, _, H, W = f21.shape
    occ = torch.full((B, 1, H, W), NAN, device=DEV)
    scratch = torch.full((B, H, W), NAN, device=DEV)
    ops.call("rcf_occu_mask_backward_f32", P(f21), P(occ), th, P(scratch), B, H, W, ops._stream())
    return occ, scratch


def occ_bidir(f12, f21, scale=0.01, bias=0.5):
    B, _, H, W = f12.shape
    occ = torch.full((B, 1, H, W), NAN, device=DEV)
    ops.call("rcf_occu_mask_bidirection_f32", P(f12), P(f21), P(occ), scale, bias, B, H, W, ops._stream())
    return occ


def photometric(im, rec, occ, w1, ws):
    B, C, H, W = im.shape
    out = torch.full((1,), 12345.0, device=DEV)
    scratch = torch.full((4,), NAN, dtype=torch.float64, device=DEV)
    ops.call("rcf_photometric_loss_f32", P(im), P(rec), P(occ), w1, ws, P(out), P(scratch), B, C, H, W, ops._stream())
    return float(out[0])


# =================================================================================================================== warp
@pytest.mark.parametrize("c", ALL)
def test_warp_forward_vs_float64(c, report):
    d = wc.inputs(c)
    x, fl = G(d["x"]), G(d["f12"])
    for pad in c.pads:
        ref, mass = wc.warp_truth(c, pad)
        out = warp(x, fl, PAD[pad])
        m = wc.elem_margin(N(out), ref, wc.warp_bound(mass))
        kern = wc.warp_kernel(c.C, c.H, c.W, pad)
        per_pixel = warp(x, fl, PAD[pad] | PP)
        eq = same(out, per_pixel)
        report(f"warp sweep forward {c.name} {pad}: {kern} kernel, worst error / bound {m:.3f}; bits of the per-pixel form: {eq}")
        assert m <= 1.0, (c.name, pad)
        assert eq, f"{c.name} {pad}: the {kern} kernel differs from the per-pixel kernel on {int((N(out) != N(per_pixel)).sum())} values"


@pytest.mark.parametrize("c", ALL)
def test_fused_l1_vs_float64(c, report):
    d = wc.inputs(c)
    x, y, fl, occ = G(d["x"]), G(d["y"]), G(d["f12"]), G(d["occ"])
    for pad in c.pads:
        kern = wc.l1_kernel(c.C, c.H, c.W, pad)
        for o_np, o_dev, tag in ((d["occ"], occ, "masked"), (None, None, "no mask")):
            s, so, bound = wc.l1_pair_ref(d["y"], d["x"], d["f12"], o_np, pad)
            got = l1(y, x, fl, o_dev, PAD[pad])
            ppx = l1(y, x, fl, o_dev, PAD[pad] | PP)
            m, mp = abs(got[0] - s) / bound, abs(ppx[0] - s) / bound
            rel = abs(got[0] - ppx[0]) / abs(ppx[0])
            report(f"warp sweep fused L1 {c.name} {pad} {tag}: {kern} kernel, error / bound {m:.3f} (per-pixel form {mp:.3f}), "
                   f"relative difference of the two forms {rel:.1e}, mask sum {got[1]} of {so}")
            assert m <= 1.0 and mp <= 1.0, (c.name, pad, tag)
            assert got[1] == so and ppx[1] == so
            assert rel <= 1e-12


@pytest.mark.parametrize("c", ALL)
def test_warp_backward_vs_float64(c, report):
    """dx as a scatter in any order, dflow with torch's clip rule; with dx or dflow null the other output keeps its bits -- for dx on
    every element that receives at most two non-zero terms.  A float32 sum of n >= 3 terms depends on the order in which the
    atomics arrive, which no call fixes (seen on the MI355X: the last bit of such elements differs from run to run): each order
    makes n - 1 additions, each rounding by at most u of a partial sum that stays under mass (1 + n u), so two orders lie within
    2 (n - 1) u mass (1 + n u) of each other, and that is what those elements are held to"""
    d = wc.inputs(c)
    x, fl, dout = G(d["x"]), G(d["f12"]), G(d["dout"])
    for pad in c.pads:
        rdx, dmass, n, rdfl, fmass = wc.bwd_truth(c, pad)
        dx, dfl = warp_bwd(x, fl, dout, PAD[pad])
        m_dx = wc.elem_margin(N(dx), rdx, wc.dx_bound(dmass, n))
        m_df = wc.elem_margin(N(dfl), rdfl, wc.warp_bound(fmass))
        dx_only, none = warp_bwd(x, fl, dout, PAD[pad], want_dflow=False)
        none2, dfl_only = warp_bwd(x, fl, dout, PAD[pad], want_dx=False)
        assert none is None and none2 is None
        few = np.broadcast_to((n <= 2)[:, None], rdx.shape)
        a, b = N(dx), N(dx_only)
        order = wc.elem_margin(a, b, 2 * np.maximum(n - 1, 0)[:, None] * wc.U * dmass * (1 + n[:, None] * wc.U))
        report(f"warp sweep backward {c.name} {pad}: worst error / bound dx {m_dx:.3f} dflow {m_df:.3f}; up to {int(n.max())} terms per element; "
               f"without dx: dflow bit-equal {same(dfl, dfl_only)}; without dflow: dx bit-equal on all {bool((a == b).all())}, "
               f"on the {int(few.sum())} elements of at most two terms {bool((a[few] == b[few]).all())}, order difference / (2 (n - 1) u mass) {order:.3f}")
        assert m_dx <= 1.0 and m_df <= 1.0, (c.name, pad)
        assert same(dfl, dfl_only), "dflow changes when dx is not asked for"
        assert np.array_equal(a[few].view(np.uint32), b[few].view(np.uint32)) and order <= 1.0, "dx changes when dflow is not asked for"
        assert not a[np.broadcast_to((n == 0)[:, None], a.shape)].any(), "an element that receives nothing is not zero"


# ================================================================================================================== masks
@pytest.mark.parametrize("c", [pytest.param(c, id=c.name) for c in wc.MASK_CASES])
def test_occlusion_masks_vs_float64(c, report):
    d = wc.inputs(c)
    m12, f21 = G(d["m12"]), G(d["f21"])
    mb, tb = wc.occ_backward_ref(d["f21"], 0.2)
    mi, ti = wc.occ_bidir_ref(d["m12"], d["f21"], 0.01, 0.5)
    ob, cnt = occ_backward(f21, 0.2)
    oi = occ_bidir(m12, f21, 0.01, 0.5)
    ref_cnt = wc.splat_ref(d["f21"])
    low = ref_cnt <= 1.0                                         # where the clamp to [0, 1] leaves the count for the threshold to see
    e_cnt = float(np.abs(N(cnt).astype(np.float64) - ref_cnt)[low].max())
    bad_b, bad_i = wc.mask_mismatch(N(ob), mb, tb), wc.mask_mismatch(N(oi), mi, ti)
    report(f"warp sweep masks {c.name}: backward mismatches {bad_b} (occluded {mb.mean():.3f}, ties {int(tb.sum())}, splat count error {e_cnt:.1e}), "
           f"bidirectional mismatches {bad_i} (occluded {mi.mean():.3f}, ties {int(ti.sum())})")
    assert set(np.unique(N(ob))) <= {0.0, 1.0} and set(np.unique(N(oi))) <= {0.0, 1.0}
    assert bad_b == 0 and bad_i == 0
    assert e_cnt <= wc.TIE / 4                                    # the tie margin covers the float32 count's own error (counts up to 1) four times


# ============================================================================================================= photometric
@pytest.mark.parametrize("name", [p[0] for p in wc.PHOTO_CASES])
def test_photometric_vs_float64(name, report):
    im, rec, occ, w1, ws = wc.photo_inputs(name)
    ref = wc.photometric_ref(im, rec, occ, w1, ws)
    got = photometric(G(im), G(rec), G(occ), w1, ws)
    if name == "zero_mask":
        report(f"warp sweep photometric {name}: {got} (the restatement: {ref})")
        assert not np.isfinite(got) and not np.isfinite(ref)
        return
    T = torch.from_numpy
    o32 = float(orc.photometric_loss(T(im), T(rec), T(occ), w1, ws))
    e, eo = abs(got - ref), abs(o32 - ref)
    report(f"warp sweep photometric {name}: {got!r} against {ref!r}, relative error {e / abs(ref) if ref else e:.2e} of {wc.PHOTO_RTOL:.0e}; "
           f"the oracle's float32 run errs by {eo:.2e}: ratio {e / eo if eo else float(e > 0):.2f}")
    assert e <= wc.PHOTO_RTOL * abs(ref)


# ============================================================================================ the second grid-stride trips
def test_second_trip_photometric(report):
    B, C, H, W = wc.BIG_PHOTO
    im, rec, occ = wc.big_photo_inputs()
    ref = wc.photometric_ref(im, rec, occ)
    got = photometric(G(im), G(rec), G(occ), 0.15, 0.85)
    report(f"warp sweep photometric second trip {B}x{C}x{H}x{W}: relative error {abs(got - ref) / ref:.2e}")
    assert abs(got - ref) <= wc.PHOTO_RTOL * ref


def test_second_trip_backward_and_masks(report):
    """just over 16384 x 256 pixels, C = 1: the last row belongs to the second trip of the backward, splat, threshold and
    bidirectional loops.  The float64 reference of the whole image takes 12 s on the CPU, so it covers the output pixels of the
    last 48 rows: their dflow and bidirectional decisions, and -- no flow there reaches 24 rows -- every dx element and splat count
    of the last 24 rows in full.  Everything above is the first trip, which the small cases check."""
    B, C, H, W = wc.BIG_PX
    g = torch.Generator().manual_seed(2049)
    x, dout = torch.rand(B, C, H, W, generator=g).numpy(), torch.randn(B, C, H, W, generator=g).numpy()
    fl = wc.big_flow(B, H, W, 2050)
    rows, last = np.arange(H - wc.BIG_PX_TAIL, H), slice(H - wc.BIG_PX_REACH, H)
    assert B * (H - 1) * W == wc.PX_TRIP and np.abs(fl[:, :, H - 2 * wc.BIG_PX_TAIL:]).max() < wc.BIG_PX_REACH - 2
    for pad in ("border", "zeros"):
        rdx, dmass, n, rdfl, fmass = wc.warp_bwd_ref(x, fl, dout, pad, rows=rows)
        dx, dfl = warp_bwd(G(x), G(fl), G(dout), PAD[pad])
        dx, dfl = N(dx), N(dfl)
        m_dx = wc.elem_margin(dx[:, :, last], rdx[:, :, last], wc.dx_bound(dmass, n)[:, :, last])
        m_df = wc.elem_margin(dfl[:, :, rows], rdfl, wc.warp_bound(fmass))
        m_row = wc.elem_margin(dfl[:, :, -1], rdfl[:, :, -1], wc.warp_bound(fmass)[:, :, -1])
        report(f"warp sweep backward second trip {B}x{C}x{H}x{W} {pad}: worst error / bound dx {m_dx:.3f} dflow {m_df:.3f} (last row {m_row:.3f})")
        assert m_dx <= 1.0 and m_df <= 1.0
        assert np.isfinite(dx).all() and np.isfinite(dfl).all()
        assert np.abs(rdfl[:, :, -1]).max() > 0.1 and np.abs(rdx[:, :, -1]).max() > 0.1           # the last row has something to get wrong
    # masks: the splat of the white flow; the bidirectional check on a smooth flow and its noisy inverse (see warp_cases.inputs)
    m12 = wc.smooth_flow(B, H, W, g, amp_y=0.4)
    f21 = (-m12 + 0.7 * torch.randn(B, 2, H, W, generator=g).numpy()).astype(np.float32)
    mb, tb = wc.occ_backward_ref(fl, 0.2, rows=rows)
    mi, ti = wc.occ_bidir_ref(m12, f21, 0.01, 0.5, rows=rows)
    ob, _ = occ_backward(G(fl), 0.2)
    oi = occ_bidir(G(m12), G(f21), 0.01, 0.5)
    ob, oi = N(ob), N(oi)
    bad_b, bad_i = wc.mask_mismatch(ob[:, :, last], mb[:, :, last], tb[:, :, last]), wc.mask_mismatch(oi[:, :, rows], mi, ti)
    sb, si = mb[:, :, last].mean(), mi.mean()
    report(f"warp sweep masks second trip {B}x{H}x{W}: backward mismatches {bad_b} (occluded {sb:.3f}, ties {tb[:, :, last].mean():.1e}), "
           f"bidirectional mismatches {bad_i} (occluded {si:.3f}, ties {ti.mean():.1e}); last row occluded {mb[:, :, -1].mean():.3f} / {mi[:, :, -1].mean():.3f}")
    assert bad_b == 0 and bad_i == 0 and tb[:, :, last].mean() <= 0.005 and ti.mean() <= 0.005
    assert 0.1 <= sb <= 0.9 and 0.1 <= si <= 0.9 and 0.1 <= mb[:, :, -1].mean() <= 0.9 and 0.1 <= mi[:, :, -1].mean() <= 0.9
    assert set(np.unique(ob)) <= {0.0, 1.0} and set(np.unique(oi)) <= {0.0, 1.0}                  # every pixel written


def test_second_trip_tile_forward(report):
    """8195 tiles: the 1024 workgroups of an XCD walk 1025 of them.  Equal bits with the per-pixel form everywhere, and against
    float64 on every 64th row and the last one"""
    B, C, H, W = wc.BIG_TILE
    g = torch.Generator().manual_seed(26209)
    x = torch.rand(B, C, H, W, generator=g)
    fl = torch.randn(B, 2, H, W, generator=g) * 2.5
    xg, fg = x.to(DEV), fl.to(DEV)
    out, ppx = warp(xg, fg, 0), warp(xg, fg, PP)
    rows = np.unique(np.concatenate([np.arange(0, H, 64), [H - 1]]))
    ref, mass = wc.warp_ref(x.numpy(), fl.numpy(), "border", rows=rows)
    m = wc.elem_margin(N(out)[:, :, rows], ref, wc.warp_bound(mass))
    eq = same(out, ppx)
    report(f"warp sweep forward second trip {B}x{C}x{H}x{W}: bits of the per-pixel form {eq}; {len(rows)} rows against float64, worst error / bound {m:.3f}")
    assert eq and m <= 1.0


def test_second_trip_fused_l1_per_pixel_kernel(report):
    """300 images of 2 x 2: B * runs = 300 > 256 workgroups per band"""
    B, H, W = wc.L1_MANY
    g = torch.Generator().manual_seed(300)
    for C, pad in ((2, "border"), (3, "zeros")):
        x, y = torch.rand(B, C, H, W, generator=g).numpy(), torch.rand(B, C, H, W, generator=g).numpy()
        fl = (torch.randn(B, 2, H, W, generator=g) * 0.7).numpy()
        occ = (torch.rand(B, 1, H, W, generator=g) > 0.3).float().numpy()
        assert wc.l1_kernel(C, H, W, pad) == "pixel"
        s, so, bound = wc.l1_pair_ref(y, x, fl, occ, pad)
        got = l1(G(y), G(x), G(fl), G(occ), PAD[pad])
        report(f"warp sweep fused L1 second trip {B}x{C}x{H}x{W} {pad}: error / bound {abs(got[0] - s) / bound:.3f}, mask sum {got[1]} of {so}")
        assert abs(got[0] - s) <= bound and got[1] == so


# ================================================================================================================ refusals
def test_warp_entries_refuse_what_they_cannot_do():
    g = torch.Generator().manual_seed(3)
    t = lambda *s: torch.randn(*s, generator=g).to(DEV)
    outs = []

    def out(*shape, dtype=torch.float32):
        o = torch.full(shape, 7.0, dtype=dtype, device=DEV)
        outs.append(o)
        return o
    st = ops._stream()

    def refused(name, *args):
        with pytest.raises(_lib.RcfHipError, match="status -1"):
            ops.call(name, *args)
    x, fl, o, o2, d2 = t(1, 3, 8, 8), t(1, 2, 8, 8), out(1, 3, 8, 8), out(1, 2, 8, 8), out(4, dtype=torch.float64)
    for H, W in ((1, 64), (64, 1)):
        refused("rcf_flow_warp_f32", P(x), P(fl), P(o), 1, 3, H, W, 0, st)
        refused("rcf_flow_warp_bwd_f32", P(x), P(fl), P(x), P(o), P(o2), 1, 3, H, W, 0, st)
        refused("rcf_warp_l1_residual_f32", P(x), P(x), P(fl), None, P(d2), 1, 3, H, W, 0, st)
        refused("rcf_occu_mask_backward_f32", P(fl), P(o), 0.2, P(o2), 1, H, W, st)
        refused("rcf_occu_mask_bidirection_f32", P(fl), P(fl), P(o), 0.01, 0.5, 1, H, W, st)
    for H, W in ((2, 32), (32, 2)):
        refused("rcf_photometric_loss_f32", P(x), P(x), P(fl), 0.15, 0.85, P(o), P(d2), 1, 3, H, W, st)
    for pad in (2, 2 | PP, -1):
        refused("rcf_flow_warp_f32", P(x), P(fl), P(o), 1, 3, 8, 8, pad, st)
        refused("rcf_flow_warp_bwd_f32", P(x), P(fl), P(x), P(o), P(o2), 1, 3, 8, 8, pad, st)
        refused("rcf_warp_l1_residual_f32", P(x), P(x), P(fl), None, P(d2), 1, 3, 8, 8, pad, st)
    refused("rcf_flow_warp_f32", None, P(fl), P(o), 1, 3, 8, 8, 0, st)
    refused("rcf_flow_warp_f32", P(x), None, P(o), 1, 3, 8, 8, 0, st)
    refused("rcf_flow_warp_f32", P(x), P(fl), None, 1, 3, 8, 8, 0, st)
    refused("rcf_flow_warp_bwd_f32", None, P(fl), P(x), P(o), P(o2), 1, 3, 8, 8, 0, st)
    refused("rcf_flow_warp_bwd_f32", P(x), None, P(x), P(o), P(o2), 1, 3, 8, 8, 0, st)
    refused("rcf_flow_warp_bwd_f32", P(x), P(fl), None, P(o), P(o2), 1, 3, 8, 8, 0, st)
    refused("rcf_warp_l1_residual_f32", None, P(x), P(fl), None, P(d2), 1, 3, 8, 8, 0, st)
    refused("rcf_warp_l1_residual_f32", P(x), None, P(fl), None, P(d2), 1, 3, 8, 8, 0, st)
    refused("rcf_warp_l1_residual_f32", P(x), P(x), None, None, P(d2), 1, 3, 8, 8, 0, st)
    refused("rcf_warp_l1_residual_f32", P(x), P(x), P(fl), None, None, 1, 3, 8, 8, 0, st)
    refused("rcf_occu_mask_backward_f32", None, P(o), 0.2, P(o2), 1, 8, 8, st)
    refused("rcf_occu_mask_backward_f32", P(fl), None, 0.2, P(o2), 1, 8, 8, st)
    refused("rcf_occu_mask_backward_f32", P(fl), P(o), 0.2, None, 1, 8, 8, st)
    refused("rcf_occu_mask_bidirection_f32", None, P(fl), P(o), 0.01, 0.5, 1, 8, 8, st)
    refused("rcf_occu_mask_bidirection_f32", P(fl), None, P(o), 0.01, 0.5, 1, 8, 8, st)
    refused("rcf_occu_mask_bidirection_f32", P(fl), P(fl), None, 0.01, 0.5, 1, 8, 8, st)
    for k in range(5):
        a = [P(x), P(x), P(fl), P(o), P(d2)]
        a[k] = None
        refused("rcf_photometric_loss_f32", a[0], a[1], a[2], 0.15, 0.85, a[3], a[4], 1, 3, 8, 8, st)
    refused("rcf_flow_warp_f32", P(x), P(fl), P(o), 1, 3, 32768, 32768, 0, st)
    refused("rcf_warp_l1_residual_f32", P(x), P(x), P(fl), None, P(d2), 1, 3, 32768, 32768, 0, st)
    torch.cuda.synchronize()
    assert all(bool((v == 7.0).all()) for v in outs), "a refused call wrote to an output"
