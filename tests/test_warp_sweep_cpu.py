"""Conditioning of the warp sweep (tests/warp_cases.py): the restatement agrees with oracle/rcf_torch.py in float64; the oracle's
own float32 run sits inside every per-element bound the GPU test applies (so a kernel that misses one is wrong, not unlucky); the
tile kernels' 3-operation division equals float32's t / d at every image size up to 4096; the tables reach the dispatch and
geometry branches they name; the random inputs leave both occlusion masks mixed and almost free of threshold ties; and the entries
refuse what they cannot do before they touch a device.

torch's CPU grid_sample is undefined on inf / NaN positions in zeros mode (it converts them to indices unchecked: a segmentation
fault has been seen, and NaN pixels): the oracle therefore only ever sees finite flows here, and the non-finite kinds (border
mode only) are defined by the restatement alone, checked below against what it promises."""
import ctypes

import numpy as np
import pytest
import torch

import rcf_torch as orc
import warp_cases as wc

FINITE = [pytest.param(c, id=c.name) for c in wc.CASES if c.flow in wc.FINITE_FLOWS]
T = torch.from_numpy


def oracle_bwd(d, pad, dtype):
    x, fl = T(d["x"]).to(dtype).requires_grad_(True), T(d["f12"]).to(dtype).requires_grad_(True)
    out = orc.flow_warp(x, fl, pad=pad)
    out.backward(T(d["dout"]).to(dtype))
    return out.detach().numpy(), x.grad.numpy(), fl.grad.numpy()


# ------------------------------------------------------------------------------------------------ restatement vs the oracle
@pytest.mark.parametrize("c", FINITE)
def test_restatement_vs_oracle_float64(c):
    d = wc.inputs(c)
    for pad in c.pads:
        ref, mass = wc.warp_ref(d["x"], d["f12"], pad, np.float64)
        dx, dmass, n, dfl, fmass = wc.warp_bwd_ref(d["x"], d["f12"], d["dout"], pad, np.float64)
        o_out, o_dx, o_dfl = oracle_bwd(d, pad, torch.float64)
        e = (wc.elem_margin(ref, o_out, 1e-12 * mass), wc.elem_margin(dx, o_dx, 1e-12 * dmass), wc.elem_margin(dfl, o_dfl, 1e-12 * fmass))
        print(f"warp sweep {c.name} {pad}: restatement vs oracle float64, error / (1e-12 mass): warp {e[0]:.3f} dx {e[1]:.3f} dflow {e[2]:.3f}")
        assert max(e) <= 1.0
        assert bool(((n != 0)[:, None] >= (dmass != 0)).all())                # the mass vanishes where no term arrives
        s, so, bound = wc.l1_pair_ref(d["y"], d["x"], d["f12"], d["occ"], pad, np.float64)
        o_s = float(((T(d["y"]).double() - T(o_out)).abs().sum(1, keepdim=True) * T(d["occ"]).double()).sum())
        assert abs(s - o_s) <= 1e-12 * abs(o_s) and so == float(d["occ"].sum()) and 0 < bound < 1e-4 * s


@pytest.mark.parametrize("c", [pytest.param(c, id=c.name) for c in wc.MASK_CASES])
def test_mask_restatement_vs_oracle(c):
    """float64 against float64 (positions too), then the oracle's float32 masks against the float32-position restatement: equal
    outside the tie set, which stays under 0.5 % of the pixels"""
    d = wc.inputs(c)
    f12, f21 = T(d["m12"]), T(d["f21"])
    B, _, H, W = f21.shape
    xs = torch.arange(W).double().view(1, 1, W).expand(B, H, W)
    ys = torch.arange(H).double().view(1, H, 1).expand(B, H, W)
    cnt = wc.splat_ref(d["f21"], np.float64)
    o_cnt = orc.corresponding_map(torch.stack([xs, ys], 1) + f21.double())[:, 0].numpy()
    assert wc.elem_margin(cnt, o_cnt, 1e-12 * np.maximum(cnt, 1e-300)) <= 1.0
    for pdt, tdt in ((np.float64, torch.float64), (np.float32, torch.float32)):
        mb, tb = wc.occ_backward_ref(d["f21"], 0.2, pdt)
        mi, ti = wc.occ_bidir_ref(d["m12"], d["f21"], 0.01, 0.5, pdt)
        ob = orc.occu_mask_backward(f21.to(tdt), 0.2).numpy()
        oi = orc.occu_mask_bidirection(f12.to(tdt), f21.to(tdt)).numpy()
        assert wc.mask_mismatch(ob, mb, tb) == 0 and wc.mask_mismatch(oi, mi, ti) == 0, (c.name, pdt)
        assert tb.mean() <= 0.005 and ti.mean() <= 0.005, (c.name, tb.mean(), ti.mean())
        if c.flow == "gauss" and c.H * c.W >= 100 and pdt == np.float32:
            print(f"warp sweep {c.name}: occluded share backward {mb.mean():.3f} bidirectional {mi.mean():.3f}, ties {tb.mean():.1e} {ti.mean():.1e}")
            assert 0.1 <= mb.mean() <= 0.9 and 0.1 <= mi.mean() <= 0.9


@pytest.mark.parametrize("c", FINITE)
def test_oracle_float32_run_is_inside_the_bounds(c):
    d = wc.inputs(c)
    for pad in c.pads:
        ref, mass = wc.warp_truth(c, pad)
        dx, dmass, n, dfl, fmass = wc.bwd_truth(c, pad)
        o_out, o_dx, o_dfl = oracle_bwd(d, pad, torch.float32)
        e = (wc.elem_margin(o_out, ref, wc.warp_bound(mass)), wc.elem_margin(o_dx, dx, wc.dx_bound(dmass, n)),
             wc.elem_margin(o_dfl, dfl, wc.warp_bound(fmass)))
        print(f"warp sweep {c.name} {pad}: oracle float32 error / bound: warp {e[0]:.3f} dx {e[1]:.3f} dflow {e[2]:.3f}; n up to {int(n.max())}")
        assert max(e) <= 1.0
        s, so, bound = wc.l1_pair_ref(d["y"], d["x"], d["f12"], d["occ"], pad)
        o_s = float(((T(d["y"]) - T(o_out)).abs().sum(1, keepdim=True) * T(d["occ"])).double().sum())
        assert abs(o_s - s) <= bound


# ------------------------------------------------------------------------------------------------------- non-finite flows
@pytest.mark.parametrize("c", [pytest.param(c, id=c.name) for c in wc.CASES if c.flow in wc.BORDER_ONLY_FLOWS])
def test_non_finite_flows_follow_the_stated_clip(c):
    """border mode: +inf and an overflowing 2 p sample column / row size - 1, -inf and NaN sample 0, a flow of 1e-40 is no flow;
    the gradient of a clipped coordinate is 0; nothing non-finite comes out"""
    d = wc.inputs(c)
    fl, x = d["f12"], d["x"].astype(np.float64)
    assert c.pads == ("border",)
    ref, mass = wc.warp_truth(c, "border")
    dx, dmass, n, dfl, fmass = wc.bwd_truth(c, "border")
    assert np.isfinite(ref).all() and np.isfinite(dx).all() and np.isfinite(dfl).all()
    B, C, H, W = x.shape
    hi = {"nan": 0, "inf": 1, "huge": 1}.get(c.flow)
    fx, fy = fl[:, 0], fl[:, 1]
    bad = lambda f: ~np.isfinite(f) | (np.abs(f) > 1e38)
    if hi is not None:
        both = bad(fx) & bad(fy)
        assert both.sum() > 10 and (bad(fx) & ~bad(fy)).sum() > 10 and (~bad(fx) & bad(fy)).sum() > 10
        col = np.where(np.isnan(fx) | (fx < 0), 0, W - 1)
        row = np.where(np.isnan(fy) | (fy < 0), 0, H - 1)
        for b in range(B):
            yy, xx = np.nonzero(both[b])
            assert np.array_equal(ref[b][:, yy, xx], x[b][:, row[b, yy, xx], col[b, yy, xx]])
        assert not dfl[:, 0][bad(fx)].any() and not dfl[:, 1][bad(fy)].any()
        assert {int(v) for v in np.unique(col[bad(fx)])} == ({0} if c.flow == "nan" else {0, W - 1})
    else:
        zero = fl.copy()
        zero[np.abs(fl) < 1e-30] = 0
        assert (zero != fl).sum() > 10
        r0, _ = wc.warp_ref(d["x"], zero, "border")
        assert np.array_equal(r0, ref)


# ------------------------------------------------------------------------------------------------------------- photometric
@pytest.mark.parametrize("name", [p[0] for p in wc.PHOTO_CASES])
def test_photometric_restatement_vs_oracle(name):
    im, rec, occ, w1, ws = wc.photo_inputs(name)
    ref = wc.photometric_ref(im, rec, occ, w1, ws)
    with np.errstate(all="ignore"):
        o64 = float(orc.photometric_loss(T(im).double(), T(rec).double(), T(occ).double(), w1, ws))
        o32 = float(orc.photometric_loss(T(im), T(rec), T(occ), w1, ws))
    print(f"warp sweep photometric {name}: restatement {ref!r} oracle float64 {o64!r} float32 {o32!r}")
    if name == "zero_mask":
        assert not np.isfinite(ref) and not np.isfinite(o64) and not np.isfinite(o32)
        return
    assert abs(ref - o64) <= 1e-12 * abs(o64) and abs(o32 - ref) <= wc.PHOTO_RTOL * abs(ref)
    if name == "same":
        assert ref == 0.0
    else:
        assert ref > 1e-3
    if name == "patches":
        assert (occ[:, :, 2:7, 3:9] == 0).all()
    assert occ.shape[2] * occ.shape[3] > 9 or name == "one_interior"


def test_big_photometric_restatement_vs_oracle():
    B, C, H, W = wc.BIG_PHOTO
    assert wc.PHOTO_TRIP < B * H * W < 1.01 * wc.PHOTO_TRIP
    im, rec, occ = wc.big_photo_inputs()
    ref = wc.photometric_ref(im, rec, occ)
    o64 = float(orc.photometric_loss(T(im).double(), T(rec).double(), T(occ).double()))
    assert abs(ref - o64) <= 1e-12 * abs(o64)


# ----------------------------------------------------------------------------------------------------------- the division
def test_three_operation_division_is_correctly_rounded():
    """q = t r; q += fma(-q, d, t) r against float32's t / d, t = 2 p: every integer and every half position from -3 to d + 3 and
    3000 random ones, for every d = size - 1 from 1 to 4095"""
    rng = np.random.default_rng(5)
    total = 0
    for d in range(1, 4096):
        grid = np.arange(-6, 2 * (d + 3) + 1, dtype=np.float32) * np.float32(0.5)                      # integers and halves
        rnd = rng.uniform(-3.0, d + 3.0, 3000).astype(np.float32)
        t = np.float32(2) * np.concatenate([grid, rnd])
        want = t / np.float32(d)
        got = wc.div3(t, d)
        assert want.dtype == got.dtype == np.float32
        bad = got.view(np.uint32) != want.view(np.uint32)
        assert not bad.any(), (d, t[bad][:4], got[bad][:4], want[bad][:4])
        total += t.size
    assert total > 25e6
    # the helper's fma rounds once: cases where rounding the float64 sum first would round twice
    a, b = np.float32(1 + 2.0 ** -23), np.float32(1 + 2.0 ** -23)                                      # a b = 1 + 2^-22 + 2^-46
    assert wc.fma32(a, b, np.float32(2.0 ** -24)) == np.float32(1 + 2.0 ** -22 + 2.0 ** -23)           # just above the tie: up
    assert np.float32(np.float64(a) * np.float64(b) + 2.0 ** -24 - 2.0 ** -46) == np.float32(1 + 2.0 ** -22)


# -------------------------------------------------------------------------------------------------------- branch coverage
def test_tables_reach_every_branch():
    cases = {(c.H, c.W, c.C, c.B) for c in wc.CASES}
    shapes = {(c.H, c.W) for c in wc.CASES if c.C == 3}
    assert shapes >= set(wc.SHAPES_MIN + wc.SHAPES_SEAMS + wc.SHAPES_TILE + wc.SHAPES_L1 + wc.FLOW_SHAPES)
    assert {c.C for c in wc.CASES if (c.H, c.W) == (9, 70)} == {1, 2, 3, 4}
    for H, W in wc.FLOW_SHAPES:
        assert {c.flow for c in wc.CASES if (c.H, c.W, c.C) == (H, W, 3)} == set(wc.FINITE_FLOWS + wc.BORDER_ONLY_FLOWS)
    pp = {s: wc.pixel_plan(2, *s) for s in shapes}
    # the per-pixel kernels' bands (every shape runs them: zeros mode, and border mode through the per-pixel switch)
    assert any(H < 8 and 0 in p["rows"] for (H, W), p in pp.items())                                   # an empty band, H < 8
    assert pp[9, 70]["rows"] == [2, 2, 2, 2, 1, 0, 0, 0]                                               # a one-row last band
    assert max(pp[9, 70]["band_px"]) <= 256 and max(pp[2, 2]["band_px"]) <= 256                        # no paired pixel
    assert pp[17, 200]["runs"] == 2 and 0 < pp[17, 200]["band_px"][0] - 512 < 256                      # a second run under 256 pixels
    assert pp[33, 300]["runs"] == 3 and 256 < pp[33, 300]["band_px"][0] - 1024 < 512                   # RGB pairs and the generic loop together
    assert 0 < pp[17, 257]["band_px"][0] - 512 - 256 < 64                                              # ... three paired pixels only
    # dispatch
    assert {wc.warp_kernel(3, H, W, "border") for H, W in wc.SHAPES_TILE} == {"rows"}
    assert {wc.warp_kernel(3, H, W, "border") for H, W in wc.SHAPES_SEAMS + wc.SHAPES_L1 + wc.SHAPES_MIN} == {"pixel"}
    assert wc.warp_kernel(3, 17, 257, "zeros") == "pixel" and wc.warp_kernel(4, 17, 257, "border") == "pixel"
    l1 = {s: wc.l1_kernel(3, *s, "border") for s in shapes}
    assert {l1[s] for s in wc.SHAPES_L1} == {"rows", "rows2"} and l1[2, 2] == "rows2" and l1[2, 3] == "rows" and l1[3, 2] == "rows2"
    assert all(wc.l1_kernel(C, 9, 70, "border") == "pixel" for C in (1, 2, 4)) and wc.l1_kernel(3, 9, 70, "zeros") == "pixel"
    # flow_warp's tile kernel: empty XCD shares, one-lane and one-row tails, the second trip
    p = wc.warp_tile_plan(1, 16, 256)
    assert (16, 256, 3, 1) in cases and p["tx"] * p["ty"] == 4 and p["per"].count(0) == 4 and p["trips"] == 1
    rgb = [c for c in wc.CASES if c.C == 3]
    tails = {(c.W % 64, c.H % 16) for c in rgb if wc.warp_kernel(3, c.H, c.W, "border") == "rows"}
    assert (1, 1) in tails and (0, 0) in tails and wc.warp_tile_plan(2, 17, 257)["tx"] == 5            # a one-lane x tail with a one-row y tail; none
    B, C, H, W = wc.BIG_TILE
    p = wc.warp_tile_plan(B, H, W)
    assert C == 3 and p["Q"] == 1024 and p["trips"] == 2 and wc.warp_tile_plan(B, H - 16, W)["trips"] == 1 and H * W < 2 ** 30
    assert W % 64 == 1 and H % 16 == 1
    # the fused L1 tile kernels: a second r += Q trip in both, tails
    for s, kern in (((9, 130), "rows2"), ((8, 128), "rows2"), ((3, 2), "rows2"), ((17, 65), "rows"), ((17, 257), "rows"), ((33, 300), "rows2")):
        assert l1[s] == kern and wc.l1_tile_plan(2, *s)["trips"] >= 2, s
    assert wc.l1_tile_plan(2, 33, 300)["Q"] == 1 and wc.l1_tile_plan(2, 17, 257)["per"].count(0) == 0
    assert 0 in wc.l1_tile_plan(2, 9, 130)["per"]                                                      # an XCD share per == 0
    tails2 = {(c.W % 128, c.H % 8) for c in rgb if wc.l1_kernel(3, c.H, c.W, "border") == "rows2"}
    tails1 = {(c.W % 64, c.H % 16) for c in rgb if wc.l1_kernel(3, c.H, c.W, "border") == "rows"}
    assert (2, 1) in tails2 and (0, 0) in tails2 and (1, 1) in tails1                                  # one lane (one pixel pair) and one row left over
    # warp_l1_kernel: its second trip needs B * runs > 256
    Bm, Hm, Wm = wc.L1_MANY
    p = wc.pixel_plan(Bm, Hm, Wm)
    assert p["Q"] == 256 and p["trips"] == 2 and Bm * Hm * Wm < 5000
    # the grid-stride loops
    B, C, H, W = wc.BIG_PX
    assert C == 1 and wc.px_blocks(B * H * W) == 16384 and B * H * W > wc.PX_TRIP and B * (H - 1) * W <= wc.PX_TRIP


# ---------------------------------------------------------------------------------------------------------------- refusals
def test_warp_entries_refuse_before_touching_a_device():
    """H or W of 1 (photometric: of 2), a pad mode that does not exist, null operands, an image of 2^30 pixels: RCF_EINVAL, and
    nothing is launched -- there is no device here, and the host buffers keep their fill"""
    from rcf_amd import _lib
    lib = _lib.load()
    buf = (ctypes.c_float * 64)(*([7.0] * 64))
    p = ctypes.cast(buf, ctypes.c_void_p)
    PP = _lib.WARP_PER_PIXEL
    for dims in ((1, 3, 1, 8), (1, 3, 8, 1), (0, 3, 4, 4), (1, 0, 4, 4), (1, 3, 32768, 32768)):
        for pad in (0, 1, PP):
            assert lib.rcf_flow_warp_f32(p, p, p, *dims, pad, None) == -1
            assert lib.rcf_warp_l1_residual_f32(p, p, p, p, p, *dims, pad, None) == -1
    for pad in (2, 3, -1, 2 | PP):
        assert lib.rcf_flow_warp_f32(p, p, p, 1, 3, 4, 4, pad, None) == -1
        assert lib.rcf_warp_l1_residual_f32(p, p, p, p, p, 1, 3, 4, 4, pad, None) == -1
        assert lib.rcf_flow_warp_bwd_f32(p, p, p, p, p, 1, 3, 4, 4, pad, None) == -1
    for k in range(3):
        a = [p, p, p]
        a[k] = None
        assert lib.rcf_flow_warp_f32(*a, 1, 3, 4, 4, 0, None) == -1
        assert lib.rcf_flow_warp_bwd_f32(*a, p, p, 1, 3, 4, 4, 0, None) == -1
        assert lib.rcf_warp_l1_residual_f32(*a, p, p, 1, 3, 4, 4, 0, None) == -1
    assert lib.rcf_warp_l1_residual_f32(p, p, p, p, None, 1, 3, 4, 4, 0, None) == -1
    for dims in ((1, 3, 1, 8), (1, 3, 8, 1), (0, 3, 4, 4), (1, 0, 4, 4)):
        assert lib.rcf_flow_warp_bwd_f32(p, p, p, p, p, *dims, 0, None) == -1
    for dims in ((1, 1, 8), (1, 8, 1), (0, 4, 4)):
        assert lib.rcf_occu_mask_backward_f32(p, p, 0.2, p, *dims, None) == -1
        assert lib.rcf_occu_mask_bidirection_f32(p, p, p, 0.01, 0.5, *dims, None) == -1
    assert lib.rcf_occu_mask_backward_f32(None, p, 0.2, p, 1, 4, 4, None) == -1
    assert lib.rcf_occu_mask_backward_f32(p, None, 0.2, p, 1, 4, 4, None) == -1
    assert lib.rcf_occu_mask_backward_f32(p, p, 0.2, None, 1, 4, 4, None) == -1
    for k in range(3):
        a = [p, p, p]
        a[k] = None
        assert lib.rcf_occu_mask_bidirection_f32(*a, 0.01, 0.5, 1, 4, 4, None) == -1
    for dims in ((1, 3, 2, 8), (1, 3, 8, 2), (0, 3, 4, 4), (1, 0, 4, 4)):
        assert lib.rcf_photometric_loss_f32(p, p, p, 0.15, 0.85, p, p, *dims, None) == -1
    for k in range(5):
        a = [p] * 5
        a[k] = None
        assert lib.rcf_photometric_loss_f32(a[0], a[1], a[2], 0.15, 0.85, a[3], a[4], 1, 3, 4, 4, None) == -1
    assert list(buf) == [7.0] * 64
