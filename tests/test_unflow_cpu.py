"""Conditioning of the flow-loss sweep (tests/unflow_cases.py) and the host side of rcf_amd.unFlowLoss, without a GPU: the float64
restatement reproduces the reference-made fixture (tests/golden/unflow.npz) to 1e-12 and its masks exactly; its analytic
gradients -- the form the kernels implement -- equal torch autograd of its own forward; the area windows and the nearest rule are
torch's; the case table reaches the branches it names, judged by the kernel's own geometry query; the tie set stays under its cap;
the entry points refuse bad arguments before they touch a device; the module refuses what it does not build."""
import ctypes
import os

import numpy as np
import pytest
import torch
import torch.nn.functional as F

import unflow_cases as uc
import warp_cases as wc
import rcf_amd
from rcf_amd import _lib

T = torch.from_numpy


@pytest.fixture(scope="module")
def golden(golden_dir):
    return np.load(os.path.join(golden_dir, "unflow.npz"))


def golden_inputs(z, levels):
    return [z[f"flow_{l}"] for l in range(levels)], z["target"]


# ----------------------------------------------------------------------------------------------------- against the reference
def test_fixture_is_small_and_holds_the_cases(golden, golden_dir):
    assert os.path.getsize(os.path.join(golden_dir, "unflow.npz")) < 200 * 1024
    B, H, W = uc.GOLDEN_SHAPE
    assert [str(n) for n in golden["names"]] == [n for n, _, _ in uc.golden_cfgs()]
    assert golden["target"].shape == (B, 6, H, W) and golden["target"].dtype == np.float32
    assert 0 <= golden["target"].min() and golden["target"].max() <= 1
    for l in range(uc.GOLDEN_LEVELS):
        assert golden[f"flow_{l}"].shape == (B, 4, H >> l, W >> l) and golden[f"flow_{l}"].dtype == np.float32
    for k, (_, cfg, levels) in enumerate(uc.golden_cfgs()):
        assert golden[f"vals64_{k}"].shape == (4,) and golden[f"vals64_{k}"].dtype == np.float64
        assert golden[f"mask1_{k}"].shape == (B, 1, H, W)
        for l in range(levels):
            assert (f"g64_{k}_{l}" in golden.files) == (cfg.w_scales[l] != 0)


@pytest.mark.parametrize("k", range(len(uc.golden_cfgs())))
def test_restatement_equals_the_reference(golden, k):
    name, cfg, levels = uc.golden_cfgs()[k]
    flows, target = golden_inputs(golden, levels)
    r = uc.loss_ref(cfg, flows, target, pdt=np.float64)
    got = np.asarray([r["total"], r["warp"], r["smooth"], r["absmean"]])
    rel = np.abs(got - golden[f"vals64_{k}"]) / np.maximum(np.abs(golden[f"vals64_{k}"]), 1e-300)
    rel = np.where(golden[f"vals64_{k}"] == 0, np.abs(got), rel)
    print(f"unflow golden {name}: restatement vs the reference's float64 run, relative difference {rel}")
    assert rel.max() <= 1e-12
    assert np.array_equal(r["mask1"], golden[f"mask1_{k}"]) and np.array_equal(r["mask2"], golden[f"mask2_{k}"])
    assert 0.05 < r["mask1"].mean() < 1 and 0.05 < r["mask2"].mean() < 1
    for l in range(levels):
        if cfg.w_scales[l] == 0:
            assert r["grads"][l] is None
            continue
        want = golden[f"g64_{k}_{l}"]
        g = r["grads"][l].reshape(-1)[::uc.GOLDEN_STRIDE]
        e = float(np.abs(g - want).max())
        print(f"unflow golden {name} level {l}: gradient max abs difference {e:.1e} of {np.abs(want).max():.1e}")
        assert np.abs(want).max() > 1e-6 and e <= 1e-12 * np.abs(want).max()
    # the float32 positions of the kernels choose the same taps: the flows sit on odd multiples of 1 / 64
    r32 = uc.loss_ref(cfg, flows, target, pdt=np.float32)
    assert abs(r32["total"] - r["total"]) <= 1e-5 * abs(r["total"])
    assert np.array_equal(r32["mask1"], r["mask1"]) and np.array_equal(r32["mask2"], r["mask2"])


@pytest.mark.parametrize("k", [0, 2, 3])
def test_module_restatement_analytic_equals_autograd(golden, k):
    name, cfg, levels = uc.golden_cfgs()[k]
    flows, target = golden_inputs(golden, levels)
    a = uc.loss_ref(cfg, flows, target)
    b = uc.loss_ref(cfg, flows, target, analytic=False)
    assert abs(a["total"] - b["total"]) <= 1e-13 * abs(a["total"])
    for ga, gb, tie in zip(a["grads"], b["grads"], a["ties"]):
        if ga is not None:
            assert uc.max_err(gb, ga, tie) <= 1e-12 * np.abs(ga).max()
            assert tie.mean() <= uc.MAX_TIE_SHARE


# ------------------------------------------------------------------------------------------------- gradients of the restatement
@pytest.mark.parametrize("c", [pytest.param(c, id=c.name) for c in uc.CASES])
def test_analytic_gradient_equals_autograd_and_ties_stay_rare(c):
    d = uc.inputs(c)
    p, e32, loss32 = uc.photo_truth(c)
    taps = wc.make_taps(d["flow"], "border")
    occ = uc.nearest_mask(d["occ"], c.h, c.w)
    with np.errstate(all="ignore"):
        l64, g64 = uc.photo_autograd(T(d["im"]).double(), T(d["other"]).double(), taps, T(occ).double(), c.md, *c.weights)
    assert uc.rel_err(l64, p.loss) <= 1e-14 and uc.rel_err(loss32, p.loss) <= uc.SCALAR_RTOL
    if c.mask == "zeros":
        assert np.isnan(p.loss) and p.occ_mean == 0
    if not c.grad:
        return
    err = uc.max_err(g64, p.dflow, p.tie[:, None])
    print(f"unflow {c.name}: analytic vs autograd {err:.1e}, float32 CPU run {e32:.1e}, max |g| {np.abs(p.dflow).max():.1e}, tie share {p.tie.mean():.4f}")
    assert np.isfinite(p.dflow).all() and np.abs(p.dflow).max() > 1e-6
    assert err <= 1e-12 * np.abs(p.dflow).max()
    assert p.tie.mean() <= uc.MAX_TIE_SHARE
    assert np.isfinite(e32)


@pytest.mark.parametrize("h,w,second", uc.SMOOTH_CASES)
def test_smoothness_gradient_equals_autograd(h, w, second):
    im, fl = uc.smooth_inputs(h, w, second)
    s = float(min(h, w))
    loss, g, tie = uc.smooth_analytic(T(fl).double(), T(im).double(), 10.0, s, second)
    l2, g2 = uc.smooth_autograd(T(fl).double(), T(im).double(), 10.0, s, second)
    reach = 2 if second else 1
    assert np.isnan(loss) == (h <= reach or w <= reach) and uc.rel_err(l2, loss) <= 1e-14
    assert uc.max_err(g2, g, tie) <= 1e-12 * max(np.abs(g).max(), 1e-30)
    assert tie.mean() <= uc.MAX_TIE_SHARE
    if h * w > 20:                               # the planted zero differences: decided (sign(0) = 0), not ties
        assert fl[0, 0, 1, 0] == fl[0, 0, 1, 1] == fl[0, 0, 1, 2] and not tie[0, 0, 1, :3].any()


def test_area_windows_and_nearest_rule_are_torchs():
    g = torch.Generator().manual_seed(5)
    for H, W, h, w in uc.AREA_CASES:
        x = torch.rand(2, 3, H, W, generator=g)
        out, mass, n = uc.area_ref(x.numpy(), h, w)
        want = F.interpolate(x.double(), (h, w), mode="area").numpy()
        assert np.abs(out - want).max() <= 1e-15 and n.min() >= 1
        got32 = F.interpolate(x, (h, w), mode="area").numpy()
        assert (np.abs(got32 - out) <= uc.area_bound(mass, n)).all()
        m = torch.rand(2, 1, H, W, generator=g)
        assert np.array_equal(uc.nearest_mask(m.numpy(), h, w), F.interpolate(m, (h, w), mode="nearest").numpy())
    assert any(H % h or W % w for H, W, h, w in uc.AREA_CASES) and any((H, W) == (h, w) for H, W, h, w in uc.AREA_CASES)
    for inp in (32, 48, 384, 640, 9, 11):
        for out in (1, 2, 3, 5, 7, inp // 2, inp // 4 or 1, inp):
            m = torch.arange(inp).float().view(1, 1, 1, inp)
            assert np.array_equal(uc.nearest_index(out, inp), F.interpolate(m, (1, out), mode="nearest").numpy().reshape(-1).astype(np.int64))


# ------------------------------------------------------------------------------------------------------------ the case table
def test_table_reaches_every_branch():
    TH, TW, MD = uc.geometry()
    assert TH > 0 and TW > 0 and TH * TW == 256 and MD == 3 and _lib.load().rcf_unflow_geometry(3) == 0
    cs = uc.CASES
    assert max(c.B * c.h * c.w for c in cs) <= 2 * 70 * 140 and all(c.B == 2 for c in cs)
    shapes = {(c.h, c.w) for c in cs}
    assert {(3, 3), (3, 40), (40, 3)} <= shapes
    assert any((c.h, c.w, c.md) == (5, 5, 2) for c in cs) and any((c.h, c.w, c.md) == (7, 7, 3) for c in cs)
    for md in (1, 3):
        of = [c for c in cs if c.md == md and c.grad]
        assert {TH, TH + 1, 2 * TH + 1} <= {c.h for c in of} and {TW, TW + 1, 2 * TW + 1} <= {c.w for c in of}
    assert any(c.h == TH - 1 and c.w == TW - 1 for c in cs)
    assert any(c.mask_size == (9, 11) and (c.h, c.w) == (4, 5) for c in cs)
    assert {"ones", "random", "zeros", "tile"} <= {c.mask for c in cs}
    assert {"gauss", "integer", "half", "edges", "far", "nan"} <= {c.flow for c in cs}
    assert any(c.image == "const" and not c.grad for c in cs)
    assert {(0.15, 0.0, 0.0), (0.0, 0.85, 0.0), (0.0, 0.0, 1.0), uc.ALL_W} <= {c.weights for c in cs}
    assert all(c.grad or c.mask == "zeros" or c.image == "const" for c in cs)          # forward-only cases are the two named kinds
    # what the kinds promise
    for c in cs:
        d = uc.inputs(c)
        if c.mask == "random" and d["occ"].size >= 400:
            assert 0.05 < 1 - d["occ"].mean() < 0.4
        if c.mask == "tile":
            assert not d["occ"][:, :, :TH, :TW].any() and d["occ"].mean() > 0.3
        if c.flow == "edges":
            t = wc.make_taps(d["flow"], "border")
            assert (~t.live_x).any() and (~t.live_y).any() and t.live_x.any()
        if c.flow == "nan":
            assert np.isnan(d["flow"]).any()
        if c.flow == "far":
            assert (np.abs(d["flow"]) >= 1e9).any()
        if c.flow in ("integer", "half"):
            assert np.array_equal(d["flow"] * 2, np.round(d["flow"] * 2))
        if c.image == "const":
            p, _, _ = uc.photo_truth(c)
            assert p.tie.mean() > uc.MAX_TIE_SHARE                                     # why it is forward only
    mods = uc.module_cases()
    assert any(not cfg.with_bk for _, cfg, _, _ in mods) and any(not cfg.occ_from_back for _, cfg, _, _ in mods)
    assert any(0 in cfg.w_scales[1:-1] and cfg.w_scales[2] != 0 for _, cfg, _, _ in mods)      # a weight of 0 in the middle
    assert any(cfg.get("smooth_2nd") for _, cfg, _, _ in mods) and any(cfg.w_real_smooth > 0 and not cfg.get("smooth_2nd") for _, cfg, _, _ in mods)


# ------------------------------------------------------------------------------------------------------------ host surface
def test_module_refuses_what_it_does_not_build():
    assert isinstance(rcf_amd.unFlowLoss(uc.fcn_cfg()), torch.nn.Module) and rcf_amd.unFlowLoss(uc.fcn_cfg()).ssim_sz == 1
    with pytest.raises(NotImplementedError):
        rcf_amd.unFlowLoss(uc.fcn_cfg(warp_pad="zeros"))
    with pytest.raises(NotImplementedError):
        rcf_amd.unFlowLoss(uc.fcn_cfg(ssim_sz=4))
    B, H, W = 1, 32, 48
    flows = [torch.zeros(B, 4, H >> l, W >> l) for l in range(5)]
    target = torch.zeros(B, 6, H, W)
    with pytest.raises(_lib.RcfHipError, match="no CPU"):
        rcf_amd.unFlowLoss(uc.fcn_cfg())(flows, target)
    with pytest.raises(_lib.RcfHipError, match="level 3 is 2 x 3"):      # a 16 x 24 pyramid: level 3 is under the 3 x 3 window
        rcf_amd.unFlowLoss(uc.fcn_cfg())(flows[1:] + [torch.zeros(B, 4, 1, 1)], target)
    x = torch.zeros(1, 3, 5, 5)
    for call in (lambda: rcf_amd.ops.unflow_photo(x, x, x[:, :2], x[:, :1]), lambda: rcf_amd.ops.unflow_smooth(x[:, :2], x),
                 lambda: rcf_amd.ops.area_resize(x, (2, 2)), lambda: rcf_amd.ops.unflow_photo_bwd(x, x, x[:, :2], x[:, :1], x, x),
                 lambda: rcf_amd.ops.unflow_smooth_bwd(x[:, :2], x, x)):
        with pytest.raises(_lib.RcfHipError):
            call()


def test_entries_refuse_before_touching_a_device():
    """sizes and ranges first (with every pointer NULL the status is the same), then pointers: nothing is launched -- there is no
    device here -- and the host buffer keeps its fill"""
    lib = _lib.load()
    buf = (ctypes.c_float * 64)(*([7.0] * 64))
    p = ctypes.cast(buf, ctypes.c_void_p)
    fwd, bwd = lib.rcf_unflow_photo_fwd_f32, lib.rcf_unflow_photo_bwd_f32
    sfwd, sbwd, area = lib.rcf_unflow_smooth_fwd_f32, lib.rcf_unflow_smooth_bwd_f32, lib.rcf_unflow_area_f32

    def photo(ptrs, B, h, w, md, H0=None, W0=None, bs=None):
        H0, W0 = H0 or h, W0 or w
        bs = 2 * h * w if bs is None else bs
        a, b, c, d, e, f, g = ptrs
        if g is None and None not in ptrs[:6]:          # the seventh pointer is the backward's alone
            return (-1, bwd(a, b, c, bs, d, H0, W0, md, 0.15, 0.85, 0.0, e, f, g, B, h, w, None))
        return (fwd(a, b, c, bs, d, H0, W0, md, 0.15, 0.85, 0.0, e, f, 1 << 40, B, h, w, None),
                bwd(a, b, c, bs, d, H0, W0, md, 0.15, 0.85, 0.0, e, f, g, B, h, w, None))

    bad = [(0, 8, 8, 1), (-1, 8, 8, 1), (1, 0, 8, 1), (1, 8, 0, 1), (1, 8, 8, 0), (1, 8, 8, 4), (1, 8, 8, -1),
           (1, 2, 8, 1), (1, 8, 2, 1), (1, 4, 8, 2), (1, 8, 4, 2), (1, 6, 8, 3), (1, 8, 6, 3),       # under the window
           (1, 32768, 32768, 1), (1, 1 << 15, 1 << 16, 1), (2147483647, 2147483647, 2147483647, 3)]      # h w >= 2^30
    for B, h, w, md in bad:
        for ptr in (p, None):
            assert photo([ptr] * 7, B, h, w, md) == (-1, -1), (B, h, w, md)
    assert photo([p] * 7, 1, 8, 8, 1, H0=-1) == (-1, -1) and photo([p] * 7, 1, 8, 8, 1, W0=1 << 30) == (-1, -1)
    assert photo([p] * 7, 2, 8, 8, 1, bs=127) == (-1, -1)
    for k in range(7):
        a = [p] * 7
        a[k] = None
        assert photo(a, 1, 8, 8, 1) == (-1, -1), k
    assert fwd(p, p, p, 128, p, 8, 8, 1, 0.15, 0.85, 0.0, p, p, 3, 1, 8, 8, None) == -2          # a workspace of 3 doubles
    assert lib.rcf_unflow_photo_partials(1, 8, 8) == 4 and lib.rcf_unflow_photo_partials(2, 9, 33) == 4 * 2 * 2 * 2
    for B, h, w in ((0, 4, 4), (1, 0, 4), (1, 4, 0), (1, 32768, 32768)):
        for ptr in (p, None):
            assert sfwd(ptr, 2 * h * w, ptr, 10.0, 4.0, 0, ptr, ptr, B, h, w, None) == -1
            assert sbwd(ptr, 2 * h * w, ptr, 10.0, 4.0, 0, ptr, ptr, B, h, w, None) == -1
            assert area(ptr, 3 * h * w, ptr, B, h, w, 2, 2, None) == -1 and area(ptr, 12, ptr, max(B, 1), 2, 2, h, w if B else 0, None) == -1
    assert sfwd(p, 32, p, 10.0, 4.0, 2, p, p, 1, 4, 4, None) == -1 and sbwd(p, 31, p, 10.0, 4.0, 0, p, p, 1, 4, 4, None) == -1
    for k in range(4):
        a = [p] * 4
        a[k] = None
        assert sfwd(a[0], 32, a[1], 10.0, 4.0, 0, a[2], a[3], 1, 4, 4, None) == -1
        assert sbwd(a[0], 32, a[1], 10.0, 4.0, 0, a[2], a[3], 1, 4, 4, None) == -1
    assert area(None, 48, p, 1, 4, 4, 2, 2, None) == -1 and area(p, 48, None, 1, 4, 4, 2, 2, None) == -1 and area(p, 47, p, 1, 4, 4, 2, 2, None) == -1
    assert list(buf) == [7.0] * 64
