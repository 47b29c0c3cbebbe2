"""The host side of rcf_amd.PWCLite and the conditioning of its sweep (tests/pwc_cases.py), without a GPU: the vector-segment
restatement reproduces the reference-made fixture (tests/golden/pwclite.npz); the module's state dict carries the reference's names
and shapes; every kernel restatement's analytic backward equals torch autograd of its forward; the resize adjoint is the adjoint;
the case tables reach the branches they name, judged by the library's own geometry query; the entry points refuse bad arguments
before they touch a device; the module refuses what it does not build."""
import ctypes
import os

import numpy as np
import pytest
import torch
import torch.nn.functional as F

import pwc_cases as pc
import rcf_amd
from rcf_amd import _lib


@pytest.fixture(scope="module")
def golden(golden_dir):
    return np.load(os.path.join(golden_dir, "pwclite.npz"))


_REF = {}


def ref_run(k):
    if k not in _REF:
        _REF[k] = pc.run_ref(pc.GOLDEN[k])
    return _REF[k]


def rel(got, want):
    return float(np.abs(got - want).max() / max(np.abs(want).max(), 1e-300))


# ----------------------------------------------------------------------------------------------------- against the reference
def test_fixture_is_small_and_holds_the_cases(golden, golden_dir):
    assert os.path.getsize(os.path.join(golden_dir, "pwclite.npz")) < 200 * 1024
    assert [c.name for c in pc.GOLDEN] == ["smallest", "tiles"] and (pc.GOLDEN[0].H, pc.GOLDEN[0].W, pc.GOLDEN[0].M) == (64, 128, 5)
    assert (pc.GOLDEN[1].H, pc.GOLDEN[1].W, pc.GOLDEN[1].M) == (128, 192, 2) and all(c.B == 2 for c in pc.GOLDEN)
    n_par = len(pc.param_shapes())
    for k, c in enumerate(pc.GOLDEN):
        n_out = 2 * (5 + 5 + c.M + 1)
        assert golden[f"e32_{k}"].shape == golden[f"amax_{k}"].shape == (n_out + 2 + n_par,)
        rel32 = golden[f"e32_{k}"] / np.maximum(golden[f"amax_{k}"], 1e-300)
        assert rel32.max() <= 1e-5                                        # the yardstick: the reference's own float32 run
        assert sum(f.startswith(f"out_{k}_") for f in golden.files) == n_out
        frames, masks = pc.draw_inputs(c)
        assert np.array_equal(frames * 255, np.round(frames * 255)) and np.abs(masks.sum(2) - 1).max() < 1e-6
        flows = max(np.abs(golden[f]).max() for f in golden.files if f.startswith(f"out_{k}_") and "group" not in f)
        assert 0.5 < flows < 10                                           # flows of pixels, not of a hundred
        assert pc.kink_distance(c) >= pc.MIN_KINK_DISTANCE                # no slope of the float64 run is a tie for a float32 run


@pytest.mark.parametrize("k", range(len(pc.GOLDEN)))
def test_restatement_equals_the_reference(golden, k):
    outs, gp, gm = ref_run(k)
    worst = {"out": 0.0, "mask": 0.0, "param": 0.0}
    for key, t in outs.items():
        want = golden[f"out_{k}_{key}"]
        e = rel(t.reshape(-1)[pc.sample(t.numel(), pc.OUT_BUDGET)].numpy(), want)
        if key.endswith("_group_0"):
            # the -1 accumulator: the reference keeps it in float32 whatever the run's dtype (the `.float()` of its initial zeros,
            # which only this entry never leaves) and interpolates it five times, six roundings each
            assert e <= 32 * pc.U32, key
            continue
        worst["out"] = max(worst["out"], e)
    for i, t in enumerate(gm):
        worst["mask"] = max(worst["mask"], rel(t.reshape(-1)[pc.sample(t.numel(), pc.MASK_BUDGET)].numpy(), golden[f"dmask_{k}_{i}"]))
    for j, (name, t) in enumerate(gp.items()):
        want = golden[f"dparam_{k}_{j}"]
        assert np.abs(want).max() > 0, name
        worst["param"] = max(worst["param"], rel(t.reshape(-1)[pc.sample(t.numel(), pc.GRAD_BUDGET, 1)].numpy(), want))
    print(f"pwclite golden {pc.GOLDEN[k].name}: restatement vs the reference's float64 run, relative to each tensor's range {worst}")
    assert max(worst.values()) <= 1e-10


def test_state_dict_is_the_references(golden):
    names = [str(n) for n in golden["names"]]
    shapes, cur = [], []
    for v in golden["shapes"]:
        if v < 0:
            shapes.append(tuple(cur))
            cur = []
        else:
            cur.append(int(v))
    assert list(zip(names, shapes)) == pc.param_shapes()
    for M in (1, 5):
        net = rcf_amd.PWCLite(M)
        sd = net.state_dict()
        assert [(k, tuple(v.shape)) for k, v in sd.items()] == list(zip(names, shapes))
        assert net.num_parameters() == sum(int(np.prod(s)) for s in shapes) == 1721714
        assert (net.search_range, net.output_level, net.upsample, net.mask_layer) == (4, 4, True, M) and net.num_chs == pc.NUM_CHS
    net.load_state_dict({k: torch.from_numpy(v) for k, v in pc.draw_params(1).items()}, strict=True)
    assert torch.equal(net.flow_estimators.conv1[0].weight, torch.from_numpy(pc.draw_params(1)["flow_estimators.conv1.0.weight"]))
    net.init_weights()
    assert all(float(p.detach().abs().max()) == 0 for n, p in net.named_parameters() if n.endswith("bias"))
    # conv1's operand: [x1_1by1 32 | corr 81 | flow 2 | zero 1] from the reference's [corr | x1_1by1 | flow]
    c1 = net.flow_estimators.conv1[0]
    wp, bp = c1.packed()
    assert tuple(wp.shape) == (128, 116, 3, 3) and wp.permute(0, 2, 3, 1).is_contiguous() and float(wp[:, 115].abs().max()) == 0
    assert torch.equal(wp[:, :32], c1.weight[:, 81:113]) and torch.equal(wp[:, 32:113], c1.weight[:, :81]) and torch.equal(wp[:, 113:115], c1.weight[:, 113:])
    assert c1.packed()[0] is wp                                           # cached per weight version
    with torch.no_grad():
        c1.weight.mul_(2)
    assert c1.packed()[0] is not wp and torch.equal(c1.packed()[0][:, :32], c1.weight[:, 81:113])
    p2 = net.flow_estimators.predict_flow2[0].packed()
    assert tuple(p2[0].shape) == (4, 64, 1, 1) and tuple(p2[1].shape) == (4,) and float(p2[0][2:].abs().max()) == 0


# ------------------------------------------------------------------------------------------------- gradients of the restatements
@pytest.mark.parametrize("c", [pytest.param(c, id=c.name) for c in pc.seg_cases()])
def test_segment_restatements_analytic_equals_autograd(c):
    d = pc.seg_inputs(c)
    feat = d["wide"][..., c.c0:c.c0 + c.C].double().requires_grad_(True)
    mask = d["mask"].double().requires_grad_(True)
    pooled, msum, mass = pc.pool_ref(feat, mask)
    (pooled * d["dpooled"].double()).sum().backward()
    dfeat, dmask, _, _ = pc.pool_bwd_ref(feat.detach(), mask.detach(), pooled.detach(), msum.detach(), d["dpooled"].double())
    assert pc.rel_err(dfeat, feat.grad) <= 1e-12 and pc.rel_err(dmask, mask.grad) <= 1e-12
    assert bool((mass >= pooled.abs() * (1 - 1e-12)).all())
    mask2, group = d["mask"].double().requires_grad_(True), d["group"].double().requires_grad_(True)
    flow, _ = pc.flow_ref(mask2, group)
    (flow * d["dflow"].double()).sum().backward()
    dm, dg, _, _ = pc.flow_bwd_ref(mask2.detach(), group.detach(), d["dflow"].double())
    assert pc.rel_err(dm, mask2.grad) <= 1e-12 and pc.rel_err(dg, group.grad) <= 1e-12


def test_elementwise_restatements_analytic_equals_autograd():
    g = torch.Generator().manual_seed(3)
    x = torch.randn(5, 7, 8, generator=g, dtype=torch.float64).requires_grad_(True)
    y = F.leaky_relu(x, pc.SLOPE)
    dy = torch.randn(5, 7, 8, generator=g, dtype=torch.float64)
    (y * dy).sum().backward()
    assert torch.equal(pc.leaky_bwd_ref(dy, y.detach()), x.grad)
    zero = torch.tensor([0.0, -0.0, 1e-30, -1e-30], dtype=torch.float64)
    assert pc.leaky_bwd_ref(torch.ones(4, dtype=torch.float64), zero).tolist() == [pc.SLOPE, pc.SLOPE, 1.0, pc.SLOPE]
    for B, h, w in pc.PACK:
        corr = torch.randn(B, 81, h, w, generator=g, dtype=torch.float64).requires_grad_(True)
        flow = torch.randn(B, 2, h, w, generator=g, dtype=torch.float64).requires_grad_(True)
        buf = torch.full((B, h, w, 116), 7.0, dtype=torch.float64)
        out = pc.pack_ref(corr, flow, buf, 32)
        assert float(out.detach()[..., 115].abs().max()) == 0 and bool((out[..., :32] == 7).all())
        d = torch.randn(B, h, w, 116, generator=g, dtype=torch.float64)
        (out * d).sum().backward()
        dc, df = pc.unpack_ref(d, 32, 81)
        assert torch.equal(dc, corr.grad) and torch.equal(df, flow.grad)


@pytest.mark.parametrize("planes,Hi,Wi,Ho,Wo", pc.RESIZE)
@pytest.mark.parametrize("align", [True, False])
def test_resize_adjoint_is_the_adjoint(planes, Hi, Wi, Ho, Wo, align):
    g = torch.Generator().manual_seed(Hi * 100 + Wo)
    x = torch.randn(planes, Hi, Wi, generator=g, dtype=torch.float64)
    y = torch.randn(planes, Ho, Wo, generator=g, dtype=torch.float64)
    Rx = pc.resize_fwd_ref(x, Ho, Wo, align)
    Rty, mass, terms = pc.resize_adjoint_ref(y, Hi, Wi, align)
    a, b = float((Rx * y).sum()), float((x * Rty).sum())
    assert abs(a - b) <= 1e-13 * float((Rx.abs() * y.abs()).sum())
    want = F.interpolate(x[None], size=(Ho, Wo), mode="bilinear", align_corners=align)[0]
    # torch's float64 run takes its positions in float64, the kernels (and torch's float32 run) in float32: a position of up to 40
    # carries 40 * 2^-24 of error, times a difference of neighbours of up to ~6
    assert float((Rx - want).abs().max()) <= 6 * max(Hi, Wi) * 2 * pc.U32
    if (Hi, Wi) == (Ho, Wo):
        assert torch.equal(Rty, y) and int(terms.max()) == 1
    if Hi > 2 * Ho:
        assert float((terms == 0).double().mean()) > 0.5 and bool((Rty[:, terms == 0] == 0).all())      # most inputs receive nothing


# ------------------------------------------------------------------------------------------------------------ the case tables
def test_tables_reach_every_branch():
    chunk, maxm, maxc, tile, packc = pc.geometry()
    assert chunk > 0 and maxm >= 5 and maxc >= 96 and tile > 0 and packc >= 84 and _lib.load().rcf_pwc_geometry(5) == 0
    cs = pc.seg_cases()
    px = [c.h * c.w for c in cs]
    assert 2 in px and any(2 < p < chunk for p in px) and any(p > chunk and p % chunk for p in px) and chunk + 1 in px
    assert any(p > 3 * chunk for p in px)
    assert {1, 2, 5, maxm} <= {c.M for c in cs} and {4, 96} <= {c.C for c in cs}
    assert any(c.C == 96 and c.pitch == 448 and c.c0 > 0 for c in cs) and {0, 1} <= {c.beta for c in cs}
    tiny = [c for c in cs if c.mask == "tiny"]
    assert tiny and all(abs(float(pc.seg_inputs(c)["mask"].sum((2, 3)).max()) - 1e-6) < 1e-8 for c in tiny)
    assert (1, 2, 2, 4) in [r[1:] for r in pc.RESIZE] and (24, 40, 6, 10) in [r[1:] for r in pc.RESIZE]
    assert any(r[1:3] == r[3:5] for r in pc.RESIZE) and (3, 5, 6, 10) in [r[1:] for r in pc.RESIZE] and (5, 7, 20, 28) in [r[1:] for r in pc.RESIZE]
    assert {4, 448} <= {c for _, c, _, _, _ in pc.LEAKY} and any(dp > c for _, c, dp, _, _ in pc.LEAKY) and any(dp == yp == gp == c for _, c, dp, yp, gp in pc.LEAKY)
    assert any(h * w == 2 for _, h, w in pc.PACK) and any(h * w > tile and (h * w) % tile for _, h, w in pc.PACK)
    # the fixture's levels: one row at level 0 of the first case, levels that cross 8 x 32 in the second
    assert pc.GOLDEN[0].H // 64 == 1 and pc.GOLDEN[1].H // 4 == 32 and pc.GOLDEN[1].W // 4 == 48


# ------------------------------------------------------------------------------------------------------------ host surface
def test_module_refuses_what_it_does_not_build():
    net = rcf_amd.PWCLite(2)
    x = torch.zeros(1, 6, 64, 64)
    m = [torch.zeros(1, 2, 16, 16)] * 2
    with pytest.raises(_lib.RcfHipError, match="no CPU"):
        net(x, m)
    if torch.cuda.is_available():
        x, m, net = x.cuda(), [t.cuda() for t in m], net.cuda()
        with pytest.raises(_lib.RcfHipError, match="float32"):
            net(x.half(), m)
        with pytest.raises(_lib.RcfHipError, match=r"\[B, 6, H, W\]"):
            net(x[:, :5], m)
        with pytest.raises(_lib.RcfHipError, match="multiples of 64"):
            net(x[:, :, :48], m)
        with pytest.raises(_lib.RcfHipError, match="mask_layer = 2"):
            net(x, [torch.zeros(1, 3, 16, 16).cuda()] * 2)
    else:
        # without a device the order of the checks is what can be seen: device first, then the type and the shapes
        check = rcf_amd.PWCLite._check

        class Cuda(torch.Tensor):          # a CPU tensor that says it is on the device: the later refusals, reached without one
            is_cuda = True

        def on(t):
            return t.as_subclass(Cuda)
        with pytest.raises(_lib.RcfHipError, match="float32"):
            check(net, on(x.half()), [on(t) for t in m])
        with pytest.raises(_lib.RcfHipError, match=r"\[B, 6, H, W\]"):
            check(net, on(x[:, :5]), [on(t) for t in m])
        with pytest.raises(_lib.RcfHipError, match="multiples of 64"):
            check(net, on(x[:, :, :48]), [on(t) for t in m])
        with pytest.raises(_lib.RcfHipError, match="mask_layer = 2"):
            check(net, on(x), [on(torch.zeros(1, 3, 16, 16))] * 2)
        check(net, on(x), [on(t) for t in m])
    f = torch.zeros(1, 2, 2, 4)
    k = torch.zeros(1, 1, 2, 2)
    for call in (lambda: rcf_amd.ops.segment_pool(f, k), lambda: rcf_amd.ops.segment_pool_bwd(f, k, f, f, f),
                 lambda: rcf_amd.ops.segment_flow(k, torch.zeros(1, 1, 2)), lambda: rcf_amd.ops.segment_flow_bwd(k, torch.zeros(1, 1, 2), f),
                 lambda: rcf_amd.ops.resize_nchw_bwd(k, (4, 4), True), lambda: rcf_amd.ops.leaky_bwd(f, f, 0.1),
                 lambda: rcf_amd.ops.pwc_pack(k, f[:, :, :, :2].permute(0, 3, 1, 2), f, 0), lambda: rcf_amd.ops.pwc_unpack(f, 0, 1)):
        with pytest.raises(_lib.RcfHipError, match="no CPU"):
            call()


def test_entries_refuse_before_touching_a_device():
    """sizes and ranges first (with every pointer NULL the status is the same), then pointers: nothing is launched -- there is no
    device here -- and the host buffer keeps its fill"""
    lib = _lib.load()
    chunk, maxm, maxc, tile, packc = pc.geometry()
    buf = (ctypes.c_float * 64)(*([7.0] * 64))
    p = ctypes.cast(buf, ctypes.c_void_p)
    big = 1 << 40

    # a call with nothing wrong would launch on host memory: every call below has something to refuse, `only` picks the entry point
    def pool(ptrs, B, M, C, hw, pitch=None, dpitch=None, beta=0, n=big, only=None):
        pitch, dpitch = C if pitch is None else pitch, C if dpitch is None else dpitch
        a = ptrs
        fwd = None if only == "bwd" else lib.rcf_pwc_segment_pool_fwd_f32(a[0], pitch, a[1], a[2], a[3], a[4], n, B, M, C, hw, None)
        bwd = None if only == "fwd" else lib.rcf_pwc_segment_pool_bwd_f32(a[0], pitch, a[1], a[2], a[3], a[4], a[5], dpitch, beta, a[6], B, M,
                                                                          C, hw, None)
        return fwd, bwd

    def flow(ptrs, B, M, hw, beta=0, n=big, only=None):
        a = ptrs
        fwd = None if only == "bwd" else lib.rcf_pwc_segment_flow_fwd_f32(a[0], a[1], a[2], B, M, hw, None)
        bwd = None if only == "fwd" else lib.rcf_pwc_segment_flow_bwd_f32(a[0], a[1], a[2], a[3], beta, a[4], a[5], n, B, M, hw, None)
        return fwd, bwd

    bad = [(0, 1, 4, 8), (-1, 1, 4, 8), (65536, 1, 4, 8), (1, 0, 4, 8), (1, maxm + 1, 4, 8), (1, 1, 0, 8), (1, 1, 6, 8), (1, 1, maxc + 4, 8),
           (1, 1, 4, 0), (1, 1, 4, -3), (1, 1, 4, 1 << 30)]
    for B, M, C, hw in bad:
        for ptr in (p, None):
            assert pool([ptr] * 7, B, M, C, hw) == (-1, -1), (B, M, C, hw)
            if C == 4:
                assert flow([ptr] * 6, B, M, hw) == (-1, -1), (B, M, hw)
        assert lib.rcf_pwc_pool_partials(B, M, C, hw) == 0
    assert pool([p] * 7, 1, 1, 8, 4, pitch=4) == (-1, -1) and pool([p] * 7, 1, 1, 4, 4, pitch=6) == (-1, -1)
    assert pool([p] * 7, 1, 1, 4, 4, dpitch=6, only="bwd")[1] == -1 and pool([p] * 7, 1, 1, 4, 4, beta=2, only="bwd")[1] == -1
    assert flow([p] * 6, 1, 1, 4, beta=2, only="bwd")[1] == -1
    for k in range(7):                                                  # the forward's pointers are the first five
        a = [p] * 7
        a[k] = None
        assert pool(a, 1, 2, 4, 8, only="bwd")[1] == -1, k
        if k < 5:
            assert pool(a, 1, 2, 4, 8, only="fwd")[0] == -1, k
    odd = ctypes.c_void_p(p.value + 4)                                  # not 16-byte aligned
    assert pool([odd] + [p] * 6, 1, 2, 4, 8) == (-1, -1)
    assert pool([p] * 7, 1, 2, 4, 8, n=9, only="fwd")[0] == -2 and lib.rcf_pwc_pool_partials(1, 2, 4, 8) == 10
    assert lib.rcf_pwc_pool_partials(2, 5, 96, chunk + 1) == 2 * 2 * 5 * 97 and lib.rcf_pwc_flow_partials(2, 5, chunk + 1) == 2 * 2 * 5 * 2
    for k in (0, 1, 2, 4, 5):                                           # a NULL dmask (index 3) is a constant mask; the forward's are 0..2
        a = [p] * 6
        a[k] = None
        assert flow(a, 1, 2, 8, only="bwd")[1] == -1, k
        if k < 3:
            assert flow(a, 1, 2, 8, only="fwd")[0] == -1, k
    assert flow([p] * 6, 1, 2, 8, n=3, only="bwd")[1] == -2
    leaky, pack, unpack, rsz = lib.rcf_pwc_leaky_bwd_f32, lib.rcf_pwc_pack_f32, lib.rcf_pwc_unpack_f32, lib.rcf_resize_bilinear_nchw_bwd_f32
    for ptr in (p, None):
        for rows, C, a, b, c in ((0, 4, 4, 4, 4), (-1, 4, 4, 4, 4), (3, 0, 4, 4, 4), (3, 6, 8, 8, 8), (3, 8, 4, 8, 8), (3, 8, 8, 4, 8), (3, 8, 8, 8, 4),
                                 (3, 4, 6, 4, 4), (1 << 40, 4, 4, 4, 4)):
            assert leaky(ptr, a, ptr, b, ptr, c, rows, C, 0.1, None) == -1
        for pitch, c0, D, B, hw in ((116, 32, 81, 0, 4), (116, 32, 81, 1, 0), (116, 32, 0, 1, 4), (116, 30, 81, 1, 4), (114, 32, 81, 1, 4),
                                    (112, 32, 81, 1, 4), (116, -4, 81, 1, 4), (256, 0, packc - 1, 1, 4), (116, 32, 81, 65536, 4), (116, 32, 81, 1, 1 << 30)):
            assert pack(ptr, ptr, ptr, pitch, c0, D, B, hw, None) == -1 and unpack(ptr, pitch, c0, ptr, ptr, D, B, hw, None) == -1
        for planes, Hi, Wi, Ho, Wo in ((0, 2, 2, 4, 4), (1, 0, 2, 4, 4), (1, 2, 0, 4, 4), (1, 2, 2, 0, 4), (1, 2, 2, 4, -1), (1, 1 << 15, 1 << 15, 4, 4)):
            assert rsz(ptr, ptr, planes, Hi, Wi, Ho, Wo, 1, None) == -1
    for k in range(3):
        a = [p] * 3
        a[k] = None
        assert leaky(a[0], 4, a[1], 4, a[2], 4, 3, 4, 0.1, None) == -1
        assert pack(a[0], a[1], a[2], 116, 32, 81, 1, 2, None) == -1 and unpack(a[0], 116, 32, a[1], a[2], 81, 1, 2, None) == -1
    assert leaky(odd, 4, p, 4, p, 4, 3, 4, 0.1, None) == -1
    assert rsz(None, p, 1, 2, 2, 4, 4, 1, None) == -1 and rsz(p, None, 1, 2, 2, 4, 4, 1, None) == -1
    assert list(buf) == [7.0] * 64
