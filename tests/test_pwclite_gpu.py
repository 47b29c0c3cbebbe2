"""rcf_amd.PWCLite and the kernels of csrc/pwc.hip on the device.

Kernel sweep: every new kernel against its float64 restatement (tests/pwc_cases.py) per element, under k 2^-24 mass with the k
csrc/pwc.hip states beside each kernel (mass: the sum of the absolute terms).  Whole module: outputs and the gradients of a fixed
linear functional with respect to both masks and every parameter against the reference's float64 run (tests/golden/pwclite.npz);
per tensor the error may reach max(6 e32, 16 2^-24 max |truth|), e32 being the reference's own float32 run's error -- the project's
standing margin (README, parity).  Measured margins of a run: profiles/pwclite_parity.txt."""
import os

import numpy as np
import pytest
import torch

import pwc_cases as pc
import rcf_amd
from rcf_amd import ops

pytestmark = pytest.mark.gpu
U = pc.U32
DEV = "cuda"


def dev(t):
    return t.to(DEV)


# ================================================================================================================ kernel sweep
@pytest.mark.parametrize("c", [pytest.param(c, id=c.name) for c in pc.seg_cases()])
def test_segment_pool_sweep(c, report):
    d = pc.seg_inputs(c)
    wide = dev(d["wide"])
    feat, mask = wide[..., c.c0:c.c0 + c.C], dev(d["mask"])
    pooled, msum = ops.segment_pool(feat, mask)
    f64, m64 = d["wide"][..., c.c0:c.c0 + c.C].double(), d["mask"].double()
    want, wsum, mass = pc.pool_ref(f64, m64)
    a = pc.margin(pooled.cpu(), want, 3 * U * mass)
    b = pc.margin(msum.cpu(), wsum, 3 * U * m64.abs().sum((2, 3)))
    # backward from the forward's own pooled and msum, onto a buffer that holds `old` everywhere
    old = dev(d["old"]).clone()
    dfeat, dmask = ops.segment_pool_bwd(feat, mask, pooled, msum, dev(d["dpooled"]), dfeat=old[..., c.c0:c.c0 + c.C], beta=c.beta)
    wf, wm, mf, mm = pc.pool_bwd_ref(f64, m64, pooled.cpu().double(), msum.cpu().double(), d["dpooled"].double())
    o64 = d["old"][..., c.c0:c.c0 + c.C].double() * c.beta
    e = pc.margin(dfeat.cpu(), wf + o64, (c.M + 4) * U * (mf + o64.abs()))
    f = pc.margin(dmask.cpu(), wm, 3 * U * mm)
    report(f"pwc pool {c.name}: margins pooled {a:.3f} msum {b:.3f} dfeat {e:.3f} dmask {f:.3f} (1 = the bound)")
    assert max(a, b, e, f) <= 1
    keep = torch.ones(c.pitch, dtype=torch.bool)
    keep[c.c0:c.c0 + c.C] = False
    assert torch.equal(old.cpu()[..., keep], d["old"][..., keep])              # the rest of the buffer is untouched
    p2, s2 = ops.segment_pool(feat, mask)
    assert torch.equal(p2, pooled) and torch.equal(s2, msum)                    # the same bits on every call


@pytest.mark.parametrize("c", [pytest.param(c, id=c.name) for c in pc.seg_cases()])
def test_segment_flow_sweep(c, report):
    d = pc.seg_inputs(c)
    mask, group, dflow = dev(d["mask"]), dev(d["group"]), dev(d["dflow"])
    m64, g64, d64 = d["mask"].double(), d["group"].double(), d["dflow"].double()
    flow = ops.segment_flow(mask, group)
    want, mass = pc.flow_ref(m64, g64)
    a = pc.margin(flow.cpu(), want, (c.M + 2) * U * mass)
    old = dev(d["old_mask"]).clone()
    dmask, dgroup = ops.segment_flow_bwd(mask, group, dflow, dmask=old, beta=c.beta)
    wm, wg, mm, mg = pc.flow_bwd_ref(m64, g64, d64)
    o64 = d["old_mask"].double() * c.beta
    b = pc.margin(dmask.cpu(), wm + o64, 5 * U * (mm + o64.abs()))
    e = pc.margin(dgroup.cpu(), wg, 3 * U * mg)
    report(f"pwc compose {c.name}: margins flow {a:.3f} dmask {b:.3f} dgroup {e:.3f}")
    assert max(a, b, e) <= 1 and dmask.data_ptr() == old.data_ptr()
    none, dg2 = ops.segment_flow_bwd(mask, group, dflow, need_dmask=False)
    assert none is None and torch.equal(dg2, dgroup)


@pytest.mark.parametrize("planes,Hi,Wi,Ho,Wo", pc.RESIZE)
@pytest.mark.parametrize("align", [True, False])
def test_resize_adjoint_sweep(planes, Hi, Wi, Ho, Wo, align, report):
    g = torch.Generator().manual_seed(Hi * 100 + Wo)
    dy = torch.randn(planes, Ho, Wo, generator=g)
    out = torch.full((planes, Hi, Wi), float("nan"), device=DEV)
    got = ops.resize_nchw_bwd(dev(dy), (Hi, Wi), align, out=out).cpu()
    want, mass, terms = pc.resize_adjoint_ref(dy.double(), Hi, Wi, align)
    m = pc.margin(got, want, (terms[None].double() + 7) * U * mass)
    report(f"pwc resize adjoint {Hi}x{Wi} <- {Ho}x{Wo} align {align}: margin {m:.3f}, {int((terms == 0).sum())} of {Hi * Wi} inputs receive nothing")
    assert m <= 1 and bool((got[:, terms == 0] == 0).all())
    if (Hi, Wi) == (Ho, Wo):
        assert torch.equal(got, dy)
    # the adjoint of the forward the library has: <R x, dy> = <x, R^T dy>
    x = torch.randn(planes, Hi, Wi, generator=g)
    Rx = ops.resize_nchw(dev(x), (Ho, Wo), align).cpu().double()
    lhs, rhs = float((Rx * dy.double()).sum()), float((x.double() * got.double()).sum())
    assert abs(lhs - rhs) <= 32 * U * float((Rx.abs() * dy.double().abs()).sum())


@pytest.mark.parametrize("rows,C,dp,yp,gp", pc.LEAKY)
def test_leaky_bwd_sweep(rows, C, dp, yp, gp):
    g = torch.Generator().manual_seed(rows + C)
    dyw, yw = torch.randn(1, 1, rows, dp, generator=g), torch.randn(1, 1, rows, yp, generator=g)
    yw[0, 0, ::3, 0], yw[0, 0, 1::3, 1] = 0.0, -0.0
    gw = torch.full((1, 1, rows, gp), 7.0)
    dy, y, out = dev(dyw)[..., :C], dev(yw)[..., :C], dev(gw)
    got = ops.leaky_bwd(dy, y, pc.SLOPE, out=out[..., :C])
    want = pc.leaky_bwd_ref(dyw[..., :C].double(), yw[..., :C].double())
    assert pc.margin(got.cpu(), want, 3 * U * dyw[..., :C].double().abs()) <= 1
    assert torch.equal(got.cpu()[0, 0, ::3, 0], dyw[0, 0, ::3, 0] * torch.tensor(pc.SLOPE))           # y = 0 takes the slope
    assert torch.equal(got.cpu()[0, 0, 1::3, 1], dyw[0, 0, 1::3, 1] * torch.tensor(pc.SLOPE))         # and so does -0.0
    assert bool((out.cpu()[..., C:] == 7).all())
    dense = ops.leaky_bwd(dy, y, pc.SLOPE)
    assert dense.is_contiguous() and torch.equal(dense, got)


@pytest.mark.parametrize("B,h,w", pc.PACK)
def test_pack_and_unpack(B, h, w):
    g = torch.Generator().manual_seed(h * w)
    corr, flow = torch.randn(B, 81, h, w, generator=g), torch.randn(B, 2, h, w, generator=g)
    buf = torch.randn(B, h, w, 116, generator=g)
    got = ops.pwc_pack(dev(corr), dev(flow), dev(buf).clone(), 32).cpu()
    assert torch.equal(got, pc.pack_ref(corr, flow, buf, 32))
    assert float(got[..., 115].abs().max()) == 0 and torch.equal(got[..., :32], buf[..., :32])
    dcorr, dflow = ops.pwc_unpack(dev(buf), 32, 81)
    wc, wf = pc.unpack_ref(buf, 32, 81)
    assert torch.equal(dcorr.cpu(), wc) and torch.equal(dflow.cpu(), wf)
    wide = torch.randn(B, h, w, 12, generator=g)                                    # another geometry: D = 1 at channel 4, no guard
    got = ops.pwc_pack(dev(corr[:, :1].contiguous()), dev(flow), dev(wide).clone(), 4).cpu()
    assert torch.equal(got, pc.pack_ref(corr[:, :1], flow, wide, 4))


# =============================================================================================================== whole module
_RUNS = {}


def native_run(k):
    """one forward and backward of the module on fixture case k, shared by the tests"""
    if k not in _RUNS:
        c = pc.GOLDEN[k]
        frames, masks = pc.draw_inputs(c)
        net = rcf_amd.PWCLite(c.M).to(DEV)
        net.load_state_dict({n: torch.from_numpy(v) for n, v in pc.draw_params(c.seed).items()}, strict=True)
        m = [dev(torch.from_numpy(masks[i])).requires_grad_(True) for i in range(2)]
        x = dev(torch.from_numpy(frames))
        res = net(x, m)
        pc.functional(res, c.seed).backward()
        torch.cuda.synchronize()
        _RUNS[k] = (net, x, m, res)
    return _RUNS[k]


@pytest.mark.parametrize("k", range(len(pc.GOLDEN)))
def test_module_against_the_reference(golden_dir, report, k):
    z = np.load(os.path.join(golden_dir, "pwclite.npz"))
    c = pc.GOLDEN[k]
    net, x, m, res = native_run(k)
    e32, amax = z[f"e32_{k}"], z[f"amax_{k}"]
    items = [(f"out_{k}_{key}", t, pc.OUT_BUDGET, 7) for key, t in pc.output_items(res)]
    items += [(f"dmask_{k}_{i}", t.grad, pc.MASK_BUDGET, 7) for i, t in enumerate(m)]
    items += [(f"dparam_{k}_{j}", p.grad, pc.GRAD_BUDGET, 1) for j, (_, p) in enumerate(net.named_parameters())]
    assert len(items) == len(e32)
    assert [tuple(t.shape) for _, t in pc.output_items(res)[:5]] == [(c.B, 2, c.H >> i, c.W >> i) for i in range(5)]      # each level x 4
    worst = {"out": (0.0, ""), "dmask": (0.0, ""), "dparam": (0.0, "")}
    over = []
    for i, (key, t, budget, least) in enumerate(items):
        assert t is not None, key
        got = t.detach().reshape(-1)[pc.sample(t.numel(), budget, least)].double().cpu().numpy()
        want = z[key]
        bound = max(6 * e32[i], 16 * U * amax[i])
        err = float(np.abs(got - want).max())
        assert np.isfinite(got).all(), key
        kind = key.split("_")[0]
        if err / bound > worst[kind][0]:
            worst[kind] = (err / bound, key)
        if err > bound:
            over.append(f"{key}: error {err:.3e} = {err / bound:.2f} x the bound {bound:.3e} (6 e32 = {6 * e32[i]:.3e}, 16 ulp of the range = "
                        f"{16 * U * amax[i]:.3e}), {err / amax[i]:.1e} of the range")
    report(f"pwclite {c.name} ({c.B} x {c.H} x {c.W}, M = {c.M}): worst error / bound -- outputs {worst['out'][0]:.3f} ({worst['out'][1]}), "
           f"mask gradients {worst['dmask'][0]:.3f} ({worst['dmask'][1]}), parameter gradients {worst['dparam'][0]:.3f} ({worst['dparam'][1]}); "
           f"{len(over)} of {len(items)} tensors over their bound")
    for line in over:
        report("  " + line)
    assert not over, "\n".join(over)


def test_forward_is_bit_equal_and_with_bk_false_drops_the_backward_keys():
    net, x, m, res = native_run(0)
    with torch.no_grad():
        again = net(x, [t.detach() for t in m])
        fw = net(x, [t.detach() for t in m], with_bk=False)
    assert sorted(again) == sorted(res) == ["flows_bw", "flows_bw_all", "flows_bw_group", "flows_fw", "flows_fw_all", "flows_fw_group"]
    for (ka, a), (kb, b) in zip(pc.output_items(again), pc.output_items(res)):
        assert ka == kb and torch.equal(a, b), ka
    assert sorted(fw) == ["flows_fw", "flows_fw_all", "flows_fw_group"]
    for (ka, a), (kb, b) in zip(pc.output_items(fw), pc.output_items(res)):
        assert ka == kb and torch.equal(a, b), ka
    M = pc.GOLDEN[0].M
    assert len(res["flows_fw"]) == len(res["flows_fw_all"]) == 5 and len(res["flows_fw_group"]) == M + 1
    assert all(g.shape == res["flows_fw"][0].shape and g.stride()[2:] == (0, 0) for g in res["flows_fw_group"])      # expanded views
    assert float(res["flows_fw_group"][0].max()) == float(res["flows_fw_group"][0].min()) == -124.0


def test_gradients_reach_every_parameter_and_a_packed_weight_follows_its_parameter():
    net, x, m, res = native_run(0)
    assert all(p.grad is not None and p.grad.shape == p.shape and float(p.grad.abs().max()) > 0 for p in net.parameters())
    assert all(t.grad is not None and float(t.grad.abs().max()) > 0 for t in m)
    c1 = net.flow_estimators.conv1[0]
    before = c1.packed()[0]
    with torch.no_grad():
        c1.weight.mul_(1.0)                                   # a new version of the same values
    assert c1.packed()[0] is not before and torch.equal(c1.packed()[0], before)
