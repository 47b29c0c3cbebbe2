"""The flow head + loss tail (csrc/flowhead.hip, flow_head.py) against the oracle's float64 run at the edge shapes of
tests/flowhead_cases.py: every loss term, the flow maps and masks, dlogits (and its pad channels), dres at the residual's
own resolution and all eight parameter gradients; limit per quantity max(floor, 4 x the oracle's own float32 error),
floors 1e-5 (losses) / 2e-4 (tensors) / 2e-3 (tensors under the robust loss) as in tests/test_flowhead_gpu.py.
tests/test_flowhead_sweep_cpu.py keeps that float32 error under a quarter of the floor, so the floor decides."""
import ctypes
import dataclasses

import numpy as np
import pytest
import torch

import flowhead_cases as fc
import rcf_amd
from rcf_amd import _lib, ops
from rcf_amd.layers import Act

pytestmark = pytest.mark.gpu
DEV = "cuda:0"


def to_nhwc(x):
    return ops.nchw_to_nhwc(torch.from_numpy(np.ascontiguousarray(x)).to(DEV))


def hip_head(case, weights=None):
    head = rcf_amd.FlowAggregationHeadWithResidual(**fc.head_kwargs(case))
    weights = fc.state_dict(case) if weights is None else weights
    head.load_state_dict({k: torch.from_numpy(v) for k, v in weights.items()})
    return head.to(DEV)


def run_hip(case, head, inp):
    """one loss_and_grads + seed on fresh Acts and zeroed parameter gradients; everything back as CPU tensors"""
    model = fc.model_namespace(case, rcf_amd.CompactnessHead)
    logits, res = Act(to_nhwc(inp["logits"])), Act(to_nhwc(inp["res"]))
    for p in head.parameters():
        p.grad = None
    extra = {"pl_masks": torch.from_numpy(inp["pl"]).to(DEV), "crf_masks": torch.from_numpy(inp["crf"]).to(DEV)}
    losses, seed = head.loss_and_grads(model, logits, res, torch.from_numpy(inp["gfw"]).to(DEV),
                                       torch.from_numpy(inp["gbw"]).to(DEV), extra, case.B, 2, want_flows=True)
    # seed() takes its three gradient buffers (dlogits, dR at the mask's resolution, dfeat) with torch.empty: free blocks of
    # exactly those sizes full of NaN just before (the caching allocator hands a freed block of the same size back; best
    # effort, two of each), so that a pixel or pad channel the kernels leave unwritten shows instead of reading as a lucky 0
    n, h, w = logits.t.shape[:3]
    poison = [torch.full(shp, float("nan"), device=DEV) for shp in
              (tuple(logits.t.shape), (case.B, h, w, 4 * case.C), (n, h, w, 64)) * 2]
    del poison
    seed(case.scale)
    out = {"loss." + k: v.cpu() for k, v in losses.items()}
    out.update({"flow." + k: head.last_flows[k].cpu() for k in ("pred", "agg", "adj", "aff", "masks")})
    out["dlogits"] = ops.nhwc_to_nchw(logits.grad, case.C).cpu()
    out["dlogits_raw"] = logits.grad.cpu()                      # NHWC at the logits' pitch, pad channels included
    out["dres"] = ops.nhwc_to_nchw(res.grad).cpu()
    out.update({"d" + n: p.grad.cpu() for n, p in head.named_parameters()})
    return out


@pytest.mark.parametrize("case", fc.PARAMS_CASES)
def test_flow_head_sweep_vs_float64_oracle(case, report):
    truth, ref32 = fc.flatten(fc.cached_reference(case.name, True)), fc.ref32_errors(case)
    head, inp = hip_head(case), fc.make_inputs(case)
    out = run_hip(case, head, inp)
    again = run_hip(case, head, inp)
    assert {k for k in out if k.startswith("loss.")} == {k for k in truth if k.startswith("loss.")}
    assert {"d" + n for n in fc.PARAMS} <= set(out)
    err, lim = {}, {}
    for k, t in truth.items():
        got = out[k].numpy().reshape(np.shape(t))
        assert np.isfinite(got).all(), k
        err[k], lim[k] = fc.rel(got, t), max(fc.floor_of(case, k), 4 * ref32[k])
    Cp = out["dlogits_raw"].shape[3]
    pad = out["dlogits_raw"][..., case.C:]
    pad = (float("nan") if pad.isnan().any() else float(pad.abs().max())) if Cp > case.C else 0.0
    same = all(torch.equal(out[k], again[k]) for k in out)
    report(f"flow head sweep {case.name} (Cp {Cp}, err/limit): " + " ".join(f"{k} {err[k]:.2e}/{lim[k]:.0e}" for k in err)
           + f" | pad channels max {pad:.1e} | repeat bit-identical {same}")
    if case.C == 1:                                             # the float64 dlogits are identically zero: so are the kernel's
        assert not truth["dlogits"].any() and not out["dlogits"].any()
    assert pad == 0.0
    bad = {k: (err[k], lim[k]) for k in err if not err[k] < lim[k]}
    assert not bad, bad
    # fixed-order fp64 reductions, no float atomics (header of csrc/flowhead.hip): the same bits every time
    assert same, [k for k in out if not torch.equal(out[k], again[k])]


def test_flow_head_refuses_more_than_256_segment_sums():
    """B = 17, C = 8: 2 B C = 272 values for the one-block kernels of 256 threads; refused before anything is launched"""
    case = dataclasses.replace(fc.BY_NAME["block_limit"], B=17)
    head = hip_head(case)
    model = fc.model_namespace(case, rcf_amd.CompactnessHead)
    cfg = head._cfg(model, case.B, 8, [])
    assert _lib.load().rcf_flowhead_workspace_bytes(cfg) == 0
    with pytest.raises(_lib.RcfHipError):
        head._workspace(cfg, torch.device(DEV))
    logits = Act(torch.zeros((2 * case.B, case.h, case.w, 8), device=DEV))
    res = Act(torch.zeros((case.B, case.h, case.w, 32), device=DEV))
    z = torch.zeros((case.B, 1, 2, case.h, case.w), device=DEV)
    with pytest.raises(_lib.RcfHipError):
        head.loss_and_grads(model, logits, res, z, z, {}, case.B, 2)
    assert head._ws is None and logits.grad is None


def test_flow_head_zero_mass_segment_quadratic(report):
    """test_flow_head_zero_mass_segment_is_absent_not_nan at quad_kl's shape (D = 5, C = 5 -> pitch 8, non-2x resize): the last
    segment's logits at -1e4; loss and the live segments' dlogits equal the float64 oracle of the head WITHOUT that channel."""
    case = dataclasses.replace(fc.BY_NAME["quad_kl"], w_sharpen=0.0, w_seg=1.0)
    B, C, h, w = case.B, case.C, case.h, case.w
    inp = {k: v.copy() for k, v in fc.make_inputs(fc.BY_NAME["quad_kl"]).items()}
    inp["logits"].reshape(B, 2, C, h, w)[:, :, C - 1] = -1.0e4
    hr, wr = case.res_size
    sub = dataclasses.replace(case, C=C - 1)
    inp_sub = dict(inp, logits=np.ascontiguousarray(inp["logits"].reshape(B, 2, C, h, w)[:, :, :C - 1]).reshape(2 * B, C - 1, h, w),
                   res=np.ascontiguousarray(inp["res"].reshape(B, 2, 2, C, hr, wr)[:, :, :, :C - 1]).reshape(B, 4 * (C - 1), hr, wr))
    fc.move_ties(sub, inp_sub, fc.state_dict(case))             # the L1 ties of THIS prediction (gfw / gbw are shared with inp)
    out = run_hip(case, hip_head(case), inp)
    ref = fc.reference(sub, torch.float64, inp_sub, fc.state_dict(case))
    assert ref["tie"] > 0.9 * fc.TIE_MARGIN
    loss_dead, loss_ref = float(out["loss.loss_warp_seg"]), ref["losses"]["loss_warp_seg"]
    g_dead = out["dlogits"].numpy().reshape(B, 2, C, h, w)
    e_loss = abs(loss_dead - loss_ref) / abs(loss_ref)
    e_g = fc.rel(g_dead[:, :, :C - 1], ref["dlogits"].reshape(B, 2, C - 1, h, w))
    report(f"flow head quadratic, segment of zero mass: loss {loss_dead:.6f} vs the float64 oracle without that segment "
           f"{loss_ref:.6f} ({e_loss:.1e}); dlogits of the live segments {e_g:.1e}; dead segment's dlogits max "
           f"{np.abs(g_dead[:, :, C - 1]).max():.1e}; tie distance {ref['tie']:.1e}")
    assert np.isfinite(loss_dead) and np.isfinite(g_dead).all()
    assert e_loss < 1e-5 and e_g < 2e-4 and np.abs(g_dead[:, :, C - 1]).max() == 0.0


def lrelu_bwd(dy, y, dx, n, slope=0.1):
    return _lib.load().rcf_lrelu_bwd_f32(ctypes.c_void_p(dy.data_ptr()), ctypes.c_void_p(y.data_ptr()),
                                         ctypes.c_void_p(dx.data_ptr()), n, slope, ops._stream())


@pytest.mark.parametrize("n", [4 * 1021, 4194304 + 4 * 77], ids=["one_trip", "grid_stride"])
def test_lrelu_bwd_bit_exact(n, report):
    """rcf_lrelu_bwd_f32 against torch.where(y > 0, dy, slope * dy), bit for bit, out of place and in place (dx aliasing
    dy, as flow_head.py calls it); 4096 blocks x 256 threads x 4 floats = 4 194 304: above it the grid-stride loop runs"""
    g = torch.Generator().manual_seed(n)
    y, dy = torch.randn(n, generator=g), torch.randn(n, generator=g)
    y[::7], y[3::11] = 0.0, -0.0                                # y == 0 takes the slope, whatever its sign bit
    y[-1], y[-2], y[-5] = 0.0, -0.0, 1.0                        # the last float4
    dy[5::13] = -0.0
    y, dy = y.to(DEV), dy.to(DEV)
    slope = torch.tensor(0.1, dtype=torch.float32, device=DEV)
    want = torch.where(y > 0, dy, slope * dy)
    guard = 64
    buf = torch.full((n + guard,), 7.0, device=DEV)             # nothing is written past n
    assert lrelu_bwd(dy, y, buf, n) == 0
    inplace = dy.clone()
    assert lrelu_bwd(inplace, y, inplace, n) == 0
    torch.cuda.synchronize()
    bits = lambda t: t.view(torch.int32)
    ok_out, ok_in = torch.equal(bits(buf[:n]), bits(want)), torch.equal(bits(inplace), bits(want))
    report(f"lrelu_bwd n {n}: out of place bit-exact {ok_out}, in place bit-exact {ok_in}")
    assert ok_out and ok_in and bool((buf[n:] == 7.0).all())


def test_lrelu_bwd_refuses_n_not_multiple_of_4():
    t = torch.zeros(8, device=DEV)
    for n in (7, 0, -4):
        assert lrelu_bwd(t, t, t, n) == -1                       # RCF_EINVAL
    with pytest.raises(_lib.RcfHipError):
        _lib.call("rcf_lrelu_bwd_f32", ctypes.c_void_p(t.data_ptr()), ctypes.c_void_p(t.data_ptr()),
                  ctypes.c_void_p(t.data_ptr()), 6, 0.1, ops._stream())
