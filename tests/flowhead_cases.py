"""Edge-shape cases of the flow head + loss tail (csrc/flowhead.hip) and their reference.

Shared by tests/test_flowhead_sweep_cpu.py (conditioning of every case: the oracle's own float32 error) and
tests/test_flowhead_sweep_gpu.py (the kernels against the float64 truth).  The reference is the ORACLE only
(oracle/rcf_torch.py, pinned to the reference by tests/test_oracle_cpu.py) with torch autograd, in the dtype asked for;
nothing of the HIP package enters it -- `rcf_amd.synth` (numpy only) draws the weights, as in the other tests.

What each case is for (kernel constants: NCHUNK = 64 pixel chunks per image, 64-pixel groups in bwd_pixel_kernel on a
fixed 512 x 4-wavefront grid, PARTW = 96 doubles per partial row, one-block kernels of 256 threads for 2*B*C values):
  tiny_single           P = 35 < NCHUNK (29 empty chunks that still write partials), C = 1 (pitch 4: three pad channels,
                        softmax == 1 so dlogits is identically 0), odd h and w
  cmax_entropy          C = 8 = CMAX (every register array full, pitch == C), P = 63 (one partial group), resize that is
                        not an exact 2x, entropy with an upstream scale
  row_linear            h = 1 (constant row index), P = 70 (one full + one partial group), residual without tanh
  affine_targets        D = 2, robust loss, B = 3, P = 1023 (odd), both target terms, C = 2 (two pad channels)
  quad_kl               D = 5, C = 5 (pitch 8: three pad channels), KL sharpen
  quad_partw            D = 5, C = 8: (2 + 2D) C = 96 = PARTW exactly, robust
  affine_hinge_compact  D = 2, C = 3, object-aware sharpen (hinge), compactness through the object channel
  block_limit           B = 16, C = 8: 2 B C = 256, the width of softmax_final_kernel / bwd_T_final_kernel
  p66_all_tails         P = 66, C = 4 (no pad), KL sharpen + compactness + both targets under an upstream scale (every
                        coefficient that rcf_flowhead_bwd_f32 multiplies by grad_scale)
  second_trip           P = 131 841 > 512*4*64: the outer loop of bwd_pixel_kernel takes its second trip (twelve full groups
                        and one single-pixel group)
  second_trip_affine    P = 131 709 > 131 072, D = 2, non-2x resize, w = 1021 (prime)
"""
import dataclasses
import functools
import types

import numpy as np
import pytest
import torch
import torch.nn.functional as F

import rcf_torch as orc
from rcf_amd import synth

FLOOR_LOSS, FLOOR_TENSOR, FLOOR_ROBUST = 1e-5, 2e-4, 2e-3     # tests/test_flowhead_gpu.py
PARAMS = ("flow_feat_before_agg.0.weight", "flow_feat_before_agg.0.bias", "flow_feat_before_agg.2.weight",
          "flow_feat_before_agg.2.bias", "flow_feat_after_agg.0.weight", "flow_feat_after_agg.0.bias",
          "flow_feat_after_agg.2.weight", "flow_feat_after_agg.2.bias")


@dataclasses.dataclass(frozen=True)
class Case:
    name: str
    B: int
    C: int
    h: int
    w: int
    mode: str = "free"                  # free | affine | quadratic
    robust: bool = False
    half_res: bool = False              # residual at ((h+1)//2, (w+1)//2)
    res_scale: float = 10.0             # residual_adjustment_scale; -1: the residual without tanh
    w_seg: float = 2.0
    w_entropy: float = 0.0
    w_sharpen: float = 0.0
    t_sharpen: float = 0.25
    object_aware: bool = False
    targets: bool = False               # pl (th 0.35, weight 3) + crf (th -1, weight 10), pos 2 / neg 1
    object_channel: object = None
    compact_channel: object = None      # None: no compactness head; -1: the object channel
    w_compactness: float = 0.0
    scale: float = 1.0                  # upstream gradient scale, seed(scale)
    seed: int = 0

    @property
    def res_size(self):
        return ((self.h + 1) // 2, (self.w + 1) // 2) if self.half_res else (self.h, self.w)

    @property
    def floor(self):
        return FLOOR_ROBUST if self.robust else FLOOR_TENSOR


CASES = [
    Case("tiny_single", 1, 1, 5, 7, w_seg=1.0, seed=101),
    Case("cmax_entropy", 2, 8, 7, 9, half_res=True, w_entropy=0.05, scale=0.5, seed=102),
    Case("row_linear", 1, 4, 1, 70, res_scale=-1.0, w_seg=1.0, seed=103),
    Case("affine_targets", 3, 2, 31, 33, mode="affine", robust=True, targets=True, object_channel=1, seed=104),
    Case("quad_kl", 2, 5, 13, 17, mode="quadratic", half_res=True, w_sharpen=0.1, seed=105),
    Case("quad_partw", 1, 8, 9, 11, mode="quadratic", robust=True, half_res=True, w_seg=1.0, seed=106),
    Case("affine_hinge_compact", 2, 3, 15, 27, mode="affine", half_res=True, w_sharpen=0.1, object_aware=True,
         object_channel=1, compact_channel=-1, w_compactness=0.5, seed=107),
    Case("block_limit", 16, 8, 6, 10, compact_channel=0, w_compactness=0.5, w_seg=1.0, seed=108),
    Case("p66_all_tails", 1, 4, 6, 11, w_sharpen=0.1, targets=True, object_channel=3, compact_channel=2,
         w_compactness=0.5, scale=0.5, seed=109),
    Case("second_trip", 1, 2, 257, 513, w_entropy=0.05, seed=110),
    # seed 211, not 111: of five draws the one whose float32 resize leaves flow.adj furthest inside its cap (3.9e-5 of 5e-5)
    Case("second_trip_affine", 1, 3, 129, 1021, mode="affine", half_res=True, w_seg=1.0, seed=211),
]
BY_NAME = {c.name: c for c in CASES}
PARAMS_CASES = [pytest.param(c, id=c.name) for c in CASES]


def head_kwargs(case):
    """constructor keywords shared by the oracle head and the HIP head (same signature)"""
    return dict(args=None, create_flownet=True, mask_layer=case.C, mask_size=(case.h, case.w), clamp_flow_t=20.,
                free_residual=case.mode == "free", free_residual_with_affine=case.mode != "free",
                free_residual_with_affine_quadratic=case.mode == "quadratic", allow_residual_resize=True,
                outlier_robust_loss=case.robust, residual_adjustment_scale=case.res_scale)


def model_namespace(case, compactness_head_cls):
    """what loss_and_grads / the oracle's loss methods read of an RCFModel"""
    args = types.SimpleNamespace(object_channel=case.object_channel)
    comp = None if case.compact_channel is None else compactness_head_cls(args, case.compact_channel)
    return types.SimpleNamespace(
        w_seg=case.w_seg, w_entropy=case.w_entropy, w_pl=3.0 if case.targets else 0, pl_pos_weight=2.0,
        pl_neg_weight=1.0, pl_mask_pos_th=0.35, w_crf=10.0 if case.targets else 0, crf_pos_weight=2.0,
        crf_neg_weight=1.0, crf_mask_pos_th=-1.0, compactness_head=comp, w_compactness=case.w_compactness,
        w_sharpen=case.w_sharpen, t_sharpen=case.t_sharpen, object_aware_sharpening=case.object_aware, args=args)


def state_dict(case):
    head = orc.FlowAggregationHeadWithResidual(**head_kwargs(case))
    shapes = {k: tuple(v.shape) for k, v in head.state_dict().items()}
    return synth.fill_state_dict(shapes, seed=case.seed)


TIE_MARGIN = 5e-3


def _oracle_pred(case, dtype, inputs, weights):
    """forward only: (clamped gt, predicted flow) as [B,4,h,w] (fw | bw), un-normalised"""
    B, C, h, w = case.B, case.C, case.h, case.w
    head = orc.FlowAggregationHeadWithResidual(**head_kwargs(case))
    head.load_state_dict({k: torch.from_numpy(v) for k, v in weights.items()})
    head = head.to(dtype)
    t = {k: torch.from_numpy(inputs[k]).to(dtype) for k in ("logits", "res", "gfw", "gbw")}
    with torch.no_grad():
        p = F.softmax(t["logits"].view(B, 2, C, h, w), dim=2)
        flows, _ = head(torch.zeros(B, 2, 3, 4, 4, dtype=dtype), p, t["gfw"], t["gbw"], t["res"][:, :2 * C], t["res"][:, 2 * C:])
    s = torch.tensor([h / 2.0, w / 2.0] * 2, dtype=dtype).view(1, 4, 1, 1)
    return (flows["gt_flow"][0] * s).numpy(), (flows["pred_flow"][0] * s).numpy()


@functools.lru_cache(maxsize=None)
def make_inputs(case):
    """float32 numpy inputs (shared: do not write into them): logits N(0, 2) [2B,C,h,w] (n = 2b + frame), residual N(0, 6)
    [B,4C,hr,wr] (fw | bw), flows N(0, 8) [B,1,2,h,w] (clamp_flow_t = 20 is hit, rarely), pl uniform, crf Bernoulli
    [B,2,h,w].

    The L1 (and robust) loss has a jump in its gradient where the predicted flow meets the ground truth.  float32 puts the
    prediction up to 5e-4 from the float64 one (measured: the bilinear resize 511 -> 1021 of the residual, whose source
    coordinates torch -- and the kernel, on purpose the same way -- computes in float32), so among 5e5 N(0, 10)
    differences a handful change sign between the two precisions and the oracle's OWN float32 dlogits are 0.23 of the
    maximum away from its float64 ones at those pixels.  Such a pixel measures nothing about a kernel.  So the few
    ground-truth values (4e-4 of them) within TIE_MARGIN of the float64 prediction are moved to 2 TIE_MARGIN on the side
    they were on; what that does to the prediction elsewhere (through the pooled features) is 1e-5, and
    tests/test_flowhead_sweep_cpu.py checks the margin on the final inputs."""
    g = np.random.Generator(np.random.PCG64(case.seed))
    B, C, h, w = case.B, case.C, case.h, case.w
    hr, wr = case.res_size
    inp = {"logits": g.normal(0, 2, size=(B * 2, C, h, w)).astype(np.float32),
           "res": g.normal(0, 6, size=(B, 4 * C, hr, wr)).astype(np.float32),
           "gfw": g.normal(0, 8, size=(B, 1, 2, h, w)).astype(np.float32),
           "gbw": g.normal(0, 8, size=(B, 1, 2, h, w)).astype(np.float32),
           "pl": g.random((B, 2, h, w)).astype(np.float32),
           "crf": (g.random((B, 2, h, w)) > 0.5).astype(np.float32)}
    move_ties(case, inp, state_dict(case))
    return inp


def move_ties(case, inp, weights):
    """in place: the ground-truth flows of `inp` within TIE_MARGIN of the float64 prediction go to 2 TIE_MARGIN from it"""
    gt, pred = _oracle_pred(case, torch.float64, inp, weights)
    diff = gt - pred
    tie = np.abs(diff) < TIE_MARGIN
    moved = np.where(diff >= 0, pred + 2 * TIE_MARGIN, pred - 2 * TIE_MARGIN).astype(np.float32)
    for key, sl in (("gfw", slice(0, 2)), ("gbw", slice(2, 4))):
        inp[key][:, 0][tie[:, sl]] = moved[:, sl][tie[:, sl]]


REF_THREADS = 8


class _fixed_threads:
    """torch's float32 sums over 1.3e5 pixels depend on how many threads share them: the bias gradient of the 64 -> 64 conv (a
    sum with heavy cancellation) is 1.6e-5 from float64 on 16 threads, 2.7e-5 on 8, 9.5e-5 on 3 and 6.8e-4 on one.  The
    reference is evaluated on REF_THREADS whatever the machine offers, so that its float32 error is one number."""

    def __enter__(self):
        self.n = torch.get_num_threads()
        torch.set_num_threads(REF_THREADS)

    def __exit__(self, *exc):
        torch.set_num_threads(self.n)


def reference(case, dtype, inputs=None, weights=None):
    with _fixed_threads():
        return _reference(case, dtype, inputs, weights)


def _reference(case, dtype, inputs, weights):
    """The oracle's losses, flow maps, masks and gradients of `case` in `dtype`; float64 numpy out.
    {"losses": {name: float}, "flows": {pred, agg, adj[, aff], masks}, "dlogits", "dres", "dparams": {name: array},
    "tie": min |clamped gt - predicted flow|}"""
    inputs = make_inputs(case) if inputs is None else inputs
    weights = state_dict(case) if weights is None else weights
    B, C, h, w = case.B, case.C, case.h, case.w
    head = orc.FlowAggregationHeadWithResidual(**head_kwargs(case))
    head.load_state_dict({k: torch.from_numpy(v) for k, v in weights.items()})
    head = head.to(dtype)
    m = model_namespace(case, orc.CompactnessHead)
    t = {k: torch.from_numpy(v).to(dtype) for k, v in inputs.items()}
    l, r = t["logits"].requires_grad_(True), t["res"].requires_grad_(True)
    p = F.softmax(l.view(B, 2, C, h, w), dim=2)
    logp = F.log_softmax(p, dim=2)                                          # double softmax, RCFModel.forward_train
    flows, lf = head(torch.zeros(B, 2, 3, 4, 4, dtype=dtype), p, t["gfw"], t["gbw"], r[:, :2 * C], r[:, 2 * C:])
    losses = {"loss_warp_seg": lf["seg"]}
    total = lf["seg"] * m.w_seg
    oc = case.object_channel
    if m.w_sharpen > 0 and (oc is not None or not m.object_aware_sharpening):
        ls = orc.RCFModel.get_sharpen_loss(m, p, logp, oc if m.object_aware_sharpening else None)
        losses["loss_sharpen"] = ls
        total = total + ls * m.w_sharpen
    elif m.w_entropy > 0:
        le = -(p * logp).sum(2).mean()
        losses["loss_entropy"] = le
        total = total + le * m.w_entropy
    if m.compactness_head is not None:
        lc = m.compactness_head.get_compactness_loss(p)
        if lc is not None:
            losses["loss_compactness"] = lc
            total = total + lc * m.w_compactness
    if m.w_pl > 0:
        pl = (torch.from_numpy(inputs["pl"]) > m.pl_mask_pos_th).to(dtype)   # thresholded on the float32 input itself
        lp = orc.RCFModel._asym_mse(pl, p[:, :, oc], m.pl_pos_weight, m.pl_neg_weight)
        losses["loss_pl"] = lp
        total = total + lp * m.w_pl
    if m.w_crf > 0:
        lcrf = orc.RCFModel._asym_mse(t["crf"], p[:, :, oc], m.crf_pos_weight, m.crf_neg_weight)
        losses["loss_crf"] = lcrf
        total = total + lcrf * m.w_crf
    losses["loss"] = total
    params = dict(head.named_parameters())
    grads = torch.autograd.grad(total * case.scale, [l, r] + [params[n] for n in PARAMS])
    s = torch.tensor([h / 2.0, w / 2.0], dtype=dtype).view(1, 1, 2, 1, 1)     # undo _vis_norm: [B,4,h,w] -> [2B,2,h,w]

    def planes(v):
        return ((v[0].detach().view(B, 2, 2, h, w) * s).reshape(2 * B, 2, h, w)).double().numpy()
    fl = {"pred": planes(flows["pred_flow"]), "agg": planes(flows["agg_flow"]), "adj": planes(flows["residual_adj"]),
          "masks": p.detach().reshape(2 * B, C, h, w).double().numpy()}
    if case.mode != "free":
        fl["aff"] = planes(flows["affine_flow"])
    return {"losses": {k: float(v.detach()) for k, v in losses.items()}, "flows": fl,
            "tie": float(np.abs(planes(flows["gt_flow"]) - fl["pred"]).min()),      # see make_inputs
            "dlogits": grads[0].double().numpy(), "dres": grads[1].double().numpy(),
            "dparams": {n: g.double().numpy() for n, g in zip(PARAMS, grads[2:])}}


@functools.lru_cache(maxsize=None)
def cached_reference(name, f64):
    """computed once per run and shared; callers must not write into it"""
    return reference(BY_NAME[name], torch.float64 if f64 else torch.float32)


def rel(a, b):
    a, b = np.asarray(a, dtype=np.float64), np.asarray(b, dtype=np.float64)
    return float(np.abs(a - b).max() / (np.abs(b).max() + 1e-30))


def flatten(ref):
    """one flat {quantity: value} view of a reference; loss terms under 'loss.<name>'"""
    out = {"loss." + k: v for k, v in ref["losses"].items()}
    out.update({"flow." + k: v for k, v in ref["flows"].items()})
    out["dlogits"], out["dres"] = ref["dlogits"], ref["dres"]
    out.update({"d" + k: v for k, v in ref["dparams"].items()})
    return out


def floor_of(case, key):
    return FLOOR_LOSS if key.startswith("loss.") else case.floor


def ref32_errors(case):
    """the oracle's own float32 error against its float64 run, per quantity"""
    t, s = flatten(cached_reference(case.name, True)), flatten(cached_reference(case.name, False))
    assert t.keys() == s.keys()
    return {k: rel(s[k], t[k]) for k in t}
