"""rcf_amd.AMDModel and the kernels of csrc/amd.hip on the GPU.

Kernels: per element against the float64 restatements of tests/amd_cases.py, under the bound stated beside each kernel (k 2^-24 mass;
softmax forward k = 3 on the mask value, backward k = 3 on |p_c| (|dp_c| + sum |p_k dp_k|), frame pair k = 19 on the blend of the
de-normalised absolute values), at shapes derived from rcf_amd_geometry.  Model: the flow side from the fixture's logits, the whole
training step through `.backward()` and through Trainer.step, and evaluation, against the reference's float64 run
(tests/golden/amd.npz) within max(1e-4, 4 x the reference's own float32 error) -- the criterion and the TOL of tests/test_model_gpu.py.
Measured numbers of a run: profiles/amd_parity.txt."""
import os
import types

import numpy as np
import pytest
import torch
import torch.nn as nn

import amd_cases as ac
import rcf_amd
import spatial_cases as sc
from rcf_amd import ops
from rcf_amd.layers import Act, Tape

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
TOL = 1e-4
PARITY = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "profiles", "amd_parity.txt")


@pytest.fixture(scope="module")
def golden(golden_dir):
    return np.load(os.path.join(golden_dir, "amd.npz"))


def _args(**kw):
    return types.SimpleNamespace(**dict(dict(checkpoints_dir="/tmp/rcf_amd_test", object_channel=None, eval_save=False, eval_export=False), **kw))


def _model(args=None):
    m = rcf_amd.AMDModel(args or _args(), **ac.model_kwargs())
    m.load_state_dict(ac.state_dict({k: tuple(v.shape) for k, v in m.state_dict().items()}))
    return m.to(DEV)


_NOTED = []


def _note(report, line):
    report(line)
    os.makedirs(os.path.dirname(PARITY), exist_ok=True)
    with open(PARITY, "a" if _NOTED else "w") as f:             # one run's numbers: the first line of a session starts the file
        f.write(line + "\n")
    _NOTED.append(line)


def lim(err):
    return max(TOL, 4 * float(err))


# ------------------------------------------------------------------------------------------------------------------ the kernels
@pytest.mark.parametrize("c", [pytest.param(c, id=c.name) for c in ac.softmax_cases()])
def test_mask_softmax_forward_and_backward(c):
    wide, dm = ac.softmax_inputs(c)
    dwide = wide.to(DEV)
    logits = dwide[..., :c.Cp]
    before = dwide.clone()
    masks = ops.mask_softmax(logits, c.B, c.I, c.M)
    assert tuple(masks.shape) == (c.I, c.B, c.M, c.h, c.w) and masks.is_contiguous() and masks[1].is_contiguous()
    assert torch.equal(torch.nan_to_num(dwide, 3.0), torch.nan_to_num(before, 3.0))        # the logits and their guard channels are left alone
    assert torch.equal(masks.cpu().view(torch.int32), ops.mask_softmax(logits, c.B, c.I, c.M).cpu().view(torch.int32))     # the same bits
    ref = ac.softmax_ref(wide[..., :c.Cp].double(), c.B, c.I, c.M)
    got = masks.cpu()
    # a NaN or +inf logit: NaN where torch's own float32 softmax gives NaN, and nowhere else
    t32 = torch.softmax(wide[..., :c.M].reshape(c.B, c.I, c.h, c.w, c.M), -1).permute(1, 0, 4, 2, 3)
    assert torch.equal(torch.isnan(got), torch.isnan(t32)) and torch.equal(torch.isnan(got), torch.isnan(ref))
    assert bool(torch.isnan(got).any()) == (c.kind == "naninf")
    ok = ~torch.isnan(ref)
    assert sc.elem_margin(got[ok], ref[ok], 3 * ac.U32 * ref[ok] + ac.DENORM) <= 1.0
    if c.kind == "naninf":
        assert float(got[1, 0, 2, 0, 5]) == 0.0 and int(torch.isnan(got).sum()) == 2 * c.M          # -inf gives 0; two pixels are NaN
    if c.kind == "equal":
        assert bool((got == got[0, 0, 0, 0, 0]).all()) and abs(float(got[0, 0, 0, 0, 0]) - 1.0 / c.M) <= ac.U32
    if c.M == 1:
        assert bool((got == 1).all())
    # backward, from the kernel's own float32 masks: exact arithmetic on the same inputs
    out = torch.full((c.I * c.B, c.h, c.w, c.pitch), 7.0, device=DEV)
    dl = ops.mask_softmax_bwd(masks, [None if d is None else d.to(DEV) for d in dm], c.Cp, out=out[..., :c.Cp])
    again = torch.full_like(out, 7.0)
    ops.mask_softmax_bwd(masks, [None if d is None else d.to(DEV) for d in dm], c.Cp, out=again[..., :c.Cp])
    assert torch.equal(out.cpu().view(torch.int32), again.cpu().view(torch.int32))
    o = out.cpu()
    assert bool((o[..., c.Cp:] == 7.0).all())                                     # beyond Cp: untouched
    guard = o[..., c.M:c.Cp]
    assert bool((guard == 0).all()) and not bool(torch.signbit(guard).any())      # the guard channels: written as 0
    want, mass = ac.softmax_bwd_ref(got.double(), [None if d is None else d.double() for d in dm])
    g = dl.cpu()[..., :c.M]
    assert torch.equal(torch.isnan(g), torch.isnan(want))
    ok = ~torch.isnan(want)
    assert sc.elem_margin(g[ok], want[ok], 3 * ac.U32 * mass[ok] + ac.DENORM) <= 1.0
    if c.absent is not None:
        n = torch.arange(c.I * c.B)
        assert float(g[n % c.I == c.absent].abs().max()) == 0
    if c.M == 1:
        assert float(g.abs().max()) == 0
    # a dense gradient tensor of the wrapper's own
    dense = ops.mask_softmax_bwd(masks, [None if d is None else d.to(DEV) for d in dm], c.Cp)
    assert tuple(dense.shape) == (c.I * c.B, c.h, c.w, c.Cp) and torch.equal(torch.nan_to_num(dense.cpu(), 3.0), torch.nan_to_num(o[..., :c.Cp], 3.0))


@pytest.mark.parametrize("c", [pytest.param(c, id=c.name) for c in ac.PAIRS])
def test_frame_pair(c):
    frames = ac.pair_inputs(c)
    got = ops.frame_pair(frames.to(DEV), (c.Ho, c.Wo))
    assert tuple(got.shape) == (c.B, 6, c.Ho, c.Wo)
    assert torch.equal(got.cpu().view(torch.int32), ops.frame_pair(frames.to(DEV), (c.Ho, c.Wo)).cpu().view(torch.int32))
    ref, mass = ac.frame_pair_ref(frames, (c.Ho, c.Wo))
    assert sc.elem_margin(got.cpu(), ref, ac.FRAME_PAIR_K * ac.U32 * mass) <= 1.0
    if (c.Hi, c.Wi) == (c.Ho, c.Wo):
        assert np.array_equal(got.cpu().numpy(), ac.denorm_f32(frames))           # the de-normalised input, exactly
    # the torch composition it replaces: de-normalise, then the planar resize kernel -- the same arithmetic, the same bits
    std = torch.tensor(ac.STD, device=DEV).view(1, 1, 3, 1, 1)
    mean = torch.tensor(ac.MEAN, device=DEV).view(1, 1, 3, 1, 1)
    f = frames.to(DEV)
    if c.name != "model":
        assert np.array_equal((f * std + mean).cpu().numpy().reshape(c.B, 6, c.Hi, c.Wi) / np.float32(255.0), ac.denorm_f32(frames))
    comp = ops.resize_nchw(torch.from_numpy(ac.denorm_f32(frames)).to(DEV), (c.Ho, c.Wo), align_corners=True)
    assert torch.equal(got, comp)


# -------------------------------------------------------------------------------------------------------------------- the model
@pytest.fixture(scope="module")
def stepped(golden):
    """ONE training step through `.backward()`, shared: (model, loss, logits NCHW, named gradients on the host)"""
    m = _model().train()
    loss = m(ac.batch(DEV))
    assert loss.dim() == 0 and loss.requires_grad
    logits = ops.nhwc_to_nchw(m.last_logits, ac.M).cpu().numpy()
    loss.backward()
    return m, float(loss.detach()), logits


def test_flow_side_from_the_fixtures_logits(golden, report, stepped):
    m = stepped[0]
    h, w = golden["truth_logits"].shape[-2:]
    lg = torch.from_numpy(golden["truth_logits"]).float().to(DEV)                 # rounded to float32, then NHWC
    act = Act(ops.nchw_to_nhwc(lg.contiguous(), 8))
    assert tuple(act.t.shape) == (ac.B * ac.I, h, w, 8)
    anchor = nn.Parameter(torch.zeros(1, device=DEV))                               # the bridge's parameter input: an empty tape has none
    imgs = torch.stack(ac.batch(DEV)["imgs"], dim=1)
    from rcf_amd.amd_model import _MaskBridge
    masks = _MaskBridge.apply(act, Tape(), ac.B, ac.I, ac.M, anchor)
    assert len(masks) == ac.I and all(tuple(t.shape) == (ac.B, ac.M, h, w) and t.is_contiguous() for t in masks)
    flows, flow_loss, bg, fg, groups = m.decode_head.flow_forward(imgs, list(masks), need_whole=False)
    assert flow_loss["whole"] == 0.0 and flows["whole"] == [] and len(flows["seg"]) == 1 and tuple(flows["seg"][0].shape) == (ac.B, 4, 384, 640)
    assert bg == [-1] and fg == [-1] and len(groups) == 1 and len(groups[0]) == ac.M + 1
    loss = flow_loss["seg"] * m.w_seg
    grads = torch.autograd.grad(loss, [anchor] + [p for p in m.decode_head.parameters()], allow_unused=True)
    assert float(anchor.detach()) == 0 and float(grads[0]) == 0 and all(g is not None and bool(torch.isfinite(g).all()) for g in grads)
    dl = ops.nhwc_to_nchw(act.grad, ac.M).cpu().numpy()
    assert float(act.grad[..., ac.M:].abs().max()) == 0
    e_loss, e_dl = ac.rel(float(loss), float(golden["truth_loss"])), ac.rel(dl, golden["truth_dlogits"])
    _note(report, f"amd flow side from fixture logits: loss {e_loss:.2e} (limit {lim(golden['ref32_err_loss']):.1e}) "
                  f"dlogits {e_dl:.2e} (limit {lim(golden['ref32_err_dlogits']):.1e})")
    assert e_loss < lim(golden["ref32_err_loss"]) and e_dl < lim(golden["ref32_err_dlogits"])
    # the five values with the whole-image flows, and the batch-major mask tensor: the reference's own call
    with torch.no_grad():
        bm = torch.stack([t.detach() for t in masks], 1)                          # [B, I, M, h, w]
        flows2, loss2, _, _, _ = m.decode_head.flow_forward(imgs, bm)
    assert torch.equal(loss2["seg"], flow_loss["seg"].detach()) and loss2["whole"].dim() == 0 and bool(torch.isfinite(loss2["whole"]))
    assert len(flows2["whole"]) == 1 and tuple(flows2["whole"][0].shape) == (ac.B, 4, 384, 640) and torch.equal(flows2["seg"][0], flows["seg"][0].detach())


def _grad_errors(golden, named):
    e_grad, l_grad = {}, {}
    for i, name in enumerate(golden["sampled"]):
        g = named[str(name)].grad.detach().cpu().contiguous().numpy().ravel()[:256]
        e_grad[str(name)] = ac.rel(g, golden[f"truth_grad_{i}"])
        l_grad[str(name)] = lim(golden["ref32_err_grad"][i])
    gn = ac.grad_norms(named.items())
    e_gn = {str(k): ac.rel(gn[str(k)], v) for k, v in zip(golden["gradnorm_keys"], golden["truth_gradnorm"])}
    l_gn = {str(k): lim(v) for k, v in zip(golden["gradnorm_keys"], golden["ref32_err_gradnorm"])}
    return e_grad, l_grad, e_gn, l_gn


def test_whole_step_vs_fixture(golden, report, stepped):
    m, loss, logits = stepped
    named = dict(m.named_parameters())
    assert all(p.grad is not None and bool(torch.isfinite(p.grad).all()) for p in named.values() if p.requires_grad)
    e_logits, e_loss = ac.rel(logits, golden["truth_logits"]), ac.rel(loss, float(golden["truth_loss"]))
    e_grad, l_grad, e_gn, l_gn = _grad_errors(golden, named)
    _note(report, f"amd whole step (.backward): logits vs f64 {e_logits:.2e} (limit {lim(golden['ref32_err_logits']):.1e}) loss {e_loss:.2e} "
                  f"(limit {lim(golden['ref32_err_loss']):.1e}) gradnorm {e_gn} (limits {l_gn}) grad {e_grad} (limits {l_grad})")
    assert e_logits < lim(golden["ref32_err_logits"]) and e_loss < lim(golden["ref32_err_loss"])
    assert all(e_gn[k] < l_gn[k] for k in e_gn), (e_gn, l_gn)
    assert all(e_grad[k] < l_grad[k] for k in e_grad), (e_grad, l_grad)
    assert m.train_iter == 2 and m._loss is not None
    with pytest.raises(RuntimeError):
        m.run_backward()                                                          # the graph of this step is spent


def test_trainer_step(golden, report):
    m = _model()
    tr = rcf_amd.Trainer(m, lr=1e-4, weight_decay=1e-6, device=DEV)
    ptrs = [p.grad.data_ptr() for p in tr.fp.params]
    # the gradients as the step leaves them in the flat buffer: read before Adam consumes nothing (Adam reads, it does not clear)
    out = tr.step(ac.batch(DEV))
    assert set(out) == {"loss"} and out["loss"].dim() == 0 and not out["loss"].requires_grad
    assert [p.grad.data_ptr() for p in tr.fp.params] == ptrs and all(p.grad is v for p, v in zip(tr.fp.params, tr.fp.grad_views))
    named = dict(m.named_parameters())
    e_loss = ac.rel(float(out["loss"]), float(golden["truth_loss"]))
    e_grad, l_grad, e_gn, l_gn = _grad_errors(golden, named)
    _note(report, f"amd Trainer.step: loss {e_loss:.2e} gradnorm {e_gn} (limits {l_gn}) grad {e_grad} (limits {l_grad})")
    assert e_loss < lim(golden["ref32_err_loss"])
    assert all(e_gn[k] < l_gn[k] for k in e_gn), (e_gn, l_gn)
    assert all(e_grad[k] < l_grad[k] for k in e_grad), (e_grad, l_grad)
    assert float(tr.fp.grad.abs().max()) > 0
    out2 = tr.step(ac.batch(DEV))
    assert bool(torch.isfinite(out2["loss"])) and tr.step_count == 2 and [p.grad.data_ptr() for p in tr.fp.params] == ptrs


def test_eval_masks_and_exports(golden, report, tmp_path):
    args = _args(checkpoints_dir=str(tmp_path), eval_save=True, eval_export=True, export_all_seg=False, object_channel=2)
    m = _model(args).eval()
    for d in (m.save_dir_eval, m.save_dir_eval_export):
        os.makedirs(d, exist_ok=True)
    masks = m(ac.batch(DEV))
    h, w = golden["truth_eval_masks0"].shape[-2:]
    assert tuple(masks.shape) == (ac.B, ac.M, h, w) and not masks.requires_grad
    err = float(np.abs(masks.cpu().numpy() - golden["truth_eval_masks0"]).max())
    _note(report, f"amd eval: masks of frame 0 vs f64 {err:.2e} (reference's float32 run {float(golden['ref32_err_eval_masks']):.2e})")
    assert err < TOL
    b = ac.batch()
    assert sorted(os.listdir(m.save_dir_eval)) == [f"eval_{b['seq_names'][0]}_0_00000_0000001.jpg"]
    assert sorted(os.listdir(m.save_dir_eval_export)) == sorted(f"pred_seg_{n}_{p.split('/')[-1][:-4]}_0000001.png" for n, p in zip(b["seq_names"], b["paths"][0]))
    args.export_all_seg = True
    for i in range(ac.M):
        os.makedirs(os.path.join(m.save_dir_eval_export, str(i)), exist_ok=True)
    pm, vis = m(ac.batch(DEV), return_pred_vis_list=True)
    assert torch.equal(pm, masks) and len(vis) == ac.M and tuple(vis[0].shape) == (ac.B, 3, 2 * h, 2 * w)
    assert all(len(os.listdir(os.path.join(m.save_dir_eval_export, str(i)))) == ac.B for i in range(ac.M))
