"""GPU: the device flow-colour kernel (csrc/flowvis.hip, ops.flow_color) against the float64 restatement of tests/flowvis_cases.py
under that file's rule, its strides, windows, output types and wrappers, and the training visualisation grids RCFModel and AMDModel
write with it.  The numbers of a run: profiles/flowvis_parity.txt."""
import copy
import os
import types

import numpy as np
import pytest
import torch

import flowvis_cases as fc
import rcf_amd
from rcf_amd import config, export, flowvis, ops, synth
from rcf_amd.model import SegModelBase

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
ONE_WG, TILE = ops.flow_color_geometry() if torch.cuda.is_available() else (4096, 1024)
SHAPES = fc.BASE_SHAPES + fc.geometry_shapes(ONE_WG)
_id = lambda s: f"{s[0]}x{s[1]}"


def _dev(a):
    return torch.from_numpy(np.ascontiguousarray(a)).to(DEV)


def _judge_all(got, levels, names, report, what):
    """got uint8 [N, 3, h, w] (host), levels [N, 3, h, w]: every image inside the rule; one report line"""
    vs = [fc.judge(g, lv) for g, lv in zip(got, levels)]
    report(f"{what}: " + " ".join(f"{n} {v.differing}/{got[0].size} (dist {v.worst_distance:.1e})" for n, v in zip(names, vs)) +
           f" | K {fc.K} EPS {fc.EPS:.2e} cap {fc.CAP:.0e}")
    for n, v in zip(names, vs):
        assert v.ok, (what, n, v)
    return vs


@pytest.mark.parametrize("shape", SHAPES, ids=_id)
def test_color_parity(shape, report):
    """every finite value kind at one shape, as ONE call of 7 images; integers (with both signed zeros), zeros and constants bit-equal"""
    flows, levels = fc.batch(*shape)
    got = ops.flow_color(_dev(flows)).cpu().numpy()
    assert got.dtype == np.uint8 and got.shape == levels.shape
    vs = _judge_all(got, levels, fc.FINITE_KINDS, report, f"flow_color {_id(shape)}")
    for kind, v in zip(fc.FINITE_KINDS, vs):
        if kind in fc.BIT_EQUAL_KINDS:
            assert v.differing == 0, (kind, v)
    # both launch forms, from the kernel's constants
    assert (shape[0] * shape[1] > ONE_WG) == (rcf_amd._lib.load().rcf_flow_color_workspace_bytes(7, 1, *shape) > 0)


@pytest.mark.parametrize("N,shape", [(1, (3, 5)), (2, (3, 5)), (20, (3, 5)), (20, (48, 48)), (2, SHAPES[-2]), (20, SHAPES[-2])],
                         ids=lambda v: _id(v) if isinstance(v, tuple) else str(v))
def test_batch_sizes(N, shape, report):
    """each image by its OWN maximum, whatever the number of images (both launch forms)"""
    pairs = [fc.batch(*shape, kinds=("normal",), seed=i) for i in range(N)]
    flows = np.concatenate([p[0] for p in pairs]) * np.arange(1, N + 1, dtype=np.float32).reshape(N, 1, 1, 1)
    levels = np.stack([fc.color_levels(f) for f in flows])                 # (scaled per image: the maxima differ by up to 20 x)
    got = ops.flow_color(_dev(flows)).cpu().numpy()
    _judge_all(got, levels, [str(i) for i in range(N)], report, f"flow_color N={N} {_id(shape)}")


@pytest.mark.parametrize("shape", [(48, 48), SHAPES[-1]], ids=_id)
def test_non_finite_image_is_covered_repeatable_and_alone(shape, report):
    h, w = shape
    flows = np.stack([fc.draw("normal", h, w, seed=s) for s in range(4)])
    levels = [fc.color_levels(f) for f in flows]
    bad = flows[1].reshape(2, -1)
    bad[0, 1], bad[1, (h * w) // 2], bad[0, h * w - 1] = np.nan, np.inf, 3e38
    outs = []
    for _ in range(2):
        out = torch.full((4, 3, h, w), -1.0, device=DEV)
        ops.flow_color(_dev(flows), out=out)
        outs.append(out)
    assert torch.equal(outs[0], outs[1])
    o = outs[0].cpu().numpy()
    assert ((o >= 0) & (o <= 1)).all()                                   # every element of the poisoned window written, with a level
    got = np.rint(o * 255).astype(np.uint8)
    keep = [0, 2, 3]
    _judge_all(got[keep], [levels[i] for i in keep], [str(i) for i in keep], report, f"flow_color beside a non-finite image {_id(shape)}")


@pytest.mark.parametrize("shape", [(3, 5), (48, 48), SHAPES[-2]], ids=_id)
def test_channel_slices_hw2_input_and_canvas_window(shape, report):
    h, w = shape
    B = 3
    f4 = np.concatenate([np.stack([fc.draw("normal", h, w, seed=10 + b) for b in range(B)]),
                         np.stack([fc.draw("normal", h, w, seed=20 + b) for b in range(B)])], 1)          # [B, 4, h, w]
    t4 = _dev(f4)
    for name, sl in (("[:, :2]", slice(0, 2)), ("[:, 2:]", slice(2, 4))):
        view = t4[:, sl]
        assert not view.is_contiguous() or B == 1
        got = ops.flow_color(view).cpu().numpy()
        _judge_all(got, [fc.color_levels(np.ascontiguousarray(f)) for f in f4[:, sl]], [str(b) for b in range(B)], report,
                   f"flow_color {name} {_id(shape)}")
    # a window in the middle of a canvas (odd offsets: the scalar store path; offsets of 4: the vector one), sentinel intact around it
    for y0, x0 in ((1, 3), (4, 4)):
        for dtype, sentinel in ((torch.uint8, 77), (torch.float32, -3.0)):
            canvas = torch.full((B, 3, h + 6, (w + 12) // 4 * 4), sentinel, dtype=dtype, device=DEV)     # rows a multiple of 4 wide
            win = canvas[:, :, y0:y0 + h, x0:x0 + w]
            assert ops.flow_color(t4[:, 2:], out=win) is win
            ref = ops.flow_color(t4[:, 2:].contiguous(), out_dtype=dtype)
            assert torch.equal(win, ref)
            mask = torch.ones_like(canvas, dtype=torch.bool)
            mask[:, :, y0:y0 + h, x0:x0 + w] = False
            assert (canvas[mask] == sentinel).all()
    # [h, w, 2] in place, [h, w, 3] out: flow_to_color on a tensor and on numpy
    hw2 = np.ascontiguousarray(f4[0, :2].transpose(1, 2, 0))
    lv = fc.color_levels(np.ascontiguousarray(f4[0, :2]))
    on_dev = flowvis.flow_to_color(_dev(hw2))
    assert on_dev.is_cuda and on_dev.dtype == torch.uint8 and tuple(on_dev.shape) == (h, w, 3)
    on_host = flowvis.flow_to_color(hw2)
    assert isinstance(on_host, np.ndarray) and on_host.dtype == np.uint8 and (on_host == on_dev.cpu().numpy()).all()
    _judge_all([on_host.transpose(2, 0, 1)], [lv], ["hw2"], report, f"flow_to_color {_id(shape)}")
    bgr = flowvis.flow_to_color(hw2, convert_to_bgr=True)
    assert (bgr[..., ::-1] == on_host).all()
    clipped = flowvis.flow_to_color(hw2, clip_flow=1.5)
    _judge_all([clipped.transpose(2, 0, 1)], [fc.color_levels(np.ascontiguousarray(f4[0, :2]), clip=1.5)], ["clip"], report,
               f"flow_to_color clip {_id(shape)}")


def test_float32_output_is_byte_over_255_and_grouped_layout():
    flows, _ = fc.batch(48, 48)
    t = _dev(flows)
    u8 = ops.flow_color(t)
    f32 = ops.flow_color(t, out_dtype=torch.float32)
    # byte / 255 as ONE IEEE division (numpy; torch's device division by a Python scalar multiplies by a rounded 1 / 255 instead)
    assert f32.dtype == torch.float32 and (f32.cpu().numpy() == u8.cpu().numpy().astype(np.float32) / np.float32(255.0)).all()
    assert torch.equal(ops.flow_color(t[0]), u8[0]) and torch.equal(ops.flow_color(t, convert_to_bgr=True), u8.flip(1))
    # [G, K, 2, h, w] into a [G, 3, K, h, w]-ordered canvas: the grid's flow strip
    G, K = 2, 3
    canvas = torch.full((G, 3, K + 2, 48, 48), -1.0, device=DEV)
    ops.flow_color(t[:G * K].view(G, K, 2, 48, 48), out=canvas[:, :, 1:1 + K].permute(0, 2, 1, 3, 4))
    assert torch.equal(canvas[:, :, 1:1 + K].permute(0, 2, 1, 3, 4).reshape(G * K, 3, 48, 48), f32[:G * K])
    assert (canvas[:, :, 0] == -1).all() and (canvas[:, :, K + 1] == -1).all()
    for bad in (t.double(), t.cpu(), t[:, :1], t[None, None]):
        with pytest.raises(rcf_amd._lib.RcfHipError):
            ops.flow_color(bad)
    with pytest.raises(rcf_amd._lib.RcfHipError):
        ops.flow_color(t, out=torch.empty((7, 3, 48, 47), dtype=torch.uint8, device=DEV))


@pytest.mark.parametrize("setmax", [False, True])
def test_let_tensor_vis(setmax, report):
    flow = 0.05 * fc.draw("normal", 16, 24, seed=3)[None]                 # (|flow| < 0.2 nearly everywhere; clipped below for setmax)
    flow = np.clip(flow, -0.19, 0.19).astype(np.float32)
    t = _dev(flow)
    keep = t.clone()
    out = SegModelBase().let_tensor_vis(t, setmax=setmax)
    assert torch.equal(t, keep)                                           # works on a clone
    assert out.dtype == torch.float32 and tuple(out.shape) == (1, 3, 16, 24) and out.is_cuda
    want = flow[0].copy()
    if setmax:
        want[:, 0, 0] = 0.2
    got = out[0].cpu().numpy()
    assert (got == np.rint(got)).all() and got.min() >= 0 and got.max() <= 255
    _judge_all([got.astype(np.uint8)], [fc.color_levels(want)], ["vis"], report, f"let_tensor_vis setmax={setmax}")
    if setmax:
        with pytest.raises(AssertionError):
            SegModelBase().let_tensor_vis(_dev(np.full((1, 2, 4, 4), 0.5, dtype=np.float32)), setmax=True)


# ------------------------------------------------------------------------------------------------------------------- the models
H, W, B = 64, 96, 2
SAMPLED = ["backbone2.conv1.weight", "backbone2.layer2.1.conv2.weight", "backbone2.layer4.0.downsample.0.weight",
           "decode_head2.conv_seg.bias", "decode_head3.convs.0.conv.weight", "decode_head.flow_feat_after_agg.2.weight"]


def _rcf_batch(pl):
    nb = synth.make_batch(B, H, W, config_id=1)
    out = {k: [_dev(a) for a in nb[k]] for k in ("imgs", "gt_fw_flows", "gt_bw_flows")}
    out.update(seq_ids=nb["seq_ids"], seq_names=nb["seq_names"], paths=nb["paths"])
    if pl:
        out["pl_masks"] = [_dev(a) for a in synth.make_pl_masks(B, H, W, config_id=1)]
    return out


def _rcf_model(ckpt, affine, pl, **args_kw):
    kw = config.stage1_model_kwargs(config.mask_size_for(H, W), dropout=0.0, affine=affine, norm="BN")
    if pl:
        kw.update(w_pl=2.0, pl_pos_weight=2.0, pl_neg_weight=1.0)
    kw.update(log_interval=1, train_iter=0)
    args = types.SimpleNamespace(checkpoints_dir=str(ckpt), object_channel=1 if pl else None, eval_save=False, eval_export=False,
                                 **args_kw)
    m = rcf_amd.RCFModel(args, **copy.deepcopy(kw))
    shapes = {k: tuple(v.shape) for k, v in m.state_dict().items()}
    m.load_state_dict({k: torch.from_numpy(v) for k, v in synth.fill_state_dict(shapes, seed=7).items()})
    return m.to(DEV)


def _step(model, batch):
    losses = rcf_amd.Trainer(model, device=DEV).step(batch)
    torch.cuda.synchronize()
    named = dict(model.named_parameters())
    return {k: float(v) for k, v in losses.items()}, {n: named[n].grad.detach().clone() for n in SAMPLED if n in named}


def _files(d):
    return sorted(os.listdir(d)) if os.path.isdir(d) else None


def _expected_name(batch, it=0):
    frame = batch["paths"][0][0].split("/")[-1][:-4]
    sid = batch["seq_ids"][0]
    sid = sid.item() if torch.is_tensor(sid) else sid
    return f"train_iter{it:07d}_{batch['seq_names'][0]}_{sid}_{frame}_img_pred_recons.jpg"


def _check_flow_panels(grid, panels, flows_by_kind, report, what):
    """grid [2 B, 3, P h, w] (host); flows_by_kind: name -> [B, 4, h, w] normalised flows (host), frame 0 = channels :2"""
    h = grid.shape[2] // len(panels)
    for kind, f4 in flows_by_kind.items():
        p = panels.index("flow_" + kind)
        for i in range(2):
            got = np.rint(grid[i * B:(i + 1) * B, :, p * h:(p + 1) * h] * 255.0)
            assert np.abs(got / 255.0 - grid[i * B:(i + 1) * B, :, p * h:(p + 1) * h]).max() < 1e-7
            lv = [fc.color_levels(np.ascontiguousarray(f4[b, 2 * i:2 * i + 2])) for b in range(B)]
            _judge_all(got.astype(np.uint8), lv, [f"b{b}" for b in range(B)], report, f"{what} flow_{kind} frame {i}")


@pytest.mark.parametrize("affine,pl", [(False, False), (True, False), (False, True)], ids=["plain", "affine", "pl"])
def test_rcf_logged_step_writes_the_grid_and_leaves_the_step_alone(affine, pl, tmp_path, report):
    batch = _rcf_batch(pl)
    os.makedirs(tmp_path / "a" / "saved")
    os.makedirs(tmp_path / "b" / "saved")
    m = _rcf_model(tmp_path / "a", affine, pl)
    losses, grads = _step(m, batch)
    assert _files(tmp_path / "a" / "saved") == [_expected_name(batch)]
    assert m.train_iter == 1
    # the same step with train_save=False: nothing written, the same bits
    m2 = _rcf_model(tmp_path / "b", affine, pl, train_save=False)
    losses2, grads2 = _step(m2, batch)
    assert _files(tmp_path / "b" / "saved") == [] and _files(tmp_path / "b" / "saved_train_export") is None
    assert losses == losses2 and grads and all(torch.equal(grads[n], grads2[n]) for n in grads), (losses, losses2)
    # the .pth dump of log_interval == 1
    frame = batch["paths"][0][0].split("/")[-1][:-4]
    dump = tmp_path / "a" / "saved_train_export" / f"{batch['seq_names'][0]}_{frame}.pth"
    assert _files(tmp_path / "a" / "saved_train_export") == [dump.name]
    saved = torch.load(dump, map_location="cpu", weights_only=False)
    assert len(saved) == 8 and (saved[6] is not None) == pl
    tosave = saved[7]
    assert torch.equal(tosave, m.last_train_grid.cpu())
    # the grid rebuilt from the head's flows, the masks and the frames
    head, (h, w), M = m.decode_head, m.mask_size, m.mask_layer
    f = head.last_flows
    kinds = ("pred", "gt", "agg", "aff", "adj") if affine else ("pred", "gt", "agg", "adj")
    panels = flowvis.grid_panels(M, kinds, pl)
    assert tuple(tosave.shape) == (2 * B, 3, len(panels) * h, w)
    s = torch.tensor([h / 2.0, w / 2.0], device=DEV).view(1, 1, 2, 1, 1)
    vis = {k: (f[k].view(B, 2, 2, h, w) / s).reshape(B, 4, h, w) for k in kinds}            # FlowAggregationHead.forward's vis()
    _check_flow_panels(tosave.numpy(), panels, {k: v.cpu().numpy() for k, v in vis.items()}, report, f"RCF grid {affine=} {pl=}")
    imgs = torch.stack(batch["imgs"], 1)
    masks = f["masks"].view(B, 2, M, h, w).transpose(0, 1)
    frames = torch.stack([(m.resize(imgs[:, i], (h, w)) + 2.0) / 4.0 for i in range(2)])
    colours = [torch.stack([ops.flow_color(v[:, 2 * i:2 * i + 2], out_dtype=torch.float32) for i in range(2)]) for v in vis.values()]
    pl_t = m.last_targets["pl_masks"].transpose(0, 1) if pl else None
    rebuilt = flowvis.assemble_grid(masks, frames, colours, pl_t)
    assert torch.equal(rebuilt.cpu(), tosave)
    export.save_image(rebuilt, str(tmp_path / "rebuilt.jpg"))
    assert open(tmp_path / "rebuilt.jpg", "rb").read() == open(tmp_path / "a" / "saved" / _expected_name(batch), "rb").read()


def test_rcf_without_saved_dir_or_paths_writes_nothing(tmp_path):
    batch = _rcf_batch(False)
    m = _rcf_model(tmp_path / "c", False, False)
    _step(m, batch)
    assert _files(tmp_path / "c") is None and not hasattr(m, "last_train_grid")
    os.makedirs(tmp_path / "d" / "saved")
    m = _rcf_model(tmp_path / "d", False, False)
    _step(m, {k: v for k, v in batch.items() if k != "paths"})
    assert _files(tmp_path / "d") == ["saved"] and _files(tmp_path / "d" / "saved") == []


def test_amd_logged_step_writes_the_grid_and_leaves_the_step_alone(tmp_path, report):
    import amd_cases as ac

    def model(ckpt, **args_kw):
        kw = ac.model_kwargs()
        kw.update(log_interval=1, train_iter=0)
        args = types.SimpleNamespace(checkpoints_dir=str(ckpt), object_channel=None, eval_save=False, eval_export=False, **args_kw)
        m = rcf_amd.AMDModel(args, **kw)
        m.load_state_dict(ac.state_dict({k: tuple(v.shape) for k, v in m.state_dict().items()}))
        return m.to(DEV).train()

    def step(m):
        loss = m(batch)
        loss.backward()
        torch.cuda.synchronize()
        return float(loss.detach()), {n: p.grad.detach().clone() for n, p in m.named_parameters() if p.grad is not None}

    batch = ac.batch(DEV)
    os.makedirs(tmp_path / "a" / "saved")
    os.makedirs(tmp_path / "b" / "saved")
    m = model(tmp_path / "a")
    loss, grads = step(m)
    assert _files(tmp_path / "a" / "saved") == [_expected_name(batch)] and _files(tmp_path / "a" / "saved_train_export") is None
    m2 = model(tmp_path / "b", train_save=False)
    loss2, grads2 = step(m2)
    assert _files(tmp_path / "b" / "saved") == [] and not hasattr(m2, "last_train_grid")
    # The loss and every gradient that is a fixed-order function of the step: the same bits.  The 20 gradients of the flow network's
    # feature pyramid are sums of float atomics (the warp's backward scatters into the feature maps, csrc/warp.hip) and differ between
    # ANY two runs of the same step, logged or not -- measured on an MI355X, two unlogged steps: 20 of 215 tensors, at most 4.8e-7 of
    # the tensor's largest element; unlogged against logged: the same 20, at most 3.7e-7.  They are held to 64 x 2^-24 of it.
    loose = "decode_head.flownet.feature_pyramid_extractor."
    exact = [n for n in grads if not n.startswith(loose)]
    assert loss == loss2 and set(grads) == set(grads2) and len(exact) >= 190 and set(ac.SAMPLED) - set(exact) <= {ac.SAMPLED[6]}
    assert not [n for n in exact if not torch.equal(grads[n], grads2[n])]
    worst = max(float((grads[n] - grads2[n]).abs().max() / grads2[n].abs().max()) for n in grads if n.startswith(loose))
    report(f"AMD logged vs unlogged step: loss and {len(exact)} gradients bit-equal; {len(grads) - len(exact)} feature-pyramid gradients "
           f"(float atomics in the warp's backward) within {worst:.1e}")
    assert worst < 64 * 2.0 ** -24
    # the grid rebuilt: masks and flows recomputed from the step's logits (every kernel on the way gives the same bits on every call)
    tosave = m.last_train_grid
    imgs = torch.stack(batch["imgs"], 1)
    with torch.no_grad():
        masks = ops.mask_softmax(m.last_logits, ac.B, 2, ac.M)
        h, w = masks.shape[-2:]
        flows, _, _, _, _ = m.decode_head.flow_forward(imgs, list(masks), need_whole=True)
        vis = {k: m.resize(flows[k][0], (h, w)) for k in ("seg", "whole")}
        frames = torch.stack([(m.resize(imgs[:, i], (h, w)) + 2.0) / 4.0 for i in range(2)])
        colours = [torch.stack([ops.flow_color(v[:, 2 * i:2 * i + 2], out_dtype=torch.float32) for i in range(2)]) for v in vis.values()]
    panels = flowvis.grid_panels(ac.M, ("seg", "whole"))
    assert tuple(tosave.shape) == (2 * ac.B, 3, len(panels) * h, w)
    _check_flow_panels(tosave.cpu().numpy(), panels, {k: v.cpu().numpy() for k, v in vis.items()}, report, "AMD grid")
    rebuilt = flowvis.assemble_grid(masks, frames, colours)
    assert torch.equal(rebuilt, tosave)
    export.save_image(rebuilt, str(tmp_path / "rebuilt.jpg"))
    assert open(tmp_path / "rebuilt.jpg", "rb").read() == open(tmp_path / "a" / "saved" / _expected_name(batch), "rb").read()
