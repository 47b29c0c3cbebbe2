"""The host side of rcf_amd.AMDModel and of csrc/amd.hip, without a GPU: the model builds from config.amd_model_kwargs() and from the
reference's own settings file (tests/golden/amd.yaml) with the reference's state-dict names and shapes (tests/golden/amd.npz); the flow
head holds exactly `flownet.*`; RCFModel still refuses a flow network in its FCN heads; anything but float32 raises; the float64
restatements of the three kernels (tests/amd_cases.py) agree with torch's own float64 softmax + autograd and with the reference's
de-normalise-then-interpolate formula; the entry points are exported, bound, and refuse bad arguments before they touch a device."""
import copy
import ctypes
import os
import types

import numpy as np
import pytest
import torch
import torch.nn.functional as F

import amd_cases as ac
import rcf_amd
from rcf_amd import _lib, config


def _args():
    return types.SimpleNamespace(checkpoints_dir="/tmp/rcf_amd_test", object_channel=None, eval_save=False, eval_export=False)


@pytest.fixture(scope="module")
def golden(golden_dir):
    return np.load(os.path.join(golden_dir, "amd.npz"))


# ------------------------------------------------------------------------------------------------------------------ the model
def test_fixture_is_small_and_records_its_conditioning(golden, golden_dir):
    assert os.path.getsize(os.path.join(golden_dir, "amd.npz")) < 200 * 1024
    assert (int(golden["B"]), int(golden["H"]), int(golden["W"]), int(golden["M"]), int(golden["seed"])) == (ac.B, ac.H, ac.W, ac.M, ac.SEED)
    assert golden["truth_logits"].shape == golden["truth_dlogits"].shape == (ac.B * ac.I, ac.M, ac.H // 8, ac.W // 8)
    assert golden["truth_logits"].dtype == np.float64 and golden["truth_eval_masks0"].shape == (ac.B, ac.M, ac.H // 8, ac.W // 8)
    # the reference's own float32 run: its loss is within 1e-5 of the float64 run; its logit gradient is NOT (make_golden_amd.py: no
    # seed reaches that at 384 x 640, the flow network's LeakyReLUs always hold pre-activations that float32 decides either way) --
    # what it has is recorded, and the GPU tests' limits are 4 x that
    assert float(golden["ref32_err_loss"]) <= 1e-5 and 1e-5 < float(golden["ref32_err_dlogits"]) < 1e-2 and int(golden["kink_count"]) > 0
    print(f"amd fixture: reference float32 vs float64, logit gradient {float(golden['ref32_err_dlogits']):.1e}, "
          f"{int(golden['kink_count'])} pre-activations within MIN_KINK_DISTANCE (nearest {float(golden['kink_distance']):.1e})")
    assert [str(s) for s in golden["sampled"]] == ac.SAMPLED and sorted(str(k) for k in golden["gradnorm_keys"]) == ["backbone2", "decode_head", "decode_head2"]
    assert all(np.abs(golden[f"truth_grad_{i}"]).max() > 0 for i in range(len(ac.SAMPLED)))
    assert np.abs(golden["truth_eval_masks0"].sum(1) - 1).max() < 1e-12


def test_builds_from_kwargs_and_from_the_references_yaml(golden, golden_dir):
    cfg = config.load_yaml(os.path.join(golden_dir, "amd.yaml"))
    assert cfg["model_cls"] == "AMDModel" and cfg["model_kwargs"] == config.amd_model_kwargs()
    kw = config.amd_model_kwargs()
    assert kw["backbone2"]["dilations"] == [1, 1, 1, 2] and kw["backbone2"]["contract_dilation"] is False and kw["mask_layer"] == 5
    assert (kw["decode_head2"]["in_index"], kw["decode_head2"]["in_channels"]) == (3, 2048)
    want = list(zip((str(n) for n in golden["names"]), ac.unflat_shapes(golden["shapes"])))
    for kwargs in (config.amd_model_kwargs(), copy.deepcopy(cfg["model_kwargs"]), ac.model_kwargs()):
        m = rcf_amd.AMDModel(_args(), **kwargs)
        assert [(k, tuple(v.shape)) for k, v in m.state_dict().items()] == want
        assert {k.split(".")[0] for k, _ in want} == {"backbone2", "decode_head", "decode_head2"}
        assert all(k.startswith("decode_head.flownet.") for k, _ in want if k.startswith("decode_head."))
        assert (m.mask_layer, m.num_classes, m.w_seg, m.align_corners) == (5, 5, 1.0, False) and not hasattr(m, "grad_ready_hook")
    assert rcf_amd.model.REGISTRY["AMDModel"] is rcf_amd.AMDModel
    m.load_state_dict(ac.state_dict({k: s for k, s in want}))                # the seeded weights load, strictly
    assert m.train_iter == 1 and m.log_interval == 10 ** 9


def test_flow_head_holds_exactly_the_flow_network():
    kw = config.amd_model_kwargs()["decode_head"]
    kw.pop("type")
    head = rcf_amd.FCNHead(**kw)
    keys = list(head.state_dict())
    assert keys and all(k.startswith("flownet.") for k in keys)
    assert keys == ["flownet." + k for k in rcf_amd.PWCLite(5).state_dict()]
    assert isinstance(head.flownet, rcf_amd.PWCLite) and isinstance(head.loss_func, rcf_amd.unFlowLoss)
    assert not hasattr(head, "convs") and not hasattr(head, "conv_seg") and head.flow_size == (384, 640)
    c = head.loss_func.cfg                                                    # models/fcn_head.py:73-85
    assert (c.alpha, c.ssim_sz, c.occ_from_back, c.w_l1, c.w_ssim, c.w_ternary, c.w_real_smooth, c.warp_pad, c.with_bk) == \
        (10, 1, True, 0.15, 0.85, 0.0, 0.0, "border", True)
    assert c.w_scales == [1.0, 1.0, 1.0, 1.0, 0.0] and c.w_sm_scales == [1.0, 0.0, 0.0, 0.0, 0.0] and "alpha" in c.keys()
    assert all(p.requires_grad for p in head.parameters())
    frozen = rcf_amd.FCNHead(**dict(kw, freeze_flownet=True))
    assert not any(p.requires_grad for p in frozen.parameters())
    with pytest.raises(RuntimeError, match="flow_forward"):
        head.forward([torch.zeros(1, 2048, 3, 5)])
    with pytest.raises(RuntimeError, match="flow_forward"):
        head.fwd([None], None)
    plain = rcf_amd.FCNHead(2048, 256, num_classes=5, concat_input=False, norm_cfg=dict(type="BN"))
    with pytest.raises(RuntimeError, match="create_flownet=True"):
        plain.flow_forward(torch.zeros(1, 2, 3, 8, 8), torch.zeros(1, 2, 5, 2, 2))


def test_flow_head_loads_a_checkpoint(tmp_path):
    kw = config.amd_model_kwargs()["decode_head"]
    kw.pop("type")
    src = rcf_amd.PWCLite(5)
    path = str(tmp_path / "flownet.pth")
    torch.save({"state_dict": src.state_dict()}, path)
    head = rcf_amd.FCNHead(**dict(kw, load_flownet=True, flow_model_path=path))
    assert all(torch.equal(a, b) for a, b in zip(head.flownet.state_dict().values(), src.state_dict().values()))


def test_rcf_model_still_refuses_a_flow_network_in_its_fcn_heads():
    for name in ("decode_head2", "decode_head3"):
        kw = config.stage1_model_kwargs((24, 40))
        kw[name]["create_flownet"] = True
        with pytest.raises(NotImplementedError, match=name):
            rcf_amd.RCFModel(_args(), **kw)


def test_only_float32():
    m = rcf_amd.AMDModel(_args(), **ac.model_kwargs())
    b = ac.batch()
    for mode in (m.train, m.eval):
        mode()
        for prec in ("bf16", "fp16", "fp64"):
            m.precision = prec
            with pytest.raises(NotImplementedError, match="float32 only"):
                m(b)
        m.precision = None
        with torch.autocast("cpu", dtype=torch.bfloat16):
            with pytest.raises(NotImplementedError, match="float32 only"):
                m(b)
        with pytest.raises(RuntimeError, match="no CPU fallback"):
            m(b)
    with pytest.raises(RuntimeError, match="before forward"):
        m.run_backward()
    with pytest.raises(NotImplementedError, match="create_flownet=True"):
        kw = ac.model_kwargs()
        kw["decode_head"] = copy.deepcopy(kw["decode_head2"])
        rcf_amd.AMDModel(_args(), **kw)


# ------------------------------------------------------------------------------------------------------------ the restatements
@pytest.mark.parametrize("c", [pytest.param(c, id=c.name) for c in ac.softmax_cases() if c.kind != "naninf"])
def test_softmax_restatement_equals_torch(c):
    wide, dm = ac.softmax_inputs(c)
    x = wide[..., :c.M].double().requires_grad_(True)
    p = ac.softmax_ref(x, c.B, c.I, c.M)
    want = F.softmax(x.reshape(c.B, c.I, c.h, c.w, c.M), dim=-1).permute(1, 0, 4, 2, 3)
    assert float((p - want).detach().abs().max()) <= 1e-12 and float((p.detach().sum(2) - 1).abs().max()) <= 1e-12
    dmd = [None if d is None else d.double() for d in dm]
    sum((want[i] * d).sum() for i, d in enumerate(dmd) if d is not None).backward()
    dl, mass = ac.softmax_bwd_ref(p.detach(), dmd)
    assert float((dl - x.grad).abs().max()) <= 1e-12 * max(1.0, float(x.grad.abs().max()))
    assert bool((mass >= dl.abs() * (1 - 1e-12)).all())
    if c.absent is not None:
        n = torch.arange(c.I * c.B)
        assert float(dl[n % c.I == c.absent].abs().max()) == 0          # image n = b I + i: the absent frame's images get nothing
    if c.M == 1:
        assert bool((p == 1).all()) and float(dl.abs().max()) == 0


@pytest.mark.parametrize("Hi,Wi,Ho,Wo", ac.DYADIC)
def test_frame_pair_restatement_equals_the_references_formula(Hi, Wi, Ho, Wo):
    """de-normalise, then F.interpolate(align_corners=True), models/fcn_head.py:160-167.  torch's float64 run takes its sample positions
    in float64, the restatement (and the kernel, and torch's float32 run) in float32: the two coincide where (in - 1) / (out - 1) is
    dyadic, and there they agree to 1e-12"""
    frames = ac.pair_inputs(ac.Pair("cpu", 2, Hi, Wi, Ho, Wo)).double()
    got, mass = ac.frame_pair_ref(frames, (Ho, Wo))
    im = [torch.cat([frames[:, i, c:c + 1] * ac.STD[c] + ac.MEAN[c] for c in range(3)], 1) / 255.0 for i in range(2)]
    want = torch.cat([F.interpolate(t, size=(Ho, Wo), mode="bilinear", align_corners=True) for t in im], 1)
    assert float((got - want).abs().max()) <= 1e-12 and bool((mass >= got.abs() * (1 - 1e-12)).all())
    if (Hi, Wi) == (Ho, Wo):
        assert torch.equal(got, torch.cat(im, 1))


@pytest.mark.parametrize("c", [pytest.param(c, id=c.name) for c in ac.PAIRS if c.name != "model"])
def test_frame_pair_restatement_at_float32_positions(c):
    """any ratio: a float32 position of up to max(Hi, Wi) carries max(Hi, Wi) 2^-24 of error, times the largest difference of
    neighbouring de-normalised values"""
    frames = ac.pair_inputs(c).double()
    got, _ = ac.frame_pair_ref(frames, (c.Ho, c.Wo))
    v, _ = ac.denorm_ref(frames)
    want = F.interpolate(v, size=(c.Ho, c.Wo), mode="bilinear", align_corners=True)
    step = max(float(v.diff(dim=2).abs().max()) if c.Hi > 1 else 0.0, float(v.diff(dim=3).abs().max()) if c.Wi > 1 else 0.0)
    assert float((got - want).abs().max()) <= 2 * max(c.Hi, c.Wi) * 2 * ac.U32 * step + 1e-12
    assert np.abs(ac.denorm_f32(frames.float()) - v.numpy()).max() <= 3 * ac.U32 * float(v.abs().max()) * 2


def test_tables_reach_every_branch():
    pix, maxm, maxi = ac.geometry()
    assert pix > 0 and pix % 64 == 0 and maxm == 8 and maxi >= 2 and _lib.load().rcf_amd_geometry(3) == 0
    cs = ac.softmax_cases()
    px = [c.h * c.w for c in cs]
    assert 1 in px and pix - 1 in px and pix + 1 in px and any(p % 64 for p in px if p > 64)
    assert {1, 2, 5, 8} <= {c.M for c in cs} and {4, 8} == {c.Cp for c in cs} and any(c.pitch > c.Cp for c in cs)
    assert {(c.I, c.B) for c in cs} == {(2, 1), (2, 3)} and {0, 1, None} == {c.absent for c in cs}
    assert {"normal", "pm80", "equal", "naninf"} == {c.kind for c in cs}
    ps = {c.name: c for c in ac.PAIRS}
    assert (ps["identity"].Hi, ps["identity"].Wi) == (ps["identity"].Ho, ps["identity"].Wo)
    assert (ps["model"].Hi, ps["model"].Wi, ps["model"].Ho, ps["model"].Wo) == (96, 160, 384, 640)
    assert ps["up"].Ho % ps["up"].Hi and ps["down"].Hi % ps["down"].Ho and ps["one_row"].Hi == 1 and ps["one_column"].Wi == 1
    assert (ps["smallest_net"].Ho, ps["smallest_net"].Wo) == (64, 128) and {1, 3} == {c.B for c in ac.PAIRS}


# ---------------------------------------------------------------------------------------------------------------- host surface
def test_ops_refuse_host_tensors():
    lg = torch.zeros(2, 3, 4, 8)
    for call in (lambda: rcf_amd.ops.mask_softmax(lg, 1, 2, 5), lambda: rcf_amd.ops.mask_softmax_bwd(torch.zeros(2, 1, 5, 3, 4), [None, None], 8),
                 lambda: rcf_amd.ops.frame_pair(torch.zeros(1, 2, 3, 4, 4), (8, 8))):
        with pytest.raises(_lib.RcfHipError, match="no CPU"):
            call()


def test_entries_are_bound_and_refuse_before_touching_a_device():
    """sizes and ranges first (with every pointer NULL the status is the same), then pointers: nothing is launched -- there is no device
    here -- and the host buffer keeps its fill"""
    lib = _lib.load()
    for which in _lib.LIB_PATHS:
        assert not [n for n in _lib.missing_symbols(which) if n.startswith("rcf_amd_")]
    assert {"rcf_amd_geometry", "rcf_amd_mask_softmax_fwd_f32", "rcf_amd_mask_softmax_bwd_f32", "rcf_amd_frame_pair_f32"} <= set(_lib.PROTOS)
    pix, maxm, maxi = ac.geometry()
    buf = (ctypes.c_float * 64)(*([7.0] * 64))
    p = ctypes.cast(buf, ctypes.c_void_p)
    frames = (ctypes.c_void_p * 8)(*([p.value] * 8))
    fwd, bwd, pair = lib.rcf_amd_mask_softmax_fwd_f32, lib.rcf_amd_mask_softmax_bwd_f32, lib.rcf_amd_frame_pair_f32
    # (pitch, I, B, M, Cp, hw)
    bad = [(4, 0, 1, 1, 4, 8), (4, maxi + 1, 1, 1, 4, 8), (4, 2, 0, 1, 4, 8), (4, 2, -1, 1, 4, 8), (4, 2, 32768, 1, 4, 8), (4, 2, 1, 0, 4, 8),
           (8, 2, 1, maxm + 1, 8, 8), (4, 2, 1, 5, 4, 8), (4, 2, 1, 1, 4, 0), (4, 2, 1, 1, 4, -3), (4, 2, 1, 1, 4, 1 << 30), (8, 2, 1, 1, 6, 8),
           (12, 2, 1, 1, 12, 8), (4, 2, 1, 5, 8, 8), (6, 2, 1, 1, 4, 8), (16, 2, 1, 1, 0, 8)]
    for pitch, I, B, M, Cp, hw in bad:
        for ptr, fr in ((p, frames), (None, None)):
            assert fwd(ptr, pitch, ptr, I, B, M, Cp, hw, None) == -1, (pitch, I, B, M, Cp, hw)
            assert bwd(ptr, fr, ptr, pitch, I, B, M, Cp, hw, None) == -1, (pitch, I, B, M, Cp, hw)
    odd = ctypes.c_void_p(p.value + 4)                                  # not 16-byte aligned
    assert fwd(None, 8, p, 2, 1, 5, 8, 4, None) == -1 and fwd(p, 8, None, 2, 1, 5, 8, 4, None) == -1 and fwd(odd, 8, p, 2, 1, 5, 8, 4, None) == -1
    assert bwd(None, frames, p, 8, 2, 1, 5, 8, 4, None) == -1 and bwd(p, None, p, 8, 2, 1, 5, 8, 4, None) == -1
    assert bwd(p, frames, None, 8, 2, 1, 5, 8, 4, None) == -1 and bwd(p, frames, odd, 8, 2, 1, 5, 8, 4, None) == -1
    for B, Hi, Wi, Ho, Wo in ((0, 4, 4, 8, 8), (-1, 4, 4, 8, 8), (65536, 4, 4, 8, 8), (1, 0, 4, 8, 8), (1, 4, 0, 8, 8), (1, 4, 4, 0, 8), (1, 4, 4, 8, -2),
                              (1, (1 << 14) + 1, 4, 8, 8), (1, 4, 4, 8, (1 << 14) + 1)):
        for ptr in (p, None):
            assert pair(ptr, ptr, B, Hi, Wi, Ho, Wo, None) == -1, (B, Hi, Wi, Ho, Wo)
    assert pair(None, p, 1, 4, 4, 8, 8, None) == -1 and pair(p, None, 1, 4, 4, 8, 8, None) == -1
    assert list(buf) == [7.0] * 64
