"""CPU: the flow-colour restatement against hand-checked points, its float32 form against float64 under the rule of
tests/flowvis_cases.py, the new entry point's ABI, flow_to_color's asserts, and the layout of the training grid on the host helper."""
import numpy as np
import pytest
import torch

import flowvis_cases as fc
import rcf_amd
from rcf_amd import _lib, flowvis


def _bytes(flow, **kw):
    return fc.to_bytes(fc.color_levels(np.asarray(flow, dtype=np.float32), **kw))


def test_wheel_rows_and_ry_segment():
    w = fc.wheel()
    assert w.shape == (55, 3) and sum(n for _, n in fc.SEGMENTS) == 55
    assert w[0].tolist() == [255, 0, 0]
    assert w[:15, 0].tolist() == [255] * 15 and w[:15, 2].tolist() == [0] * 15
    assert w[:15, 1].tolist() == [0, 17, 34, 51, 68, 85, 102, 119, 136, 153, 170, 187, 204, 221, 238]
    # the segment starts: yellow, green, cyan, blue, magenta
    assert [w[i].tolist() for i in (15, 21, 25, 36, 49)] == [[255, 255, 0], [0, 255, 0], [0, 255, 255], [0, 0, 255], [255, 0, 255]]
    assert w[54].tolist() == [255, 0, 43]


def test_zero_flow_is_white():
    assert (_bytes(np.zeros((2, 3, 5))) == 255).all()


def test_signed_zeros_land_on_rows_0_and_54():
    """(1, +0): atan2(-0, -1) = -pi, fk = 0, row 0; (1, -0): atan2(+0, -1) = +pi, fk = 54, row 54 -- in an image whose maximum
    (radius 5) is elsewhere, so both have radius 1 / (5 + 1e-5) and col = 1 - rad (1 - wheel / 255)"""
    flow = np.zeros((2, 1, 3), dtype=np.float32)
    flow[:, 0, 0], flow[:, 0, 1], flow[:, 0, 2] = (1.0, 0.0), (1.0, -0.0), (3.0, -4.0)
    got = _bytes(flow)
    rad = 1.0 / (5.0 + 1e-5)
    for x, row in ((0, 0), (1, 54)):
        want = np.floor(255.0 * (1.0 - rad * (1.0 - fc.wheel()[row] / 255.0)))
        assert got[:, 0, x].tolist() == want.tolist(), (x, row)
    assert got[:, 0, 0].tolist() != got[:, 0, 1].tolist()
    assert (_bytes(flow, head=np.float32) == got).all()


def test_bgr_swaps_planes_and_clip_is_a_clamp_to_0_clip():
    flow = fc.draw("normal", 3, 5)
    b = _bytes(flow)
    assert (fc.planes(b, bgr=True)[0] == b[2]).all() and (fc.planes(b, bgr=True)[1] == b[1]).all()
    clipped = np.clip(flow, 0, 1.5)
    assert (_bytes(flow, clip=1.5) == _bytes(clipped)).all()
    assert (_bytes(flow, clip=1.5) != b).any()
    assert (_bytes(-np.abs(flow), clip=2.0) == 255).all()               # everything clamps to zero flow


@pytest.mark.parametrize("shape", fc.BASE_SHAPES + fc.geometry_shapes(_lib.load().rcf_flow_color_geometry(0)), ids=lambda s: f"{s[0]}x{s[1]}")
def test_float32_restatement_inside_the_rule(shape):
    flows, levels = fc.batch(*shape)
    for kind, flow, lv in zip(fc.FINITE_KINDS, flows, levels):
        v = fc.judge(fc.to_bytes(fc.color_levels(flow, head=np.float32)), lv)
        assert v.ok, (kind, v)
        if kind in fc.BIT_EQUAL_KINDS:
            assert v.differing == 0, (kind, v)
        assert np.isfinite(lv).all() and lv.min() >= 0 and lv.max() <= 255


def test_rule_constants():
    assert fc.K == 65 and abs(fc.EPS - 65 * 255 / 2 ** 24) < 1e-15 and fc.CAP == 1e-3
    lv = np.array([[[10.5, 11.0 + 0.5 * fc.EPS, 12.0 - 2 * fc.EPS]]])
    assert fc.judge(np.array([[[10, 11, 11]]], dtype=np.uint8), lv).ok
    assert not fc.judge(np.array([[[10, 10, 11]]], dtype=np.uint8), lv).ok                 # 3 elements: the cap allows none
    big = np.full((3, 40, 40), 10.5)
    big[0, 0, 0] = 11.0 - 0.5 * fc.EPS
    got = np.full((3, 40, 40), 10, dtype=np.uint8)
    assert fc.judge(got, big).ok
    got[0, 0, 0] = 11
    assert fc.judge(got, big).ok                                          # one level, within EPS of an integer, under the cap
    got[0, 0, 1] = 11
    assert not fc.judge(got, big).ok                                      # 10.5 is nowhere near an integer
    got[0, 0, 1], got[0, 0, 0] = 10, 12
    assert not fc.judge(got, big).ok                                      # two levels


def test_abi_symbol_declared_exported_and_refuses_bad_arguments():
    import os
    hdr = open(os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "include", "rcf_hip.h")).read()
    for name in ("rcf_flow_color_f32", "rcf_flow_color_workspace_bytes", "rcf_flow_color_geometry"):
        assert name + "(" in hdr and name in _lib.PROTOS
        for which in ("bf16", "f16"):
            assert hasattr(_lib.load(which), name)
    lib = _lib.load()
    one, tile = lib.rcf_flow_color_geometry(0), lib.rcf_flow_color_geometry(1)
    assert one >= tile > 0 and lib.rcf_flow_color_geometry(2) == 0
    assert lib.rcf_flow_color_workspace_bytes(20, 1, 48, 48) == 0 and lib.rcf_flow_color_workspace_bytes(20, 1, 1, one + 1) == 80
    lay = _lib.FlowLayout(0, 0, 16, 4, 1)
    ok = lambda **kw: lib.rcf_flow_color_f32(*[kw.get(k, d) for k, d in (
        ("flow", None), ("src", lay), ("out", None), ("dst", lay), ("out_type", 0), ("n", 1), ("group", 1), ("h", 4), ("w", 4),
        ("bgr", 0), ("clip", -1.0), ("ws", None), ("ws_bytes", 0), ("stream", None))])
    assert ok() == -1                                                     # NULL pointers, after the sizes passed
    for bad in (dict(h=0), dict(w=0), dict(n=0), dict(h=(1 << 14) + 1), dict(group=0), dict(n=3, group=2), dict(out_type=2),
                dict(clip=float("nan")), dict(src=None), dict(dst=_lib.FlowLayout(0, 0, 16, 4, 0)), dict(src=_lib.FlowLayout(-1, 0, 16, 4, 1))):
        assert ok(**bad) == -1, bad


def test_python_surface_refuses_cpu_and_wrong_types():
    from rcf_amd import ops
    with pytest.raises(_lib.RcfHipError):
        ops.flow_color(torch.zeros(1, 2, 4, 4))
    for bad in (np.zeros((4, 4)), np.zeros((1, 4, 4, 2)), torch.zeros(2, 4, 4, 2)):
        with pytest.raises(AssertionError, match="three dimensions"):
            flowvis.flow_to_color(bad)
    for bad in (np.zeros((4, 4, 3)), torch.zeros(2, 4, 4)):
        with pytest.raises(AssertionError, match=r"\[H,W,2\]"):
            flowvis.flow_to_color(bad)
    assert hasattr(rcf_amd.RCFModel, "let_tensor_vis") and hasattr(rcf_amd.AMDModel, "let_tensor_vis")


# ---------------------------------------------------------------------------------------------------------------------- the grid
@pytest.mark.parametrize("M", [1, 5])
@pytest.mark.parametrize("affine", [False, True])
@pytest.mark.parametrize("with_pl", [False, True])
def test_rcf_grid_layout(M, affine, with_pl):
    kinds = flowvis.rcf_flow_kinds(affine)
    assert kinds == (("pred", "gt", "agg", "aff", "adj") if affine else ("pred", "gt", "agg", "adj"))
    _check_layout(M, kinds, with_pl)


def test_amd_grid_layout():
    assert flowvis.AMD_FLOW_KINDS == ("seg", "whole")
    _check_layout(5, flowvis.AMD_FLOW_KINDS, False)


def _check_layout(M, kinds, with_pl):
    """every panel a constant that names (panel, frame, sample): the grid holds them in the reference's order, each h rows of the
    full width, frame 0's samples first"""
    I, B, h, w, K = 2, 3, 4, 6, len(kinds)
    names = flowvis.grid_panels(M, kinds, with_pl)
    assert names == [f"mask{m}" for m in range(M)] + ["frame"] + ["flow_" + k for k in kinds] + (["pl"] if with_pl else [])
    tag = lambda p: (100.0 * p + 10.0 * torch.arange(I).view(I, 1) + torch.arange(B).view(1, B)).view(I, B, 1, 1, 1)
    masks = torch.cat([tag(m).expand(I, B, 1, h, w) for m in range(M)], 2)
    frames = tag(M).expand(I, B, 3, h, w)
    flows = [tag(M + 1 + k).expand(I, B, 3, h, w) for k in range(K)]
    pl = tag(M + 1 + K)[:, :, 0].expand(I, B, h, w) if with_pl else None
    grid = flowvis.assemble_grid(masks, frames, flows, pl)
    P = len(names)
    assert tuple(grid.shape) == (I * B, 3, P * h, w)
    for p in range(P):
        for i in range(I):
            for b in range(B):
                assert (grid[i * B + b, :, p * h:(p + 1) * h] == 100.0 * p + 10.0 * i + b).all(), (names[p], i, b)
