"""CPU: the export's host side -- the float32 restatement of the panel arithmetic against its float64 yardstick (the rule the GPU
tests hold the kernel to), the test split's frame list, every checkpoint format of load_pretrained, the grid canvas geometry."""
import os
import types

import numpy as np
import pytest
import torch
import torch.nn as nn

import export_cases as xc
from rcf_amd import export, export_driver

EXTRA = [xc._case("98x175", 1, 5, 98, 175, seed=31), xc._case("98x175_align", 1, 5, 98, 175, align=True, seed=32)]
RANDOM = [c for c in xc.cases() + EXTRA if c.kind in xc.RANDOM_KINDS]


@pytest.mark.parametrize("c", [pytest.param(c, id=c.name) for c in RANDOM])
def test_float32_restatement_against_float64(c):
    masks, frames = xc.inputs(c)
    assert c.C == 5
    near = total = 0
    for b in range(c.B):
        for ch in range(c.C):
            l64 = xc.levels(masks[b, ch], (c.Ho, c.Wo), c.align, np.float64)
            got = xc.panel_bytes(masks[b, ch], (c.Ho, c.Wo), c.align)
            assert xc.passes(got, l64), (c.name, b, ch, xc.judge(got, l64))
            near += int(xc.near_integer(l64).sum())
            total += l64.size
        for ch in range(3):
            l64 = xc.levels(frames[b, ch], (c.Ho, c.Wo), c.align, np.float64, frame=True)
            got = xc.panel_bytes(frames[b, ch], (c.Ho, c.Wo), c.align, frame=True)
            assert xc.passes(got, l64), (c.name, b, ch, xc.judge(got, l64))
    assert near <= xc.NEAR_SHARE * total, f"{c.name}: {near} of {total} float64 levels within EPS of an integer"


def test_restatement_edge_values():
    """exact 0 and 1, NaN -> 0, infinities and 3e38 clamp, frames at +-2"""
    one = np.ones((3, 4), np.float32)
    for align in (False, True):
        assert (xc.panel_bytes(one, (6, 8), align) == 255).all() and (xc.panel_bytes(0 * one, (6, 8), align) == 0).all()
        assert (xc.panel_bytes(2 * one, (6, 8), align, frame=True) == 255).all()
        assert (xc.panel_bytes(-2 * one, (6, 8), align, frame=True) == 0).all()
        assert (xc.panel_bytes(np.float32(3e38) * one, (6, 8), align) == 255).all()
        assert (xc.panel_bytes(np.nan * one, (6, 8), align) == 0).all()
        inf = xc.panel_bytes(np.inf * one, (6, 8), align)
        assert set(np.unique(inf)) <= {0, 255} and (inf == 255).any()          # 0 x inf = NaN -> 0 where a blend weight is 0
        assert (xc.panel_bytes(-np.inf * one, (6, 8), align) == 0).all()
    assert xc.to_bytes(np.array([-1.0, 0.999, 1.0, 254.999, 255.0, 300.0, np.nan])).tolist() == [0, 0, 1, 254, 255, 255, 0]


def test_entry_point_refuses_bad_arguments_before_any_launch():
    import ctypes
    from rcf_amd import _lib
    lib = _lib.load()
    assert [lib.rcf_export_geometry(i) for i in range(5)] == [4, 256, 4, 2, 0]
    assert xc.cases((4, 256, 4, 2)) == xc.cases()                                 # the case list's default geometry is the library's
    lay = _lib.ExportLayout(None, 0, 12, 0, 12, 6, 3, 0, 0, 8, 1)
    assert lib.rcf_export_panels_u8(None, 0, 1, 1, 1, None, 0, 0, 0, None, 1, 1, 2, 2, 0, None) == -1       # no destination
    assert lib.rcf_export_panels_u8(None, 0, 1, 1, 1, None, 0, 0, 0, ctypes.byref(lay), 1, 1, 2, 2, 0, None) == -1   # no base
    assert ctypes.sizeof(_lib.ExportLayout) == 8 * 7 + 4 * 4 + 4 * _lib.EXPORT_MAX_SLOTS


# ---- frames ------------------------------------------------------------------------------------------------------------------
def test_list_eval_frames(tmp_path):
    root = tmp_path / "data"
    root.mkdir()
    (root / "val.txt").write_text("JPEGImages/480p/zebra/ 00000.jpg 00001.jpg 00002.jpg 00003.jpg 00004.jpg\n"
                                  "JPEGImages/480p/ant 00000.jpg 00001.jpg 00002.jpg\n")
    r = str(root)
    fr = export_driver.list_eval_frames(r, "val.txt")
    assert [(f[0], f[1]) for f in fr] == [(0, "ant")] * 3 + [(1, "zebra")] * 5                      # sorted lines
    assert fr[0][2] == os.path.join(r, "JPEGImages/480p/ant", "00000.jpg")
    assert fr[0][3] == os.path.join(r, "Annotations/480p/ant", "00000.png")
    assert fr[3][2] == os.path.join(r, "JPEGImages/480p/zebra/", "00000.jpg")
    first = export_driver.list_eval_frames(r, "val.txt", subsample_frame_interval=-1)
    assert [os.path.basename(f[2]) for f in first] == ["00000.jpg", "00000.jpg"] and [f[1] for f in first] == ["ant", "zebra"]
    third = export_driver.list_eval_frames(r, "val.txt", subsample_frame_interval=3)
    assert [(f[1], os.path.basename(f[2])) for f in third] == [("ant", "00000.jpg"), ("zebra", "00000.jpg"), ("zebra", "00003.jpg")]
    z = export_driver.list_eval_frames(r, "val.txt", zero_ann=True)
    assert len(z) == 8 and all(f[3] is None for f in z) and [f[2] for f in z] == [f[2] for f in fr]


def test_plan_batches_closes_on_size_change():
    sizes = [((4, 6), (4, 6))] * 3 + [((4, 6), (8, 12))] + [((5, 6), (8, 12))] * 2
    assert export_driver.plan_batches(list(range(6)), 2, sizes) == [[0, 1], [2], [3], [4, 5]]
    assert export_driver.plan_batches(list(range(6)), 8, sizes) == [[0, 1, 2], [3], [4, 5]]
    assert export_driver.plan_batches([], 2, []) == []


# ---- checkpoints -------------------------------------------------------------------------------------------------------------
class _Backbone(nn.Module):
    def __init__(self):
        super().__init__()
        self.conv1 = nn.Conv2d(3, 4, 3, bias=False)
        self.bn1 = nn.BatchNorm2d(4)


class _Stub(nn.Module):
    def __init__(self, ema):
        super().__init__()
        self.backbone2, self.decode_head2, self.decode_head3 = _Backbone(), nn.Conv2d(4, 5, 1), nn.Conv2d(4, 2, 1)
        self.backbone2_ema, self.decode_head2_ema = (_Backbone(), nn.Conv2d(4, 5, 1)) if ema else (None, None)


def _filled(module, seed):
    g = torch.Generator().manual_seed(seed)
    return {k: torch.rand(v.shape, generator=g).to(v.dtype) for k, v in module.state_dict().items()}


def _same(a, b):
    return all(torch.equal(a[k], b[k]) for k in b)


def _load(tmp_path, obj, model, log=None, **kw):
    p = str(tmp_path / "ckpt.pth")
    torch.save(obj, p)
    return export_driver.load_pretrained(model, p, types.SimpleNamespace(**kw), log=log or (lambda s: None))


def test_load_pretrained_main_format(tmp_path):
    src = _filled(_Stub(False), 1)
    ckpt = {"state_dict": {"model." + k: v for k, v in src.items()}}
    m = _Stub(False)
    _load(tmp_path, ckpt, m)
    assert _same(m.state_dict(), src)
    # the EMA duplication: the model has *_ema modules, the file has none
    m = _Stub(True)
    lines = []
    _load(tmp_path, ckpt, m, log=lines.append)
    assert any("Detected EMA in model but not in state_dict" in s for s in lines)
    sd = m.state_dict()
    assert _same(sd, src)
    assert all(torch.equal(sd[k.replace("backbone2", "backbone2_ema").replace("decode_head2", "decode_head2_ema")], v)
               for k, v in src.items() if "backbone2" in k or "decode_head2" in k)
    # a file WITH ema keys is loaded as it is; a bare dict (no 'state_dict') too
    src_ema = _filled(_Stub(True), 2)
    m = _Stub(True)
    _load(tmp_path, {"model." + k: v for k, v in src_ema.items()}, m)
    assert _same(m.state_dict(), src_ema)
    # drop_head_decode_head2
    m = _Stub(True)
    before = {k: v.clone() for k, v in m.state_dict().items()}
    _load(tmp_path, ckpt, m, drop_head_decode_head2=True)
    sd = m.state_dict()
    assert all(torch.equal(sd[k], before[k]) for k in sd if "decode_head2" in k)
    assert all(torch.equal(sd[k], src[k]) for k in src if "decode_head2" not in k)


def test_load_pretrained_backbone_formats(tmp_path):
    bb = _filled(_Backbone(), 3)
    for fmt in ("moco", "densecl"):
        m = _Stub(False)
        if fmt == "moco":
            obj = {"state_dict": dict({"module.encoder_q." + k: v for k, v in bb.items()},
                                      **{"module.encoder_q.fc.weight": torch.zeros(2, 2), "module.encoder_k.conv1.weight": torch.zeros(4, 3, 3, 3)})}
        else:
            obj = {"state_dict": bb}
        _, mismatches = _load(tmp_path, obj, m)
        assert _same(m.backbone2.state_dict(), bb) and not mismatches.unexpected_keys and not mismatches.missing_keys
        # a model with EMA modules cannot take a backbone-only file
        with pytest.raises(AssertionError, match="EMA is enabled but weights are not loaded"):
            _load(tmp_path, obj, _Stub(True))
    # un-prefixed main model; with pretrained_model_backbone_only the other keys are left alone
    src = _filled(_Stub(False), 4)
    m = _Stub(False)
    _load(tmp_path, src, m)
    assert _same(m.state_dict(), src)
    m = _Stub(False)
    before = {k: v.clone() for k, v in m.state_dict().items()}
    _load(tmp_path, src, m, pretrained_model_backbone_only=True)
    sd = m.state_dict()
    assert all(torch.equal(sd[k], src[k] if "backbone" in k else before[k]) for k in sd)
    with pytest.raises(ValueError, match="Unknown module"):
        _load(tmp_path, {"head.weight": torch.zeros(1)}, _Stub(False))


def test_load_pretrained_wildcard(tmp_path):
    src = {"state_dict": {"model." + k: v for k, v in _filled(_Stub(False), 5).items()}}
    torch.save(src, str(tmp_path / "epoch=3.ckpt"))
    ns = types.SimpleNamespace()
    path, _ = export_driver.load_pretrained(_Stub(False), str(tmp_path / "epoch=*.ckpt"), ns, log=lambda s: None)
    assert path == str(tmp_path / "epoch=3.ckpt")
    torch.save(src, str(tmp_path / "epoch=4.ckpt"))
    with pytest.raises(AssertionError, match="is not unique"):
        export_driver.load_pretrained(_Stub(False), str(tmp_path / "epoch=*.ckpt"), ns, log=lambda s: None)


# ---- the grid ----------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("B", [1, 2, 8, 9])
def test_grid_geometry_matches_make_grid(B):
    H, W = 6, 5
    t = torch.arange(1, B + 1, dtype=torch.float32).view(B, 1, 1, 1).expand(B, 3, H, W) / 16.0
    grid = export.make_grid(t)
    Hc, Wc, off, cell_h, cell_w, per_row = export.grid_geometry(B, H, W)
    assert tuple(grid.shape) == (3, Hc, Wc)
    canvas = torch.zeros(Hc, Wc)
    for k in range(B):
        y, x = off + (k // per_row) * cell_h, off + (k % per_row) * cell_w
        canvas[y:y + H, x:x + W] = (k + 1) / 16.0
    assert torch.equal(canvas, grid[0]) and torch.equal(canvas, grid[2])


def test_driver_command_line():
    a = export_driver.parse_args(["cfg.yaml", "--test", "--test-override-pretrained", "x/last.ckpt", "--test-override-object-channel", "2",
                                  "--batch-size", "3", "--workers", "40", "--sync", "--opts", "checkpoints_dir", "out", "object_channel", "1"])
    assert (a.config, a.test, a.test_override_pretrained, a.test_override_object_channel) == ("cfg.yaml", True, "x/last.ckpt", 2)
    assert (a.batch_size, a.workers, a.sync, a.opts) == (3, 40, True, ["checkpoints_dir", "out", "object_channel", "1"])
    b = export_driver.parse_args(["cfg.yaml"])
    assert b.batch_size is None and b.workers is None and not b.sync and b.opts == []
    assert export.MaskExporter.MAX_WORKERS == 16 and export_driver.MAX_WORKERS == 16
