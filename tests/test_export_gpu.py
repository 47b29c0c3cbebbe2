"""GPU: rcf_export_panels_u8 bit-equal to the route it replaces (ops.resize_nchw + repeat + export.to_uint8_hwc, computed here) and,
for the random cases, within the float64 rule of tests/export_cases.py; RCFModel / AMDModel with a MaskExporter attached against
`exporter = None` (same file names, byte-identical files, bit-equal returns); the export driver against a plain loop."""
import copy
import os
import types

import numpy as np
import pytest
import torch
import yaml

import amd_cases as ac
import export_cases as xc
import rcf_amd
from rcf_amd import _lib, config, export, export_driver, ops, synth

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
SENTINEL = 0xA5
CASES = xc.cases(ops.export_geometry())


# ------------------------------------------------------------------------------------------------------------------ the kernel
def _torch_route(c, masks, frames):
    """the existing route: (img0 [B, 3, Ho, Wo], vis[ch] [B, 3, Ho, Wo]) float32 on the device"""
    size = (c.Ho, c.Wo)
    vis = [ops.resize_nchw(masks[:, i:i + 1].contiguous(), size, c.align).repeat(1, 3, 1, 1) for i in range(c.C)]
    img0 = (ops.resize_nchw(frames.contiguous(), size, c.align) + 2.0) / 4.0
    return img0, vis


def _expected_panels(c, masks_np, img0, vis):
    """panel bytes [Ho, Wo, 3] by (source, sample): the torch route's, or the documented bytes for a plane that is not finite"""
    out = {}
    for b in range(c.B):
        out[ops.EXPORT_FRAME, b] = export.to_uint8_hwc(img0[b])
        for ch in range(c.C):
            if ch in xc.dirty_planes(c):
                out[ch, b] = np.repeat(xc.panel_bytes(masks_np[b, ch], (c.Ho, c.Wo), c.align)[..., None], 3, axis=2)
            else:
                out[ch, b] = export.to_uint8_hwc(vis[ch][b])
    return out


def _paste(canvas, panels, sources, c, y0, x0):
    _, _, off, cell_h, cell_w, per_row = export.grid_geometry(c.B, len(sources) * c.Ho, c.Wo)
    for b in range(c.B):
        for j, s in enumerate(sources):
            y, x = y0 + off + (b // per_row) * cell_h + j * c.Ho, x0 + off + (b % per_row) * cell_w
            canvas[y:y + c.Ho, x:x + c.Wo] = panels[s, b]


def _grid_layout(buf, sources, c, y0, x0):
    """the windows of make_grid's canvas (panels of a sample stacked downwards) inside `buf` [rows, cols, 3], canvas origin (y0, x0)"""
    _, _, off, cell_h, cell_w, per_row = export.grid_geometry(c.B, len(sources) * c.Ho, c.Wo)
    row = buf.shape[1] * 3
    return ops.export_layout(buf, sources, image=cell_w * 3, image_row=cell_h * row, slot=c.Ho * row, row=row, x=x0 + off, y=y0 + off,
                             per_row=per_row)


@pytest.mark.parametrize("c", [pytest.param(c, id=c.name) for c in CASES])
def test_panels_bit_equal_to_the_torch_route(c, report):
    masks_np, frames_np = xc.inputs(c)
    masks, frames = torch.from_numpy(masks_np).to(DEV), torch.from_numpy(frames_np).to(DEV)
    size = (c.Ho, c.Wo)
    sel = list(range(c.C)) if c.sel is None else [c.sel]
    sources = [ops.EXPORT_FRAME] + list(range(c.C))
    Hc, Wc = export.grid_geometry(c.B, len(sources) * c.Ho, c.Wo)[:2]
    y0, x0 = 1, 2 + c.xoff

    def run():
        png = torch.full((len(sel), c.B, c.Ho, c.Wo, 3), SENTINEL, dtype=torch.uint8, device=DEV)
        big = torch.full((Hc + 3, Wc + 7 + c.xoff, 3), SENTINEL, dtype=torch.uint8, device=DEV)
        ops.export_panels_u8(masks, frames, [ops.export_contiguous_layout(png, sel), _grid_layout(big, sources, c, y0, x0)], size, c.align)
        canvas = torch.zeros((Hc, Wc, 3), dtype=torch.uint8, device=DEV)
        ops.export_panels_u8(masks, frames, [_grid_layout(canvas, sources, c, 0, 0)], size, c.align)
        return png.cpu().numpy(), big.cpu().numpy(), canvas.cpu().numpy()

    png, big, canvas = run()
    img0, vis = _torch_route(c, masks, frames)
    panels = _expected_panels(c, masks_np, img0, vis)
    # the contiguous [C_sel, B, Ho, Wo, 3] destination
    for j, ch in enumerate(sel):
        for b in range(c.B):
            assert np.array_equal(png[j, b], panels[ch, b]), (c.name, "png", ch, b)
    # a canvas window inside a larger sentinel-filled buffer: the sentinel is intact outside the windows (the grid's padding too)
    want = np.full(big.shape, SENTINEL, dtype=np.uint8)
    _paste(want, panels, sources, c, y0, x0)
    assert np.array_equal(big, want), (c.name, "window", np.argwhere(big != want)[:4].tolist())
    # the whole zero-filled canvas against save_image's array of the concatenated batch
    if not xc.dirty_planes(c):
        assert np.array_equal(canvas, export.to_uint8_hwc(torch.cat([img0] + vis, 2))), (c.name, "canvas")
    want = np.zeros(canvas.shape, dtype=np.uint8)
    _paste(want, panels, sources, c, 0, 0)
    assert np.array_equal(canvas, want)
    # the same bits from call to call
    again = run()
    assert all(np.array_equal(a, b) for a, b in zip((png, big, canvas), again))
    if c.kind in xc.RANDOM_KINDS:
        taken = n = 0
        for b in range(c.B):
            for j, ch in enumerate(sel):
                l64 = xc.levels(masks_np[b, ch], size, c.align, np.float64)
                assert xc.passes(png[j, b, :, :, 0], l64), (c.name, ch, b, xc.judge(png[j, b, :, :, 0], l64))
                taken, n = taken + xc.judge(png[j, b, :, :, 0], l64)[1], n + l64.size
            for k in range(3):
                l64 = xc.levels(frames_np[b, k], size, c.align, np.float64, frame=True)
                got = panels[ops.EXPORT_FRAME, b][:, :, k]
                assert xc.passes(got, l64), (c.name, "frame", k, b, xc.judge(got, l64))
                taken, n = taken + xc.judge(got, l64)[1], n + l64.size
        report(f"export {c.name}: {taken} of {n} bytes one level from the float64 byte (allowed within {xc.EPS:.2e} of an integer)")


def test_documented_bytes_of_values_that_are_not_numbers():
    c = next(c for c in CASES if c.kind == "nonfinite")
    masks_np, _ = xc.inputs(c)
    masks = torch.from_numpy(masks_np).to(DEV)
    png = torch.full((c.C, c.B, c.Ho, c.Wo, 3), SENTINEL, dtype=torch.uint8, device=DEV)
    ops.export_panels_u8(masks, None, [ops.export_contiguous_layout(png, list(range(c.C)))], (c.Ho, c.Wo), c.align)
    png = png.cpu().numpy()
    assert (png[0] == 0).all()                                               # NaN -> 0
    assert set(np.unique(png[1, 0])) == {0, 255} and (png[1, 1] == 0).all()  # +inf: 255, and 0 where 0 x inf = NaN; -inf: 0
    assert (png[2] == 255).all()                                             # 3e38 clamps


def test_refused_arguments():
    buf = torch.zeros((1, 2, 4, 4, 3), dtype=torch.uint8, device=DEV)
    masks = torch.zeros((2, 3, 2, 2), device=DEV)
    with pytest.raises(_lib.RcfHipError):                  # a channel the masks do not have
        ops.export_panels_u8(masks, None, [ops.export_contiguous_layout(buf, [3])], (4, 4))
    with pytest.raises(_lib.RcfHipError):                  # a frame slot without frames
        ops.export_panels_u8(masks, None, [ops.export_contiguous_layout(buf, [ops.EXPORT_FRAME])], (4, 4))
    with pytest.raises(_lib.RcfHipError):                  # the last panel would end beyond the buffer
        ops.export_panels_u8(masks, None, [ops.export_contiguous_layout(buf, [0])], (4, 5))
    with pytest.raises(_lib.RcfHipError):
        ops.export_panels_u8(masks, None, [ops.export_contiguous_layout(buf, [0])] * 3, (4, 4))
    assert (buf == 0).all()


# ------------------------------------------------------------------------------------------------------------------- the models
def _files(root):
    out = {}
    for d, _, names in os.walk(root):
        for n in names:
            p = os.path.join(d, n)
            out[os.path.relpath(p, root)] = open(p, "rb").read()
    return out


def _rcf_model():
    H, W = 64, 96                                          # the smallest input of tests/test_model_gpu.py
    kw = config.stage1_model_kwargs(config.mask_size_for(H, W), dropout=0.0, affine=False, norm="BN")
    kw.update(log_interval=10 ** 9, train_iter=42)
    args = types.SimpleNamespace(checkpoints_dir="/tmp/rcf_export_test", object_channel=1, eval_save=False, eval_export=False)
    m = rcf_amd.RCFModel(args, **copy.deepcopy(kw))
    shapes = {k: tuple(v.shape) for k, v in m.state_dict().items()}
    m.load_state_dict({k: torch.from_numpy(v) for k, v in synth.fill_state_dict(shapes, seed=7).items()})
    nb = synth.make_batch(2, H, W, config_id=1)
    batch = {"imgs": [torch.from_numpy(np.ascontiguousarray(a)).to(DEV) for a in nb["imgs"]]}
    return m.to(DEV).eval(), batch


def _amd_model():
    args = types.SimpleNamespace(checkpoints_dir="/tmp/rcf_amd_export_test", object_channel=2, eval_save=False, eval_export=False)
    m = rcf_amd.AMDModel(args, **ac.model_kwargs())
    m.load_state_dict(ac.state_dict({k: tuple(v.shape) for k, v in m.state_dict().items()}))
    return m.to(DEV).eval(), {"imgs": ac.batch(DEV)["imgs"]}


@pytest.fixture(scope="module", params=["rcf", "amd"])
def small_model(request):
    return (_rcf_model if request.param == "rcf" else _amd_model)()


MODES = dict(object_channel=dict(eval_save=True, eval_export=True, export_all_seg=False),
             all_seg=dict(eval_save=True, eval_export=True, export_all_seg=True),
             save_only=dict(eval_save=True, eval_export=False, export_all_seg=False))


@pytest.mark.parametrize("B", [1, 2])
@pytest.mark.parametrize("mode", list(MODES))
def test_model_with_exporter_writes_the_same_files(small_model, mode, B, tmp_path):
    model, full = small_model
    batch = {"imgs": [t[:B] for t in full["imgs"]], "seq_names": [f"seq{i}" for i in range(B)], "seq_ids": torch.tensor([3, 4][:B]),
             "paths": [[f"/data/JPEGImages/480p/seq{i}/{i:05d}.jpg" for i in range(B)]] * 2}
    for k, v in MODES[mode].items():
        setattr(model.args, k, v)
    want_vis = mode == "all_seg"
    runs = {}
    exporter = export.MaskExporter(DEV, workers=3)
    try:
        for name, exp in (("plain", None), ("exporter", exporter)):
            root = tmp_path / name
            model.save_dir_eval, model.save_dir_eval_export = str(root / "saved_eval"), str(root / "saved_eval_export")
            model.exporter = exp
            with torch.no_grad():
                out = model(batch, return_pred_vis_list=True) if want_vis else model(batch)
                if exp is not None:                         # a second batch: the other pinned set, then the first one again
                    model(batch)
                    model(batch)
            if exp is not None:
                exp.flush()
                assert exp.pending() == 0 and exp.batches == 3
            runs[name] = (out, _files(str(root)))
    finally:
        model.exporter = None
        model.args.eval_save = model.args.eval_export = False
        exporter.close()
    (a, fa), (b, fb) = runs["plain"], runs["exporter"]
    assert sorted(fa) == sorted(fb) and len(fa) == 1 + B * {"object_channel": 1, "all_seg": model.mask_layer, "save_only": 0}[mode]
    assert all(fa[k] == fb[k] for k in fa), [k for k in fa if fa[k] != fb[k]]
    if want_vis:
        assert torch.equal(a[0], b[0]) and len(a[1]) == len(b[1]) and all(torch.equal(x, y) for x, y in zip(a[1], b[1]))
    else:
        assert torch.equal(a, b)


def test_exporter_sync_and_failed_write(small_model, tmp_path, capsys):
    """sync=True writes the same files inline; a write that fails prints the reference's line and raises nothing"""
    model, full = small_model
    batch = {"imgs": full["imgs"], "seq_names": ["a", "b"], "seq_ids": torch.tensor([0, 1]),
             "paths": [["/d/JPEGImages/a/00000.jpg", "/d/JPEGImages/b/00007.jpg"]] * 2}
    model.args.eval_save, model.args.eval_export, model.args.export_all_seg = True, True, False
    files = {}
    try:
        for name, exp in (("async", export.MaskExporter(DEV, workers=2)), ("sync", export.MaskExporter(DEV, workers=2, sync=True))):
            root = tmp_path / name
            model.save_dir_eval, model.save_dir_eval_export = str(root / "saved_eval"), str(root / "saved_eval_export")
            model.exporter = exp
            with torch.no_grad():
                model(batch)
            exp.close()
            files[name] = _files(str(root))
        assert files["async"] == files["sync"] and len(files["sync"]) == 3
        blocked = tmp_path / "blocked"
        blocked.write_text("a file where a directory is needed")
        model.save_dir_eval, model.exporter = str(blocked), export.MaskExporter(DEV, workers=2)
        with torch.no_grad():
            model(batch)
        model.exporter.close()
        assert "Error in saving: " + str(blocked) in capsys.readouterr().out
    finally:
        model.exporter = None
        model.args.eval_save = model.args.eval_export = False


# ------------------------------------------------------------------------------------------------------------------- the driver
def _write_dataset(root):
    from PIL import Image
    rng = np.random.RandomState(3)
    lines = []
    for seq, n in (("walk", 3), ("bus", 2)):
        os.makedirs(os.path.join(root, "JPEGImages/480p", seq))
        os.makedirs(os.path.join(root, "Annotations/480p", seq))
        for i in range(n):
            img = rng.randint(0, 256, size=(6, 10, 3)).astype(np.uint8).repeat(8, 0).repeat(8, 1)          # 48 x 80
            Image.fromarray(img).save(os.path.join(root, "JPEGImages/480p", seq, f"{i:05d}.jpg"), quality=95)
            ann = np.zeros((48, 80), dtype=np.uint8)
            ann[8 + 4 * i:32, 16:56 + 4 * i] = 255
            ann[0:4] = 128
            Image.fromarray(ann).save(os.path.join(root, "Annotations/480p", seq, f"{i:05d}.png"))
        lines.append(f"JPEGImages/480p/{seq} " + " ".join(f"{i:05d}.jpg" for i in range(n)) + "\n")
    with open(os.path.join(root, "val.txt"), "w") as f:
        f.writelines(lines)


@pytest.fixture(scope="module")
def driver_setup(tmp_path_factory):
    root = tmp_path_factory.mktemp("export_driver")
    data = str(root / "data")
    os.makedirs(data)
    _write_dataset(data)
    kw = config.stage1_model_kwargs(config.mask_size_for(392, 653), mask_layer=3, dropout=0.0, norm="BN")
    kw["backbone2"]["create_ema"] = kw["decode_head2"]["create_ema"] = True
    cfg = dict(batch_size=2, workers=3, model_cls="RCFModel", model_kwargs=kw, data_path=data, dataset_kwargs={},
               test_dataset_kwargs=dict(frame_num=1, load_flow=False, split="val.txt", zero_ann=False),
               test_transform_kwargs=dict(strong_aug=False), eval_pos_th=0.35, eval_save=True, eval_export=True, export_all_seg=True,
               eval_on_ema=True, object_channel=None, checkpoints_dir=str(root / "unused"), pretrained_model=None,
               allow_overwriting_checkpoints_dir=True, trainer_kwargs=dict(precision=32), saved_eval_dir_name="saved_eval_test",
               saved_eval_export_dir_name="saved_eval_export_trainval_ema")
    cfg_path = str(root / "export.yaml")
    with open(cfg_path, "w") as f:
        yaml.safe_dump(cfg, f)
    # a randomly initialised checkpoint in the `model.`-prefixed format without EMA keys
    torch.manual_seed(11)
    args = config.load_args(cfg_path)
    args.eval_on_ema = False
    m = rcf_amd.RCFModel(args, **copy.deepcopy(config.stage1_model_kwargs(config.mask_size_for(392, 653), mask_layer=3, dropout=0.0, norm="BN")))
    shapes = {k: tuple(v.shape) for k, v in m.state_dict().items()}
    sd = {"model." + k: torch.from_numpy(v) for k, v in synth.fill_state_dict(shapes, seed=13).items()}
    assert not any("_ema" in k for k in sd)
    ckpt = str(root / "last.ckpt")
    torch.save({"state_dict": sd}, ckpt)
    return dict(root=root, cfg=cfg_path, ckpt=ckpt)


def _reference_run(setup, ckpt, extra_opts):
    """a plain loop: the same batches through Evaluator.test_step with exporter = None"""
    cli = export_driver.parse_args([setup["cfg"], "--test", "--test-override-pretrained", ckpt, "--opts"] + extra_opts)
    args = export_driver.prepare_args(cli)
    export_driver.make_dirs(args)
    model = export_driver.build_model(args, DEV)
    export_driver.load_pretrained(model, args.pretrained_model, args, log=lambda s: None)
    model.eval()
    kw = args.test_dataset_kwargs
    frames = export_driver.list_eval_frames(args.data_path, kw["split"], None, kw["zero_ann"])
    loader = export_driver.EvalLoader(frames, args.batch_size, export_driver.get_transform(args, training=False), DEV, 2)
    ev = rcf_amd.Evaluator(args, args.model_kwargs["mask_layer"])
    assert model.exporter is None
    for batch in loader:
        ev.test_step(model, batch)
    loader.close()
    return export_driver.report_lines(args, ev)[0], len(frames)


@pytest.mark.filterwarnings("ignore:Mean of empty slice")           # zero_ann: every IoU is 0 / 0
@pytest.mark.parametrize("variant", ["async", "sync", "zero_ann"])
def test_driver_against_a_plain_loop(driver_setup, variant, capsys):
    root = driver_setup["root"]
    dirs = {}
    for leg in ("driver", "plain"):
        dirs[leg] = str(root / f"{variant}_{leg}")
        os.makedirs(dirs[leg])
        os.link(driver_setup["ckpt"], os.path.join(dirs[leg], "last.ckpt"))          # checkpoints_dir is the checkpoint's directory
    opts = ["test_dataset_kwargs.zero_ann", "True"] if variant == "zero_ann" else []
    argv = [driver_setup["cfg"], "--test", "--test-override-pretrained", os.path.join(dirs["driver"], "last.ckpt")]
    argv += (["--sync"] if variant == "sync" else []) + (["--opts"] + opts if opts else [])
    capsys.readouterr()
    out = export_driver.run(argv, device=DEV)
    printed = capsys.readouterr().out.splitlines()
    want_lines, n = _reference_run(driver_setup, os.path.join(dirs["plain"], "last.ckpt"), opts)
    assert out["frames"] == n == 5 and out["batches"] == 3                  # 3 + 2 frames of one size in batches of 2
    assert out["lines"] == want_lines and [s for s in printed if s in want_lines] == want_lines
    assert any("Set object channel to" in s for s in want_lines) and want_lines[-2].startswith("test_miou: ")
    assert sum(s.startswith("test_miou_") for s in want_lines) == 3        # walk, bus, frame_avg
    fa, fb = _files(dirs["plain"]), _files(dirs["driver"])
    fa.pop("last.ckpt"), fb.pop("last.ckpt")
    assert sorted(fa) == sorted(fb) and len(fa) == 3 + 5 * 3                # a JPEG per batch, a PNG per frame and channel
    assert all(k.startswith(("saved_eval_test/", "saved_eval_export_trainval_ema/")) for k in fa)
    assert all(fa[k] == fb[k] for k in fa), [k for k in fa if fa[k] != fb[k]]
