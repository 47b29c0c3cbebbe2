#!/usr/bin/env python3
"""Time the evaluation export (ops.export_panels_u8, export.MaskExporter, rcf_amd.export_driver) against the route it replaces, in one
process.

  the kernel call   8 frames of 392 x 697 with masks 98 x 175, C = 5: ONE ops.export_panels_u8 call writing the all-channel PNG buffers
                    [5, 8, 196, 350, 3] and the grid canvas, against the device work of SegModelBase._eval_outputs for the same
                    bytes: resize + repeat per channel, the frame resize, the concatenation, and export.to_uint8_hwc's mul / add /
                    clamp / permute / cast per sample and channel and for the grid (WITHOUT its copies to the host); device events
  _eval_outputs     the same batch through SegModelBase._eval_outputs with a MaskExporter attached (flushed: every file on disk)
                    against exporter = None, both writing the 40 PNGs and the JPEG into a scratch directory; host clock
  the driver        export_driver.run on a synthetic split of 64 JPEG frames (4 sequences of 16, 480 x 854), random RCF stage-1
                    weights, export_all_seg: frames per second of the loop (first batch to the last file on disk), with and without
                    --sync; --no-driver skips this part
The two legs of a pair ALTERNATE; median [min .. max] of --reps repetitions.  "faster beyond the spread": the slowest repetition of
the new route is faster than the fastest of the other.  Writes the table to --out (default profiles/export_time.txt)."""
import argparse
import copy
import os
import shutil
import sys
import tempfile
import time
import types

ROOT = os.path.join(os.path.dirname(os.path.abspath(__file__)), "..")
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
import numpy as np  # noqa: E402
import torch  # noqa: E402
import yaml  # noqa: E402

import export_cases as xc  # noqa: E402
import rcf_amd  # noqa: E402
from rcf_amd import config, export, export_driver, ops, synth  # noqa: E402
from rcf_amd.model import SegModelBase  # noqa: E402
from time_pwclite import measure, window  # noqa: E402

B, C, H, W, h, w = 8, 5, 392, 697, 98, 175


class Tail(SegModelBase):
    """just the tail of forward_eval"""

    def __init__(self, args):
        super().__init__()
        self._init_dirs(args)
        self.mask_layer, self.align_corners, self.train_iter, self.dist = C, False, 0, None


def spread(name, a, b, unit, lines, names=("exporter", "plain")):
    a, b = sorted(a), sorted(b)
    ma, mb = a[len(a) // 2], b[len(b) // 2]
    lines.append(f"  {name:34s}: {names[0]} {ma:10.2f} [{a[0]:10.2f} .. {a[-1]:10.2f}]   {names[1]} {mb:10.2f} [{b[0]:10.2f} .. {b[-1]:10.2f}] {unit}")
    print(lines[-1], flush=True)
    return a, b


def kernel_legs(masks, frames, dev):
    size = (2 * h, 2 * w)
    sources = [ops.EXPORT_FRAME] + list(range(C))
    Hc, Wc, off, cell_h, cell_w, per_row = export.grid_geometry(B, len(sources) * size[0], size[1])
    png = torch.zeros((C, B) + size + (3,), dtype=torch.uint8, device=dev)
    canvas = torch.zeros((Hc, Wc, 3), dtype=torch.uint8, device=dev)
    layouts = [ops.export_contiguous_layout(png, list(range(C))),
               ops.export_layout(canvas, sources, image=cell_w * 3, image_row=cell_h * Wc * 3, slot=size[0] * Wc * 3, row=Wc * 3, x=off, y=off,
                                 per_row=per_row)]

    def native():
        ops.export_panels_u8(masks, frames, layouts, size, False)
        return png, canvas

    def u8(t):          # export.to_uint8_hwc without the copy to the host
        return export.make_grid(t).mul(255).add_(0.5).clamp_(0, 255).permute(1, 2, 0).to(torch.uint8)

    def route():
        img0 = (ops.resize_nchw(frames.contiguous(), size, False) + 2.0) / 4.0
        vis = [ops.resize_nchw(masks[:, i:i + 1].contiguous(), size, False).repeat(1, 3, 1, 1) for i in range(C)]
        return [[u8(v[b]) for b in range(B)] for v in vis], u8(torch.cat([img0] + vis, 2))

    (p, cv), (rp, rcv) = native(), route()
    assert all(torch.equal(p[c, b], rp[c][b]) for c in range(C) for b in range(B)) and torch.equal(cv, rcv), "the routes differ"
    return native, route, png.numel() + 3 * B * len(sources) * size[0] * size[1]


def tail_times(masks, imgs, dev, reps, lines):
    scratch = tempfile.mkdtemp(prefix="rcf_export_time_")
    args = types.SimpleNamespace(checkpoints_dir=scratch, object_channel=1, eval_save=True, eval_export=True, export_all_seg=True)
    m = Tail(args)
    names = [f"seq{i}" for i in range(B)]
    paths = [[f"/data/JPEGImages/480p/seq{i}/{i:05d}.jpg" for i in range(B)]]
    ids = torch.arange(B)
    exp = export.MaskExporter(dev, workers=8)

    def run(e):
        m.exporter = e
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        m._eval_outputs(imgs, masks, ids, names, paths)
        if e is not None:
            e.flush()
        torch.cuda.synchronize()
        return (time.perf_counter() - t0) * 1e3
    for _ in range(2):
        run(exp), run(None)
    ta, tb = [], []
    for _ in range(reps):
        ta.append(run(exp))
        tb.append(run(None))
    exp.close()
    shutil.rmtree(scratch, ignore_errors=True)
    return spread("_eval_outputs, 40 PNGs + 1 JPEG", ta, tb, "ms per batch, files on disk", lines)


def driver_times(dev, reps, lines):
    from PIL import Image
    root = tempfile.mkdtemp(prefix="rcf_export_drive_")
    data = os.path.join(root, "data")
    rng = np.random.RandomState(0)
    split = []
    for s in range(4):
        os.makedirs(os.path.join(data, "JPEGImages/480p", f"seq{s}"))
        for i in range(16):
            img = rng.randint(0, 256, size=(30, 54, 3)).astype(np.uint8).repeat(16, 0).repeat(16, 1)[:480, :854]
            Image.fromarray(np.ascontiguousarray(img)).save(os.path.join(data, "JPEGImages/480p", f"seq{s}", f"{i:05d}.jpg"), quality=90)
        split.append(f"JPEGImages/480p/seq{s} " + " ".join(f"{i:05d}.jpg" for i in range(16)) + "\n")
    with open(os.path.join(data, "val.txt"), "w") as f:
        f.writelines(split)
    kw = config.stage1_model_kwargs(config.mask_size_for(H, W), mask_layer=C, dropout=0.0, norm="BN")
    cfg = dict(batch_size=B, workers=16, model_cls="RCFModel", model_kwargs=kw, data_path=data, dataset_kwargs={},
               test_dataset_kwargs=dict(frame_num=1, load_flow=False, split="val.txt", zero_ann=True),
               test_transform_kwargs=dict(strong_aug=False), eval_pos_th=0.35, eval_save=True, eval_export=True, export_all_seg=True,
               object_channel=1, checkpoints_dir=root, pretrained_model=None, allow_overwriting_checkpoints_dir=True,
               trainer_kwargs=dict(precision=32))
    cfg_path = os.path.join(root, "export.yaml")
    with open(cfg_path, "w") as f:
        yaml.safe_dump(cfg, f)
    m = rcf_amd.RCFModel(config.load_args(cfg_path), **copy.deepcopy(kw))
    shapes = {k: tuple(v.shape) for k, v in m.state_dict().items()}
    ckpt = os.path.join(root, "run", "last.ckpt")
    os.makedirs(os.path.dirname(ckpt))
    torch.save({"state_dict": {"model." + k: torch.from_numpy(v) for k, v in synth.fill_state_dict(shapes, seed=13).items()}}, ckpt)
    del m

    def run(sync):
        out = export_driver.run([cfg_path, "--test", "--test-override-pretrained", ckpt] + (["--sync"] if sync else []), device=dev)
        return out["frames"] / out["loop_seconds"]
    run(False), run(True)
    ta, tb = [], []
    for _ in range(reps):
        ta.append(run(False))
        tb.append(run(True))
    shutil.rmtree(root, ignore_errors=True)
    a, b = spread("driver, 64 frames of 480 x 854", ta, tb, "frames / s (higher is better)", lines, names=("threads", "--sync"))
    return a, b


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--iters", type=int, default=20)
    ap.add_argument("--reps", type=int, default=7)
    ap.add_argument("--no-driver", action="store_true")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "export_time.txt"))
    args = ap.parse_args()
    if not torch.cuda.is_available():
        sys.exit("time_export.py measures on the GPU; there is none here")
    dev = "cuda:0"
    rng = np.random.RandomState(7)
    masks = torch.from_numpy(xc.softmax_masks(rng, B, C, h, w)).to(dev)
    imgs = torch.from_numpy(np.clip(rng.standard_normal((B, 1, 3, H, W)), -2, 2).astype(np.float32)).to(dev)
    lines = [f"evaluation export, {B} frames of {H} x {W}, masks {h} x {w}, C = {C}; {torch.cuda.get_device_name(0)}; median [min .. max] of "
             f"{args.reps} repetitions, legs alternated"]
    native, route, nbytes = kernel_legs(masks, imgs[:, 0], dev)
    lines.append(f"kernel call: microseconds per call ({args.iters} calls per repetition, device events); {nbytes} bytes written per call")
    got = measure({"export_panels_u8 vs resize+repeat+u8": (native, route)}, args, lines)
    t = sorted(window(native, args.iters) for _ in range(args.reps))
    lines.append(f"  export_panels_u8 alone: {t[len(t) // 2]:.1f} [{t[0]:.1f} .. {t[-1]:.1f}] us = {nbytes / t[len(t) // 2] / 1e3:.1f} GB/s written "
                 f"(median); the bound is the bytes written")
    print(lines[-1], flush=True)
    lines.append("_eval_outputs with a MaskExporter attached (8 writer threads, flushed) against exporter = None:")
    a, b = tail_times(masks, imgs, dev, args.reps, lines)
    lines.append("  exporter faster beyond the spread" if a[-1] < b[0] else "  exporter NOT faster beyond the spread")
    if not args.no_driver:
        lines.append("export_driver.run, loop only (model build and checkpoint load excluded):")
        a, b = driver_times(dev, max(3, args.reps // 2), lines)
        lines.append("  threads faster than --sync beyond the spread" if a[0] > b[-1] else "  threads NOT faster than --sync beyond the spread")
    lines.append("kernel call faster than the route it replaces beyond the spread: " + str(bool(list(got.values())[0])))
    print("\n".join(lines[-3:]))
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as f:
        f.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
