"""The reference's test mode (main.py --test: evaluation and the `pred_seg_*.png` export every offline tool reads) as one batched
driver on one GPU:

    tools/export_masks.py CONFIG [--test] --test-override-pretrained CKPT [--test-override-object-channel N]
                          [--batch-size N] [--workers N] [--sync] [--opts K V ...]

config.load_args -> the model named by `model_cls` -> `load_pretrained` (main.py:76-144) -> the frames of the test split
(`list_eval_frames`: dataset/data.py:12-40,100-112) decoded on threads into BatchUploader staging -> Transform(training=False) on the
device -> Evaluator.test_step per batch with an export.MaskExporter attached to the model -> test_epoch_end and the reference's lines.

Batches.  The reference's DataLoader collates `batch_size` consecutive frames whatever their size (and fails when they differ); here a
batch closes when it is full OR when the next frame's or annotation's size differs, so a split of mixed sizes runs.  The PNGs are per
sample and do not depend on the batching; the evaluation JPEGs are one grid per BATCH named after its first sample, so on such a split
their set differs from a fixed-size loader's.
"""
import argparse
import copy
import glob
import os
import time
from concurrent.futures import ThreadPoolExecutor

import numpy as np
import torch

from . import config, ops
from .data_pipeline import BatchUploader, get_transform
from .evaluate import Evaluator
from .export import MaskExporter

MAX_WORKERS = 16


# ---------------------------------------------------------------------------------------------------------------- checkpoint
def load_pretrained(model, path, args, log=print):
    """main.py:76-144 for a bare model (the reference loads into its LightningModule, whose keys carry a `model.` prefix).
    Formats: `model.`-prefixed main checkpoints (duplicated into the `*_ema` modules when the model has them and the file does not;
    `drop_head_decode_head2`), MoCo (`module.encoder_q.`) and DenseCL (`conv1.weight`) backbones, un-prefixed main models
    (`backbone2.conv1.weight`); `pretrained_model_backbone_only` keeps the keys that name a backbone.  Returns (path, mismatches)."""
    if "*" in path:
        matches = glob.glob(path)
        assert len(matches) == 1, f"{matches} is not unique"
        path = matches[0]
    log(f"Loading pretrained model from {path}")
    ckpt = torch.load(path, map_location="cpu")
    state_dict = ckpt["state_dict"] if "state_dict" in ckpt else ckpt
    if getattr(args, "pretrained_model_backbone_only", False):
        state_dict = {k: v for k, v in state_dict.items() if "backbone" in k}
    example_key = list(state_dict.keys())[0]
    ema_loaded = False
    ema_in_model = getattr(model, "backbone2_ema", None) is not None
    if example_key.startswith("model."):
        ema_in_state_dict = len([k for k in state_dict if "_ema" in k])
        if ema_in_model and not ema_in_state_dict:
            assert model.decode_head2_ema is not None, "decode_head2_ema is not enabled with backbone2_ema enabled"
            log("Detected EMA in model but not in state_dict, loading state_dict to both the main model and ema")
            ema_state_dict = {k.replace("backbone2", "backbone2_ema").replace("decode_head2", "decode_head2_ema"): v
                              for k, v in state_dict.items() if "backbone2" in k or "decode_head2" in k}
            state_dict = {**state_dict, **ema_state_dict}
        if getattr(args, "drop_head_decode_head2", False):
            log("Dropping decode_head2 (with ema)")
            state_dict = {k: v for k, v in state_dict.items() if "decode_head2" not in k}
        # the LightningModule's strict=False load: its only child is `model`, every other key is reported as unexpected
        inner = {k[len("model."):]: v for k, v in state_dict.items() if k.startswith("model.")}
        mismatches = model.load_state_dict(inner, strict=False)
        ema_loaded = True
    elif example_key.startswith("module."):
        prefix = "module.encoder_q"
        state_dict = {k[len(prefix) + 1:]: v for k, v in state_dict.items()
                      if k.startswith(prefix) and not k.startswith(prefix + ".fc")}
        mismatches = model.backbone2.load_state_dict(state_dict, strict=False)
    elif "conv1.weight" in state_dict:
        mismatches = model.backbone2.load_state_dict(state_dict, strict=False)
    elif "backbone2.conv1.weight" in state_dict:
        mismatches = model.load_state_dict(state_dict, strict=False)
    else:
        raise ValueError("Unknown module in state_dict")
    if not ema_loaded:
        assert getattr(model, "backbone2_ema", None) is None and getattr(model, "decode_head2_ema", None) is None, \
            "EMA is enabled but weights are not loaded"
    ops.weights_changed()
    log(f"Mismatches in the pretrained model: {mismatches}")
    return path, mismatches


# -------------------------------------------------------------------------------------------------------------------- frames
def list_eval_frames(root, split, subsample_frame_interval=None, zero_ann=False):
    """dataset/data.py:12-40,100-112 in evaluation mode: the split's lines sorted, `name frame frame ...` per line; -1 keeps the first
    frame of a sequence, n > 0 every n-th.  -> [(seq_id, seq_name, frame path, annotation path or None)] in loader order; the
    annotation is the frame path with JPEGImages -> Annotations and .jpg -> .png, None (a 1 x 1 zero) with zero_ann."""
    with open(os.path.join(root, split)) as f:
        lines = f.readlines()
    lines.sort()
    out = []
    for seq_id, line in enumerate(lines):
        parts = line.split()
        seq, frames = parts[0], parts[1:]
        if subsample_frame_interval == -1:
            frames = frames[:1]
        elif subsample_frame_interval is not None:
            frames = frames[::subsample_frame_interval]
        name = seq.rstrip("/").split("/")[-1]
        for fr in frames:
            p = os.path.join(root, seq, fr)
            out.append((seq_id, name, p, None if zero_ann else p.replace("JPEGImages", "Annotations").replace(".jpg", ".png")))
    return out


def _image_size(path):
    from PIL import Image
    with Image.open(path) as im:
        return im.size[::-1]                 # (H, W); only the header is read


def plan_batches(frames, batch_size, sizes):
    """consecutive runs of at most batch_size frames with one (frame size, annotation size): [[index, ...], ...]"""
    batches, cur = [], []
    for i in range(len(frames)):
        if cur and (len(cur) == batch_size or sizes[i] != sizes[cur[0]]):
            batches.append(cur)
            cur = []
        cur.append(i)
    if cur:
        batches.append(cur)
    return batches


class EvalLoader:
    """The test DataLoader: decode threads fill BatchUploader staging (one uploader per frame size), one batch ahead of the model;
    Transform(training=False) runs on the device; `ann` is channel 0 of the annotation as uint8 [B, Ha, Wa]."""

    def __init__(self, frames, batch_size, transform, device, workers):
        self.frames, self.B, self.transform, self.device = frames, int(batch_size), transform, torch.device(device)
        self.pool = ThreadPoolExecutor(max_workers=max(1, min(int(workers), MAX_WORKERS)), thread_name_prefix="rcf-decode")
        fs = list(self.pool.map(lambda f: _image_size(f[2]), frames))
        an = list(self.pool.map(lambda f: (1, 1) if f[3] is None else _image_size(f[3]), frames))
        self.sizes = list(zip(fs, an))
        self.batches = plan_batches(frames, self.B, self.sizes)
        self.uploaders = {}

    def __len__(self):
        return len(self.batches)

    @staticmethod
    def _decode(path, convert, out):
        from PIL import Image
        with open(path, "rb") as f:
            out[...] = np.asarray(Image.open(f).convert(convert))

    def _fill(self, idx):
        (H, W), (Ha, Wa) = self.sizes[idx[0]]
        up = self.uploaders.get((H, W))
        if up is None:
            up = self.uploaders[(H, W)] = BatchUploader(self.B, 1, H, W, has_flow=False, device=self.device)
        stage = up.stage()
        ann = np.zeros((len(idx), Ha, Wa, 3), dtype=np.uint8)
        jobs = []
        for b, i in enumerate(idx):
            jobs.append(self.pool.submit(self._decode, self.frames[i][2], "RGB", stage["imgs"][b, 0]))
            if self.frames[i][3] is not None:
                jobs.append(self.pool.submit(self._decode, self.frames[i][3], "RGB", ann[b]))
        return up, ann, jobs

    def _finish(self, idx, filled):
        up, ann, jobs = filled
        for j in jobs:
            j.result()
        data = up.upload()
        n = len(idx)
        data["imgs"] = data["imgs"][:n]
        batch = self.transform(data)
        batch["ann"] = torch.from_numpy(np.ascontiguousarray(ann[..., 0])).to(self.device)
        batch["seq_ids"] = torch.tensor([self.frames[i][0] for i in idx])
        batch["seq_names"] = [self.frames[i][1] for i in idx]
        batch["paths"] = [[self.frames[i][2] for i in idx]]
        return batch

    def __iter__(self):
        filled = self._fill(self.batches[0]) if self.batches else None
        for k, idx in enumerate(self.batches):
            batch = self._finish(idx, filled)
            if k + 1 < len(self.batches):
                filled = self._fill(self.batches[k + 1])         # decoded while the model runs batch k
            yield batch

    def close(self):
        self.pool.shutdown(wait=True)


# -------------------------------------------------------------------------------------------------------------------- driver
def parse_args(argv=None):
    p = argparse.ArgumentParser(description="Evaluate and export masks (the reference's main.py --test).")
    p.add_argument("config", type=str, help="path to config")
    p.add_argument("--test", action="store_true", default=False, help="accepted and implied")
    p.add_argument("--test-override-pretrained", default=None, type=str,
                   help="override pretrained model and checkpoints directory at test")
    p.add_argument("--test-override-object-channel", default=None, type=int, help="override object channel at test")
    p.add_argument("--batch-size", default=None, type=int, help="frames per batch (default: the config's batch_size)")
    p.add_argument("--workers", default=None, type=int, help=f"decode / writer threads (default: the config's workers; at most {MAX_WORKERS})")
    p.add_argument("--sync", action="store_true", default=False, help="write every batch's files inline (debugging, A/B)")
    p.add_argument("--opts", default=[], nargs=argparse.REMAINDER, help="config overrides as KEY VALUE pairs")
    return p.parse_args(argv)


PRECISION = {32: None, "32": None, 16: "fp16", "16": "fp16", "bf16": "bf16"}        # Lightning `precision:` -> model.precision


def build_model(args, device):
    from . import AMDModel, RCFModel
    classes = dict(RCFModel=RCFModel, AMDModel=AMDModel)
    name = getattr(args, "model_cls", "RCFModel")
    if name not in classes:
        raise NotImplementedError(f"model_cls {name}")
    model = classes[name](args, **copy.deepcopy(args.model_kwargs))         # (the constructors pop from the component dicts)
    prec = (getattr(args, "trainer_kwargs", None) or {}).get("precision", 32)
    if prec not in PRECISION:
        raise ValueError(f"trainer_kwargs.precision {prec!r}")
    model.precision = PRECISION[prec]
    return model.to(device)


def prepare_args(cli):
    """main.py:420,448-466,148-152: the config, the overrides of test mode, the object channel (config, else $OBJECT_CHANNEL)"""
    args = config.load_args(cli.config, cli_opts=cli.opts)
    args.config_path, args.test, args.rank, args.multi_gpu = cli.config, True, -1, False
    if cli.test_override_pretrained is not None:
        args.pretrained_model = cli.test_override_pretrained
        args.checkpoints_dir = os.path.dirname(args.pretrained_model)
        print(f"Overriding pretrained_model to {args.pretrained_model}")
    if cli.test_override_object_channel is not None:
        args.object_channel = cli.test_override_object_channel
        print(f"Overriding object channel to {args.object_channel}")
    oc = args.object_channel if getattr(args, "object_channel", None) is not None else os.environ.get("OBJECT_CHANNEL", None)
    args.object_channel = int(oc) if isinstance(oc, str) else oc
    print(f"Using {args.object_channel} as object channel")
    return args


def make_dirs(args):
    """main.py:49-59 in test mode (no `saved/`)"""
    ok = bool(getattr(args, "allow_overwriting_checkpoints_dir", False))
    os.makedirs(args.checkpoints_dir, exist_ok=ok)
    os.makedirs(os.path.join(args.checkpoints_dir, getattr(args, "saved_eval_dir_name", "saved_eval")), exist_ok=ok)
    os.makedirs(os.path.join(args.checkpoints_dir, getattr(args, "saved_eval_export_dir_name", "saved_eval_export")), exist_ok=ok)


def report_lines(args, evaluator, name="test_miou"):
    """test_epoch_end (main.py:240-292) and the lines it logs"""
    lines = []
    had_channel = evaluator.object_channel is not None
    mean_miou, frame_avg, per_seq = evaluator.test_epoch_end(testing=True)
    if not had_channel:
        lines.append(f"Rank {args.rank}: Set object channel to {evaluator.object_channel} "
                     f"(Max channel distribution at local rank: {evaluator.max_channel_freq})")
    lines += [f"{name}_{seq}: {miou * 100.:.2f}" for seq, miou in per_seq.items()]
    lines += [f"{name}: {mean_miou * 100.:.2f}", f"{name}_frame_avg: {frame_avg * 100.:.2f}"]
    return lines, (mean_miou, frame_avg, per_seq)


def run(argv=None, device="cuda:0"):
    cli = parse_args(argv)
    if int(os.environ.get("LOCAL_RANK", "-1")) > -1:
        raise AssertionError("Testing with multi-GPUs is unsupported.")             # main.py:453-454
    if not torch.cuda.is_available():
        raise RuntimeError("export_masks needs the GPU: there is no CPU path")
    args = prepare_args(cli)
    batch_size = cli.batch_size if cli.batch_size is not None else args.batch_size
    workers = min(cli.workers if cli.workers is not None else getattr(args, "workers", 4), MAX_WORKERS)
    make_dirs(args)
    torch.cuda.set_device(device)
    model = build_model(args, device)
    if getattr(args, "pretrained_model", None) is not None:
        load_pretrained(model, args.pretrained_model, args)
    else:
        print("Not loading pretrained model")
    model.eval()
    kw = dict(getattr(args, "dataset_kwargs", None) or {}, **(getattr(args, "test_dataset_kwargs", None) or {}))
    assert kw.get("frame_num", 1) == 1, f"You need single frames for evaluaion but have {kw.get('frame_num')} frames"
    root = getattr(args, "test_data_path", None) or args.data_path
    frames = list_eval_frames(root, kw["split"], kw.get("subsample_frame_interval"), kw.get("zero_ann", False))
    loader = EvalLoader(frames, batch_size, get_transform(args, training=False), device, workers)
    exporter = MaskExporter(device, workers=workers, sync=cli.sync)
    model.exporter = exporter
    evaluator = Evaluator(args, args.model_kwargs["mask_layer"])
    t0 = time.perf_counter()
    try:
        for batch in loader:
            evaluator.test_step(model, batch)
        lines, result = report_lines(args, evaluator)
    finally:
        exporter.close()                     # everything is on disk
        seconds = time.perf_counter() - t0
        loader.close()
        model.exporter = None
    for line in lines:
        print(line)
    return dict(lines=lines, result=result, frames=len(frames), batches=len(loader), args=args, loop_seconds=seconds)


def main(argv=None):
    run(argv)
