"""SegTrackv2 / FBMS59 mIoU of exported pred_seg_*.png masks (the reference's tools/STv2-FBMS59-evaluation/eval_tool.py).

Per annotated frame the reference opens the exported mask, resizes it to the annotation's size with Pillow's default filter
(an antialiased bicubic in 8-bit fixed point), thresholds it at 0.35 and the annotation at 0.5, and forms an IoU.  Here the
resize, both comparisons and the two sums run in one device call per run of consecutive frames with the same sizes
(rcf_amd.pilresize.resize_iou_counts: Pillow's integers, bit for bit); the host reads the files, derives the integer
threshold, divides the counts and prints the reference's three kinds of lines.  Masks Pillow does not resample that way
(palette, 1-bit, alpha: other modes than L and RGB) and reductions beyond the kernel's window go through Pillow itself.
"""
import argparse
import os
import warnings

import numpy as np

POS_TH = 0.35
DATASETS = {
    # dataset -> (directory under --data_dir, list file, skip frames without annotation, annotations are .png)
    "SegTrackv2": ("data_SegTrackv2", "trainval.txt", False, False),
    "FBMS59": ("data_fbms59", "val_all.txt", True, True),      # the val list names whole sequences; few frames are annotated
}


def pred_min_for(pos_th=POS_TH):
    """the smallest u8 v with v / 255. > pos_th, in the reference's float64 expression (256: none)"""
    return next((v for v in range(256) if v / 255. > pos_th), 256)


def iou_from_counts(c):
    """eval_tool.py iou(): i.sum() / u.sum() on int64, nan on an empty union"""
    inter, union = np.int64(c[0]), np.int64(c[1])
    if union == 0:
        return float("nan")
    return inter / union


def read_annotation(path):
    """u8 [H,W] 0 / 1: np.array(Image.open(path)) / 255. > 0.5 in float64 on whatever dtype Pillow returns; channel 0 of a
    3-D array"""
    from PIL import Image
    annotation = np.array(Image.open(path)) / 255.
    if annotation.ndim == 3:
        annotation = annotation[..., 0]
    return (annotation > 0.5).astype(np.uint8)


def pillow_counts(img, annotation, pred_min):
    """one frame through Pillow on the host: the reference's lines, with the comparison on integers"""
    pred = np.array(img.resize((annotation.shape[1], annotation.shape[0])))
    if pred.ndim == 3:
        pred = pred[..., 0]
    if pred.dtype != np.uint8:                   # bool / wider integers: the reference's float comparison itself
        p = pred / 255. > POS_TH
    else:
        p = pred >= pred_min
    a = annotation != 0
    assert a.shape == p.shape, f"{a.shape} != {p.shape}"
    return np.array([(p & a).sum(), (p | a).sum()], dtype=np.int64)


class _Batcher:
    """collects consecutive frames of one geometry and mode, and scores them with one device call"""

    def __init__(self, batch_frames, pred_min, ious, routes):
        self.batch_frames, self.pred_min, self.ious, self.routes = batch_frames, pred_min, ious, routes
        self.key, self.items = None, []

    def add(self, slot, pred, annotation):
        key = (pred.shape, annotation.shape)
        if self.key != key or len(self.items) >= self.batch_frames:
            self.flush()
        self.key = key
        self.items.append((slot, pred, annotation))

    def flush(self):
        if not self.items:
            return
        from . import pilresize
        preds = np.stack([p for _, p, _ in self.items])
        anns = np.stack([a for _, _, a in self.items])
        counts = pilresize.resize_iou_counts(preds, anns, self.pred_min)
        for (slot, _, _), c in zip(self.items, counts):
            self.ious[slot] = iou_from_counts(c)
        self.routes["device_calls"] += 1
        self.key, self.items = None, []


def evaluate(dataset, pred_dir, step=0, data_dir="data", batch_frames=16, host=False):
    """-> {"sequences": [(name, mIoU)], "ious": per-frame IoUs in list order, "miou", "n_frames",
    "routes": {"device": frames, "pillow": frames, "device_calls": calls}}"""
    from PIL import Image
    sub, list_name, allow_skipping_gt, use_png = DATASETS[dataset]
    data_root = os.path.join(data_dir, sub)
    with open(os.path.join(data_root, list_name), "r") as f:
        seqs = f.readlines()
    pred_min = pred_min_for()
    if not host:
        from . import pilresize
    all_ious, seq_slices = [], []
    routes = {"device": 0, "pillow": 0, "device_calls": 0}
    batcher = _Batcher(max(1, int(batch_frames)), pred_min, all_ious, routes)
    for seq in seqs:
        seq = seq.rstrip().split()
        seq_dir = seq[0].replace("JPEGImages", "Annotations")
        seq_name = seq_dir.split("/")[-2]
        start = len(all_ious)
        for frame_ind, frame in enumerate(seq[1:]):
            path = os.path.join(data_root, seq_dir, frame)
            if use_png:
                path = path.replace(".jpg", ".png")
            if not os.path.exists(path):
                assert allow_skipping_gt, f"{path} does not exist, but skipping ground truth is not allowed"
                continue
            annotation = read_annotation(path)
            img = Image.open(os.path.join(pred_dir, f"pred_seg_{seq_name}_{frame_ind:05}_{step:07}.png"))
            H, W = annotation.shape
            on_device = not host and img.mode in ("L", "RGB") and pilresize.device_ok(img.size[1], H)
            all_ious.append(None)
            if on_device:
                batcher.add(len(all_ious) - 1, np.array(img), annotation)
                routes["device"] += 1
            else:
                all_ious[-1] = iou_from_counts(pillow_counts(img, annotation, pred_min))
                routes["pillow"] += 1
        seq_slices.append((seq_name, start, len(all_ious)))
    batcher.flush()
    with warnings.catch_warnings():
        warnings.simplefilter("ignore", category=RuntimeWarning)      # a sequence of nans / without annotations: nan, as printed
        sequences = [(name, np.nanmean(all_ious[a:b])) for name, a, b in seq_slices]
        miou = np.nanmean(all_ious)
    return {"sequences": sequences, "ious": all_ious, "miou": miou, "n_frames": len(all_ious), "routes": routes}


def report_lines(res):
    """the reference tool's output"""
    return [f"mIoU on {name}: {v * 100:.2f}" for name, v in res["sequences"]] + \
        [f"mIoU: {res['miou'] * 100:.2f}", f"Number of frames: {res['n_frames']}"]


def parse_args(argv=None):
    parser = argparse.ArgumentParser(description="SegTrackv2 / FBMS59 mIoU of exported masks")
    parser.add_argument("--dataset", choices=["SegTrackv2", "FBMS59"], required=True,
                        help="Dataset: either SegTrackv2 (resized training output) or FBMS59 (resized training output)")
    parser.add_argument("--step", type=int, default=0,
                        help="The step to evaluate, should use 0 if you export with the export config.")
    parser.add_argument("--pred_dir", type=str, required=True,
                        help="Prediction directory (the directory which includes the prediction masks directly, often with "
                             "the name of a channel index)")
    parser.add_argument("--data_dir", type=str, default="data", help="the folder that holds data_SegTrackv2 / data_fbms59")
    parser.add_argument("--batch-frames", type=int, default=16, help="most frames per device call")
    parser.add_argument("--host", action="store_true", help="resize with Pillow on the host: no device call")
    return parser.parse_args(argv)


def main(argv=None):
    """python tools/stv2_fbms_eval.py --dataset FBMS59 --step 0 --pred_dir <exp dir>/saved_eval_export/0 [--data_dir data]"""
    args = parse_args(argv)
    res = evaluate(args.dataset, args.pred_dir, step=args.step, data_dir=args.data_dir, batch_frames=args.batch_frames,
                   host=args.host)
    for line in report_lines(res):
        print(line)
    return res
