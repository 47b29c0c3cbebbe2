"""DAVIS-2016/2017 evaluation (the reference's tools/davis2016-evaluation: davis2017/{metrics,utils,davis,results,
evaluation}.py and evaluation_method.py) with the boundary measure on the device.

The only costly part of the tool, the per-frame boundary F-measure (two boundary maps, each dilated by a disk of
radius ceil(0.008 * diagonal)), and the per-frame region counts run in ONE kernel per (proposal, object) pair and
sequence (csrc/davis_eval.hip) that returns integer counts.  Everything else -- precision, recall, J, F, the statistics,
the assignment of proposals to objects, the CSV tables -- is the reference's float64 arithmetic on those integers, in the
reference's order, so every figure matches it bit for bit.  No cv2, skimage or pandas is needed.
"""
import argparse
import csv
import io
import os
import sys
import time
import warnings
from collections import defaultdict
from glob import glob

import numpy as np
import torch

from . import _lib
from .ops import _p, _stream

MAX_RADIUS = 64          # csrc/davis_eval.hip RMAX
POS_TH = 0.35            # davis2017/results.py: threshold on the exported mask


def radius_for(H, W, bound_th=0.008):
    """f_measure's bound_pix: bound_th pixels when bound_th >= 1, else ceil(bound_th * |(H, W)|) in float64"""
    if bound_th >= 1:
        if float(bound_th) != int(bound_th):
            raise ValueError(f"bound_th = {bound_th} >= 1 is a radius in pixels and must be an integer")
        r = int(bound_th)
    else:
        r = int(np.ceil(bound_th * np.linalg.norm((H, W))))
    if r < 0 or r > MAX_RADIUS:
        raise ValueError(f"boundary radius {r} (bound_th {bound_th}, frame {H}x{W}) is outside [0, {MAX_RADIUS}]")
    return r


def _as_u8_frames(a, device):
    t = a if isinstance(a, torch.Tensor) else torch.from_numpy(np.ascontiguousarray(np.asarray(a)))
    if t.dim() == 2:
        t = t.unsqueeze(0)
    if t.dim() != 3:
        raise ValueError(f"masks must be [N,H,W] or [H,W], got shape {tuple(t.shape)}")
    if t.dtype != torch.uint8:
        t = t != 0
    return t.to(device=device, dtype=torch.uint8).contiguous()


def boundary_counts(pred, gt, void=None, bound_th=0.008):
    """pred, gt (, void): [N,H,W] or [H,W] torch / numpy, bool or uint8 (nonzero = on) -> int64 numpy [N,6]:
    inter, union, n_fg, n_gt, fg_match, gt_match per frame over the non-void pixels (one device call)"""
    dev = next((t.device for t in (pred, gt, void) if isinstance(t, torch.Tensor) and t.is_cuda), None)
    dev = dev or torch.device("cuda", torch.cuda.current_device())
    p, g = _as_u8_frames(pred, dev), _as_u8_frames(gt, dev)
    v = None if void is None else _as_u8_frames(void, dev)
    if p.shape != g.shape or (v is not None and v.shape != p.shape):
        raise ValueError(f"shape mismatch: pred {tuple(p.shape)}, gt {tuple(g.shape)}"
                         + ("" if v is None else f", void {tuple(v.shape)}"))
    N, H, W = p.shape
    r = radius_for(H, W, bound_th)
    counts = torch.zeros((N, 6), dtype=torch.int64, device=dev)
    with torch.cuda.device(dev):
        _lib.call("rcf_davis_counts_u8", _p(p), _p(g), _p(v), N, H, W, r, _p(counts), _stream())
    return counts.cpu().numpy()


# ---- float64 measures from the counts (davis2017/metrics.py expressions and empty-case rules) --------------------------

def _j_from_counts(c):
    """db_eval_iou: inters / union, 1 where the union is 0"""
    inters, union = c[:, 0], c[:, 1]
    with np.errstate(divide="ignore", invalid="ignore"):
        j = inters / union
    j[np.isclose(union, 0)] = 1
    return j


def _f_from_counts(n_fg, n_gt, fg_match, gt_match):
    """the tail of f_measure on one frame's integers"""
    n_fg, n_gt = np.int64(n_fg), np.int64(n_gt)
    if n_fg == 0 and n_gt > 0:
        precision, recall = 1, 0
    elif n_fg > 0 and n_gt == 0:
        precision, recall = 0, 1
    elif n_fg == 0 and n_gt == 0:
        precision, recall = 1, 1
    else:
        precision = np.uint64(fg_match) / float(n_fg)
        recall = np.uint64(gt_match) / float(n_gt)
    if precision + recall == 0:
        return 0
    return 2 * precision * recall / (precision + recall)


def _check_void(annotation, void_pixels):
    if void_pixels is not None:
        assert np.shape(annotation) == np.shape(void_pixels), \
            f"Annotation({np.shape(annotation)}) and void pixels:{np.shape(void_pixels)} dimensions do not match."


def db_eval_iou(annotation, segmentation, void_pixels=None):
    """region similarity J: a float for [H,W] masks, an array over the leading dimensions otherwise"""
    shape = np.shape(annotation)
    assert shape == np.shape(segmentation), \
        f"Annotation({shape}) and segmentation:{np.shape(segmentation)} dimensions do not match."
    _check_void(annotation, void_pixels)
    lead = shape[:-2]
    flat = lambda a: None if a is None else np.reshape(np.asarray(a), (-1,) + tuple(shape[-2:]))
    c = boundary_counts(flat(segmentation), flat(annotation), flat(void_pixels))
    if len(lead) == 0:
        inters, union = c[0, 0], c[0, 1]
        j = inters / union if union != 0 else np.float64("nan")
        return 1 if np.isclose(union, 0) else j
    return _j_from_counts(c).reshape(lead)


def f_measure(foreground_mask, gt_mask, void_pixels=None, bound_th=0.008):
    """boundary F-measure of one [H,W] frame"""
    assert np.atleast_3d(foreground_mask).shape[2] == 1
    c = boundary_counts(foreground_mask, gt_mask, void_pixels, bound_th)[0]
    return _f_from_counts(*c[2:6])


def db_eval_boundary(annotation, segmentation, void_pixels=None, bound_th=0.008):
    """boundary F per frame ([N,H,W] -> float64 [N]) or of one [H,W] frame"""
    assert np.shape(annotation) == np.shape(segmentation)
    if void_pixels is not None:
        assert np.shape(annotation) == np.shape(void_pixels)
    ndim = len(np.shape(annotation))
    if ndim == 3:
        c = boundary_counts(segmentation, annotation, void_pixels, bound_th)
        f_res = np.zeros(c.shape[0])
        for frame_id in range(c.shape[0]):
            f_res[frame_id] = _f_from_counts(*c[frame_id, 2:6])
        return f_res
    if ndim == 2:
        return f_measure(segmentation, annotation, void_pixels, bound_th=bound_th)
    raise ValueError(f"db_eval_boundary does not support tensors with {ndim} dimensions")


def db_statistics(per_frame_values):
    """mean, recall (fraction > 0.5) and decay (first quarter minus last quarter) of a per-frame measure, nan-aware"""
    with warnings.catch_warnings():
        warnings.simplefilter("ignore", category=RuntimeWarning)
        M = np.nanmean(per_frame_values)
        O = np.nanmean(per_frame_values > 0.5)
    N_bins = 4
    ids = np.round(np.linspace(1, len(per_frame_values), N_bins + 1) + 1e-10) - 1
    ids = ids.astype(np.uint8)            # as the reference: wraps past 255 frames
    D_bins = [per_frame_values[ids[i]:ids[i + 1] + 1] for i in range(0, 4)]
    with warnings.catch_warnings():
        warnings.simplefilter("ignore", category=RuntimeWarning)
        D = np.nanmean(D_bins[0]) - np.nanmean(D_bins[3])
    return M, O, D


# ---- dataset and results readers (davis2017/davis.py, davis2017/results.py) -------------------------------------------

def _read_png(path):
    from PIL import Image
    return np.array(Image.open(path))


class DAVIS:
    SUBSET_OPTIONS = ["train", "val", "test-dev", "test-challenge"]
    TASKS = ["semi-supervised", "unsupervised"]
    YEARS = ["2016", "2017", "2019"]
    DATASET_WEB = "https://davischallenge.org/davis2017/code.html"

    def __init__(self, root, task="unsupervised", subset="val", sequences="all", resolution="480p", codalab=False,
                 year="2017", step=0):
        if subset not in self.SUBSET_OPTIONS:
            raise ValueError(f"Subset should be in {self.SUBSET_OPTIONS}")
        if task not in self.TASKS:
            raise ValueError(f"The only tasks that are supported are {self.TASKS}")
        if year not in self.YEARS:
            raise ValueError(f"Year should be one of the following {self.YEARS}")
        self.task, self.subset, self.root, self.step, self.year = task, subset, root, step, year
        self.img_path = os.path.join(root, "JPEGImages", resolution)
        self.mask_path = os.path.join(root, "Annotations", resolution)
        if year == "2019" and not (task == "unsupervised" and subset in ("test-dev", "test-challenge")):
            raise ValueError("Set 'task' to 'unsupervised' and subset to 'test-dev' or 'test-challenge'")
        self.imagesets_path = os.path.join(root, "ImageSets", resolution)
        self._check_directories()
        if sequences == "all":
            with open(os.path.join(self.imagesets_path, f"{subset}.txt")) as f:
                tmp = f.readlines()
            names = set(x.strip().split("/")[3] for x in tmp)
        else:
            names = sequences if isinstance(sequences, list) else [sequences]
        self.sequences = defaultdict(dict)
        for seq in sorted(names):
            images = np.sort(glob(os.path.join(self.img_path, seq, "*.jpg"))).tolist()
            if len(images) == 0 and not codalab:
                raise FileNotFoundError(f"Images for sequence {seq} not found.")
            self.sequences[seq]["images"] = images
            masks = np.sort(glob(os.path.join(self.mask_path, seq, "*.png"))).tolist()
            masks.extend([-1] * (len(images) - len(masks)))
            self.sequences[seq]["masks"] = masks

    def _check_directories(self):
        if not os.path.exists(self.root):
            raise FileNotFoundError(f"DAVIS not found in the specified directory, download it from {self.DATASET_WEB}")
        if not os.path.exists(os.path.join(self.imagesets_path, f"{self.subset}.txt")):
            raise FileNotFoundError(f"Subset sequences list for {self.subset} not found, download the missing subset "
                                    f"for the {self.task} task from {self.DATASET_WEB}")
        if self.subset in ["train", "val"] and not os.path.exists(self.mask_path):
            raise FileNotFoundError(f"Annotations folder for the {self.task} task not found, download it from {self.DATASET_WEB}")

    def get_all_masks(self, sequence, separate_objects_masks=False):
        paths = self.sequences[sequence]["masks"]
        first = _read_png(paths[0])
        masks = np.zeros((len(paths), *first.shape))
        masks_id = []
        for i, path in enumerate(paths):
            masks[i, ...] = _read_png(path)
            masks_id.append("".join(path.split("/")[-1].split(".")[:-1]))
        masks_void = np.zeros_like(masks)
        if separate_objects_masks:
            num_objects = int(np.max(masks[0, ...]))
            tmp = np.ones((num_objects, *masks.shape)) * np.arange(1, num_objects + 1)[:, None, None, None]
            masks = (tmp == masks[None, ...]) > 0
        else:                                     # single object (DAVIS 2016)
            masks = np.expand_dims(masks, axis=0) > 0
        return masks, masks_void, masks_id

    def get_sequences(self):
        yield from self.sequences


class Results:
    def __init__(self, root_dir, step=0):
        self.root_dir, self.step = root_dir, step

    def _read_mask(self, sequence, frame_id):
        from PIL import Image
        path = os.path.join(self.root_dir, f"pred_seg_{sequence}_{frame_id}_{self.step:07}.png")
        if not os.path.exists(path):
            query = os.path.join(self.root_dir, f"pred_seg_{sequence}_*_{frame_id}_{self.step:07}.png")
            found = glob(query)
            if len(found) != 1:
                raise FileNotFoundError(
                    f"{sequence} frame {frame_id} not found! ({query} matches {len(found)} files)\n"
                    "The frames have to be indexed PNG files placed inside the corespondent sequence folder.\n"
                    "The indexes have to match with the initial frame.")
            path = found[0]
        arr = np.array(Image.open(path).resize(size=(854, 480), resample=Image.BILINEAR))
        return arr[..., 0] if arr.ndim == 3 else arr

    def read_masks(self, sequence, masks_id):
        mask_0 = self._read_mask(sequence, masks_id[0])
        masks = np.zeros((len(masks_id), *mask_0.shape))
        for ii, m in enumerate(masks_id):
            masks[ii, ...] = (self._read_mask(sequence, m) > 256 * POS_TH).astype(np.uint8)
        num_objects = int(np.max(masks))
        tmp = np.ones((num_objects, *masks.shape)) * np.arange(1, num_objects + 1)[:, None, None, None]
        return (tmp == masks[None, ...]) > 0


# ---- evaluation (davis2017/evaluation.py) -----------------------------------------------------------------------------

def _j_f(gt, res, void, metric):
    """J and F per frame of one (object, proposal) pair: one device call"""
    if void is not None and not np.any(void):
        void = None
    c = boundary_counts(res, gt, void)
    j = _j_from_counts(c) if "J" in metric else None
    f = np.array([_f_from_counts(*row[2:6]) for row in c], dtype=np.float64) if "F" in metric else None
    return j, f


class DAVISEvaluation:
    def __init__(self, davis_root, task, gt_set, sequences="all", codalab=False, year="2017", step=0):
        self.davis_root, self.task, self.year, self.step = davis_root, task, year, step
        self.dataset = DAVIS(root=davis_root, task=task, subset=gt_set, sequences=sequences, codalab=codalab, year=year,
                             step=step)

    @staticmethod
    def _evaluate_semisupervised(all_gt_masks, all_res_masks, all_void_masks, metric):
        if all_res_masks.shape[0] > all_gt_masks.shape[0]:
            raise ValueError("In your PNG files there is an index higher than the number of objects in the sequence!")
        elif all_res_masks.shape[0] < all_gt_masks.shape[0]:
            zero_padding = np.zeros((all_gt_masks.shape[0] - all_res_masks.shape[0], *all_res_masks.shape[1:]))
            all_res_masks = np.concatenate([all_res_masks, zero_padding], axis=0)
        j_metrics_res, f_metrics_res = np.zeros(all_gt_masks.shape[:2]), np.zeros(all_gt_masks.shape[:2])
        for ii in range(all_gt_masks.shape[0]):
            j, f = _j_f(all_gt_masks[ii], all_res_masks[ii], all_void_masks, metric)
            if "J" in metric:
                j_metrics_res[ii, :] = j
            if "F" in metric:
                f_metrics_res[ii, :] = f
        return j_metrics_res, f_metrics_res

    @staticmethod
    def _evaluate_unsupervised(all_gt_masks, all_res_masks, all_void_masks, metric, max_n_proposals=20):
        from scipy.optimize import linear_sum_assignment
        if all_res_masks.shape[0] > max_n_proposals:
            raise ValueError(f"In your PNG files there is an index higher than the maximum number ({max_n_proposals}) "
                             "of proposals allowed!")
        elif all_res_masks.shape[0] < all_gt_masks.shape[0]:
            zero_padding = np.zeros((all_gt_masks.shape[0] - all_res_masks.shape[0], *all_res_masks.shape[1:]))
            all_res_masks = np.concatenate([all_res_masks, zero_padding], axis=0)
        j_metrics_res = np.zeros((all_res_masks.shape[0], all_gt_masks.shape[0], all_gt_masks.shape[1]))
        f_metrics_res = np.zeros((all_res_masks.shape[0], all_gt_masks.shape[0], all_gt_masks.shape[1]))
        for ii in range(all_gt_masks.shape[0]):
            for jj in range(all_res_masks.shape[0]):
                j, f = _j_f(all_gt_masks[ii], all_res_masks[jj], all_void_masks, metric)
                if "J" in metric:
                    j_metrics_res[jj, ii, :] = j
                if "F" in metric:
                    f_metrics_res[jj, ii, :] = f
        if "J" in metric and "F" in metric:
            all_metrics = (np.mean(j_metrics_res, axis=2) + np.mean(f_metrics_res, axis=2)) / 2
        else:
            all_metrics = np.mean(j_metrics_res, axis=2) if "J" in metric else np.mean(f_metrics_res, axis=2)
        row_ind, col_ind = linear_sum_assignment(-all_metrics)
        return j_metrics_res[row_ind, col_ind, :], f_metrics_res[row_ind, col_ind, :]

    def evaluate(self, res_path, metric=("J", "F"), debug=False):
        metric = metric if isinstance(metric, (tuple, list)) else [metric]
        if "T" in metric:
            raise ValueError("Temporal metric not supported!")
        if "J" not in metric and "F" not in metric:
            raise ValueError("Metric possible values are J for IoU or F for Boundary")
        metrics_res = {}
        if "J" in metric:
            metrics_res["J"] = {"M": [], "R": [], "D": [], "M_per_object": {}, "seq_len": {}}
        if "F" in metric:
            metrics_res["F"] = {"M": [], "R": [], "D": [], "M_per_object": {}, "seq_len": {}}
        separate_objects_masks = self.year != "2016"
        results = Results(root_dir=res_path, step=self.step)
        for seq in list(self.dataset.get_sequences()):
            all_gt_masks, all_void_masks, all_masks_id = self.dataset.get_all_masks(seq, separate_objects_masks)
            if self.task == "semi-supervised":
                all_gt_masks, all_masks_id = all_gt_masks[:, 1:-1, :, :], all_masks_id[1:-1]
            all_res_masks = results.read_masks(seq, all_masks_id)
            if self.task == "unsupervised":
                j_metrics_res, f_metrics_res = self._evaluate_unsupervised(all_gt_masks, all_res_masks, all_void_masks,
                                                                           metric)
            else:
                j_metrics_res, f_metrics_res = self._evaluate_semisupervised(all_gt_masks, all_res_masks, None, metric)
            for ii in range(all_gt_masks.shape[0]):
                seq_name = f"{seq}_{ii + 1}"
                if "J" in metric:
                    JM, JR, JD = db_statistics(j_metrics_res[ii])
                    metrics_res["J"]["M"].append(JM)
                    metrics_res["J"]["R"].append(JR)
                    metrics_res["J"]["D"].append(JD)
                    metrics_res["J"]["M_per_object"][seq_name] = JM
                    metrics_res["J"]["seq_len"][seq_name] = all_gt_masks.shape[1]
                if "F" in metric:
                    FM, FR, FD = db_statistics(f_metrics_res[ii])
                    metrics_res["F"]["M"].append(FM)
                    metrics_res["F"]["R"].append(FR)
                    metrics_res["F"]["D"].append(FD)
                    metrics_res["F"]["M_per_object"][seq_name] = FM
            if debug:
                sys.stdout.write(seq + "\n")
                sys.stdout.flush()
        return metrics_res


# ---- evaluation_method.py ---------------------------------------------------------------------------------------------

G_MEASURES = ["J&F-Mean", "J-Mean", "J-FrameMean", "J-Recall", "J-Decay", "F-Mean", "F-Recall", "F-Decay"]
SEQ_MEASURES = ["Sequence", "J-Mean", "F-Mean"]


def _cell(v):
    if isinstance(v, str):
        return v
    return "" if np.isnan(v) else "%.3f" % v


def csv_text(columns, rows):
    """the text of pandas' DataFrame(rows, columns).to_csv(index=False, float_format="%.3f") for str / float cells"""
    buf = io.StringIO()
    w = csv.writer(buf, lineterminator="\n", quoting=csv.QUOTE_MINIMAL)
    w.writerow(columns)
    for row in rows:
        w.writerow([_cell(v) for v in row])
    return buf.getvalue()


def table_text(columns, rows):
    """a plain right-aligned table of the same cells (what the tool prints)"""
    cells = [[str(c) for c in columns]] + [[v if isinstance(v, str) else f"{v:.6f}" for v in row] for row in rows]
    widths = [max(len(r[i]) for r in cells) for i in range(len(columns))]
    return "\n".join(" ".join(c.rjust(wd) for c, wd in zip(r, widths)) for r in cells)


def summary_tables(metrics_res):
    """(global row, per-sequence rows) of evaluation_method.py"""
    J, F = metrics_res["J"], metrics_res["F"]
    seq_names = list(J["M_per_object"].keys())
    sum_J, sum_num_frames = 0., 0
    for x in seq_names:
        sum_J += J["M_per_object"][x] * J["seq_len"][x]
        sum_num_frames += J["seq_len"][x]
    J_frame_avg = sum_J / sum_num_frames
    final_mean = (np.mean(J["M"]) + np.mean(F["M"])) / 2.
    g_res = np.array([final_mean, np.mean(J["M"]), J_frame_avg, np.mean(J["R"]), np.mean(J["D"]), np.mean(F["M"]),
                      np.mean(F["R"]), np.mean(F["D"])])
    seq_rows = [(x, float(J["M_per_object"][x]), float(F["M_per_object"][x])) for x in seq_names]
    return [list(map(float, g_res))], seq_rows


def main(argv=None):
    """python tools/davis_eval.py --davis_path ... --results_path ... [--set val --task unsupervised --year 2016 --step N]"""
    time_start = time.time()
    parser = argparse.ArgumentParser()
    parser.add_argument("--davis_path", type=str, default="/path/to/the/folder/DAVIS",
                        help="Path to the DAVIS folder containing the JPEGImages, Annotations, ImageSets folders")
    parser.add_argument("--set", type=str, default="val", help="Subset to evaluate the results")
    parser.add_argument("--task", type=str, default="unsupervised", choices=["semi-supervised", "unsupervised"])
    parser.add_argument("--results_path", type=str, required=True, help="Path to the folder with the pred_seg_*.png files")
    parser.add_argument("--year", type=str, default="2017", choices=["2016", "2017", "2019"])
    parser.add_argument("--step", type=int, default=0, help="The step to evaluate (0 for an export-config run)")
    parser.add_argument("--sequences", type=str, default="all", help="sequence to eval")
    args, _ = parser.parse_known_args(argv)
    csv_global = os.path.join(args.results_path, f"global_results-{args.set}.csv")
    csv_per_seq = os.path.join(args.results_path, f"per-sequence_results-{args.set}.csv")
    print(f"Evaluating sequences {args.sequences} for the {args.task} task...")
    ev = DAVISEvaluation(davis_root=args.davis_path, task=args.task, gt_set=args.set, year=args.year,
                         sequences=args.sequences, step=args.step)
    metrics_res = ev.evaluate(args.results_path)
    g_rows, seq_rows = summary_tables(metrics_res)
    with open(csv_global, "w") as f:
        f.write(csv_text(G_MEASURES, g_rows))
    print(f"Global results saved in {csv_global}")
    with open(csv_per_seq, "w") as f:
        f.write(csv_text(SEQ_MEASURES, seq_rows))
    print(f"Per-sequence results saved in {csv_per_seq}")
    sys.stdout.write(f"--------------------------- Global results for {args.set} ---------------------------\n")
    print(table_text(G_MEASURES, g_rows))
    sys.stdout.write(f"\n---------- Per sequence results for {args.set} ----------\n")
    print(table_text(SEQ_MEASURES, seq_rows))
    sys.stdout.write("\nTotal time:" + str(time.time() - time_start) + "\n")
    return metrics_res
