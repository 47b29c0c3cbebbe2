"""Semantic constraints: rewrite every exported mask of the object channel as CRF(mask) x CRF(NCut-refine(mask)), the targets
stage 2.2 trains on.  The driver of the reference's tools/SemanticConstraintsAndMAA/semantic_constraints.py:280-460 on the
HIP kernels.

After stage 2.1 the EMA model's masks have been exported as {pretrain_dir}/{export dir}/{channel}/pred_seg_{seq}_{frame}_
{step:07}.png ({export dir}: saved_eval_export_trainval_ema for davis and fbms59, saved_eval_export_ema for stv2).  For every
frame of every sequence under the images directory the mask is refined by 10 Adam steps on its soft NCut over DINO ViT-S/8
keys (NCutHead, lr 0.45), both the mask and the refined mask go through the dense CRF (crf_scale 0.7 and 0.5), and the product
of the two -- for fbms59 the single-CRF mask when the two disagree on more than 10 000 pixels -- is saved as a mode-L PNG under
{export dir}_torchcrf_ncut_torchcrf/{channel}/ with the file name of the export.

The reference does this one frame at a time.  Here `--batch-frames` frames share a ViT forward, their Adam steps run together
on bit-packed affinities (ncut.ncut_refine_batch), both CRFs take the batch in one call each, and the merge and the conversion
to bytes are one kernel (offline.double_crf_merge_u8): the only copy to the host is the finished u8 batch.  Nothing is
downloaded: `--dino_ckpt` names the DINO checkpoint.
"""
import argparse
import os
from glob import glob

import numpy as np

from . import maa

SAVE_SUFFIX = "_torchcrf_ncut_torchcrf"
EXPORT_DIR_NAMES = {"davis": "saved_eval_export_trainval_ema", "stv2": "saved_eval_export_ema", "fbms59": "saved_eval_export_trainval_ema"}
UMI_TH = {"davis": None, "stv2": None, "fbms59": 10000}
NCUT_KW = dict(steps=10, learning_rate=0.45, weight_decay=1e-6)
CRF_KW = dict(srgb=5., scomp=5., sxy=60., scomp_smooth=0., sxy_smooth=0., refine_iters=50)
CRF_SCALE_SINGLE, CRF_SCALE = 0.7, 0.5          # the CRF on the exported mask / on the NCut-refined mask


def build_parser():
    ap = argparse.ArgumentParser(description="Refine exported masks with semantic constraints (NCut on DINO features + CRF).")
    ap.add_argument("--pretrain_dir", help="path to pretraining dir", default=None, type=str)
    ap.add_argument("--first-frames-only", help="accepted and unused, as in the reference", action="store_true")
    ap.add_argument("--num-channels", default=4, type=int)
    ap.add_argument("--object-channel", default=None, type=int, help="object channel (tools/maa.py selects it); required")
    ap.add_argument("--dataset", type=str, help="dataset", default="davis", choices=sorted(maa.DATASETS))
    ap.add_argument("--step", type=int, default=0,
                    help="The step of the export masks (should be 0 if exported with evaluation config)")
    ap.add_argument("--data_dir", type=str, default="data", help="directory that holds data_davis / data_SegTrackv2_resized / ...")
    ap.add_argument("--dino_ckpt", type=str, default=None,
                    help="DINO ViT-S/8 checkpoint: a state dict with the reference's parameter names (never downloaded)")
    ap.add_argument("--batch-frames", type=int, default=4, help="frames refined together")
    return ap


def export_dirs(pretrain_dir, dataset, channel):
    """-> (directory of the exported masks, directory of the refined masks of `channel`)"""
    name = EXPORT_DIR_NAMES[dataset]
    return os.path.join(pretrain_dir, name), os.path.join(pretrain_dir, name + SAVE_SUFFIX, str(channel))


def list_sequences(images_dir):
    """every sequence under the images directory (training and validation), sorted, dot files skipped"""
    return [s for s in sorted(os.listdir(images_dir)) if not s.startswith(".")]


def list_frames(images_dir, seqs):
    """[(seq, frame)]: every *.jpg of every sequence, sorted"""
    return [(seq, os.path.basename(p)[:-4]) for seq in seqs for p in sorted(glob(os.path.join(images_dir, seq, "*.jpg")))]


def save_path(save_dir, seq, frame, step):
    return os.path.join(save_dir, os.path.basename(maa.mask_path("", seq, frame, 0, step)))


class Refiner:
    """(images f32 [n,480,854,3] in [0,1], masks f32 [n,480,854] in [0,1]) -> u8 [n,480,854]: semantic_constraints.py:305-336
    for a batch of frames, on the GPU"""

    def __init__(self, model, umi_th=None, device="cuda"):
        from . import crf, ncut
        self.device, self.umi_th = device, umi_th
        self.ncut_head = ncut.NCutHead(args=None, model=model, **NCUT_KW).to(device).eval()
        self.crf_head_single = crf.CRFHead(args=None, crf_scale=CRF_SCALE_SINGLE, **CRF_KW)
        self.crf_head = crf.CRFHead(args=None, crf_scale=CRF_SCALE, **CRF_KW)

    def __call__(self, images, masks):
        import torch
        from . import offline
        imgs = torch.from_numpy(np.ascontiguousarray(images)).to(self.device)
        m = torch.from_numpy(np.ascontiguousarray(masks)).to(self.device)
        refined = self.ncut_head.forward_batch(imgs, m, standardize=True)
        return offline.double_crf_merge_u8(self.crf_head_single, self.crf_head, imgs, m, refined, umi_th=self.umi_th).cpu().numpy()


def main(argv=None, model=None, refiner=None):
    """The reference script's run; returns the paths written.  `model`: a module with get_last_qkv in place of the DINO
    checkpoint; `refiner(images, masks) -> u8 [n,H,W]`: in place of `Refiner` (tests)."""
    from PIL import Image
    args = build_parser().parse_args(argv)
    if args.object_channel is None:
        raise ValueError("no object channel: pass --object-channel K (tools/maa.py selects it; the refined masks are written "
                         "to a directory named after it)")
    if refiner is None and model is None:
        if not args.dino_ckpt:
            raise ValueError("no DINO checkpoint: pass --dino_ckpt PATH (the ViT-S/8 state dict the reference downloads; "
                             "nothing is downloaded here)")
        model = maa.load_dino(args.dino_ckpt)
    print("Dataset:", args.dataset)
    images_dir = maa.dataset_layout(args.dataset, args.data_dir)[0]
    pred_masks_dir, save_dir = export_dirs(args.pretrain_dir, args.dataset, args.object_channel)
    seqs = list_sequences(images_dir)
    print(f"Found {len(seqs)} sequences: {seqs}")
    frames = list_frames(images_dir, seqs)
    for seq, frame in frames:                                       # the reference asserts the same, frame by frame
        p = save_path(save_dir, seq, frame, args.step)
        if os.path.exists(p):
            raise FileExistsError(f"refusing to overwrite {p}: remove {save_dir} to refine again")
    if refiner is None:
        refiner = Refiner(model, umi_th=UMI_TH[args.dataset])
    os.makedirs(save_dir, exist_ok=True)
    print(f"Start refinement: {save_dir}")
    written = []
    bf = max(1, int(args.batch_frames))
    for i in range(0, len(frames), bf):
        chunk = frames[i:i + bf]
        images = np.stack([maa.load_image(images_dir, s, f) for s, f in chunk])
        masks = np.stack([maa.load_mask(pred_masks_dir, s, f, args.object_channel, args.step) for s, f in chunk])
        out = np.asarray(refiner(images, masks))
        assert out.dtype == np.uint8 and out.shape == masks.shape, (out.dtype, out.shape)
        for (s, f), u8 in zip(chunk, out):
            p = save_path(save_dir, s, f, args.step)
            Image.fromarray(u8).convert("L").save(p)
            written.append(p)
    return written
