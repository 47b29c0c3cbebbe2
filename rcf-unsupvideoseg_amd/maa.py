"""Motion-appearance alignment (MAA): which exported mask channel is the object?  The driver of the reference's
tools/SemanticConstraintsAndMAA/maa.py:141-402 on the HIP kernels.

After stage 1 every channel c of the model has been exported as {pretrain_dir}/saved_eval_export/{c}/pred_seg_*.png.  The
MAA of a channel is the mean over the validation frames of MINUS the soft NCut of the channel's mask on DINO ViT-S/8 keys;
the channel with the largest MAA is `object_channel` for stage 2.1, stage 2.2, the export and the evaluators.

The reference scores one (frame, channel) pair at a time: a ViT forward, a Gram product, a threshold and two mat-vecs each.
Nothing but the mask depends on the channel, so here a frame costs ONE ViT forward and ONE Gram product, and
NCutEvalHead.forward_multi scores all its channels in one pass over the raw Gram matrix (rcf_ncut_values_f32);
`--batch-frames` frames go through the ViT together.  Nothing is downloaded: `--dino_ckpt` names the DINO checkpoint.
"""
import argparse
import os
from glob import glob

import numpy as np

EXPORT_DIR_NAME = "saved_eval_export"
IMG_SIZE = (480, 854)

DAVIS_VAL_SEQS = ["blackswan", "bmx-trees", "breakdance", "camel", "car-roundabout", "car-shadow", "cows", "dance-twirl",
                  "dog", "drift-chicane", "drift-straight", "goat", "horsejump-high", "kite-surf", "libby", "motocross-jump",
                  "paragliding-launch", "parkour", "scooter-black", "soapbox"]
STV2_VAL_SEQS = ["bird_of_paradise", "birdfall", "bmx", "cheetah", "drift", "frog", "girl", "hummingbird", "monkey",
                 "monkeydog", "parachute", "penguin", "soldier", "worm"]                                  # all sequences
FBMS59_VAL_SEQS = ["camel01", "cars1", "cars10", "cars4", "cars5", "cats01", "cats03", "cats06", "dogs01", "dogs02",
                   "farm01", "giraffes01", "goats01", "horses02", "horses04", "horses05", "lion01", "marple12", "marple2",
                   "marple4", "marple6", "marple7", "marple9", "people03", "people1", "people2", "rabbits02", "rabbits03",
                   "rabbits04", "tennis"]
# dataset -> (root under data_dir, images below the root, validation sequences)
DATASETS = {
    "davis": ("data_davis", os.path.join("JPEGImages", "480p"), DAVIS_VAL_SEQS),
    "stv2": ("data_SegTrackv2_resized", "JPEGImages", STV2_VAL_SEQS),
    "fbms59": ("data_fbms59_resized", "JPEGImages", FBMS59_VAL_SEQS),
}


def build_parser():
    ap = argparse.ArgumentParser(description="Evaluate motion-appearance alignment.")
    ap.add_argument("--pretrain_dir", help="path to pretraining dir", default=None, type=str)
    ap.add_argument("--first-frames-only", help="use the first frame of each sequence only", action="store_true")
    ap.add_argument("--num-channels", default=4, type=int)
    ap.add_argument("--object-channel", default=None, type=int,
                    help="object channel, if not supplied, perform MAA on all object channels and select the one with best MAA")
    ap.add_argument("--dataset", type=str, help="dataset", default="davis", choices=sorted(DATASETS))
    ap.add_argument("--step", type=int, default=0,
                    help="The step of the export masks (should be 0 if exported with evaluation config)")
    ap.add_argument("--data_dir", type=str, default="data", help="directory that holds data_davis / data_SegTrackv2_resized / ...")
    ap.add_argument("--dino_ckpt", type=str, default=None,
                    help="DINO ViT-S/8 checkpoint: a state dict with the reference's parameter names (never downloaded)")
    ap.add_argument("--batch-frames", type=int, default=4, help="frames per ViT forward")
    return ap


def dataset_layout(dataset, data_dir="data"):
    """-> (images_dir, gt_dir, val_seqs)"""
    root, images, seqs = DATASETS[dataset]
    images_dir = os.path.join(data_dir, root, images)
    return images_dir, images_dir.replace("JPEGImages", "Annotations"), list(seqs)


def mask_path(pred_masks_dir, seq, frame, channel, step):
    return os.path.join(pred_masks_dir, str(channel), f"pred_seg_{seq}_{frame}_{step:07}.png")


def load_mask(pred_masks_dir, seq, frame, channel, step):
    """f32 [480,854] in [0,1]: the exported mask, resized by PIL with its default filter (the reference passes none)"""
    from PIL import Image
    path = mask_path(pred_masks_dir, seq, frame, channel, step)
    if not os.path.exists(path):
        raise FileNotFoundError(f"exported mask of channel {channel} is missing: {path} (export every channel of the "
                                f"stage-1 model at step {step} first)")
    mask = np.asarray(Image.open(path).resize((IMG_SIZE[1], IMG_SIZE[0]))).astype(np.float32) / 255.
    return mask[..., 0] if mask.ndim == 3 else mask


def load_image(images_dir, seq, frame):
    from PIL import Image
    img = np.asarray(Image.open(os.path.join(images_dir, seq, frame + ".jpg")).convert("RGB")).astype(np.float32) / 255.
    assert img.shape == IMG_SIZE + (3,), f"{seq}/{frame}.jpg is {img.shape}, expected {IMG_SIZE + (3,)}"
    return img


def skip_frame(dataset, gt_dir, seq, frame):
    """FBMS59 annotates a few frames per sequence and only those count; every frame of the other datasets counts"""
    return "fbms59" in dataset and not os.path.exists(os.path.join(gt_dir, seq, frame + ".png"))


def list_frames(dataset, images_dir, gt_dir, val_seqs, first_frames_only=False):
    """[(seq, frame)] in evaluation order"""
    out = []
    for seq in val_seqs:
        for path in sorted(glob(os.path.join(images_dir, seq, "*.jpg"))):
            frame = os.path.basename(path)[:-4]
            if skip_frame(dataset, gt_dir, seq, frame):
                continue
            out.append((seq, frame))
            if first_frames_only:
                break
    return out


def select_channel(frame_maas):
    return int(np.argmax(np.array(frame_maas)))


def load_dino(path):
    import torch
    from . import vit
    model = vit.vit_small(patch_size=8)
    model.load_state_dict(torch.load(path, map_location="cpu"))          # strict, like the reference's get_dino_model
    return model


def evaluate(args, channels, model):
    """float64 [frames, len(channels)]: the soft NCut of every channel's mask on every validation frame"""
    import torch
    from . import ncut
    images_dir, gt_dir, val_seqs = dataset_layout(args.dataset, args.data_dir)
    pred_masks_dir = os.path.join(args.pretrain_dir, EXPORT_DIR_NAME)
    frames = list_frames(args.dataset, images_dir, gt_dir, val_seqs, args.first_frames_only)
    head = ncut.NCutEvalHead(args=None, model=model).to("cuda").eval()
    values = []
    bf = max(1, int(args.batch_frames))
    for i in range(0, len(frames), bf):
        chunk = frames[i:i + bf]
        imgs = np.stack([load_image(images_dir, s, f) for s, f in chunk])
        masks = np.stack([np.stack([load_mask(pred_masks_dir, s, f, c, args.step) for c in channels]) for s, f in chunk])
        values.append(head.forward_multi(torch.from_numpy(imgs).to("cuda"), torch.from_numpy(masks).to("cuda"), standardize=True))
    return np.concatenate(values) if values else np.zeros((0, len(channels)))


def main(argv=None, model=None, evaluator=None):
    """The reference script's run: prints its lines, returns (frame_maas, best_channel); best_channel is None when
    --object-channel fixed the channel (the reference then ends without an exit code).  `model`: a module with
    get_last_qkv in place of the DINO checkpoint; `evaluator(args, channels)`: in place of `evaluate` (tests)."""
    args = build_parser().parse_args(argv)
    if evaluator is None and model is None:
        if not args.dino_ckpt:
            raise ValueError("no DINO checkpoint: pass --dino_ckpt PATH (the ViT-S/8 state dict the reference downloads; "
                             "nothing is downloaded here)")
        model = load_dino(args.dino_ckpt)
    print("Dataset:", args.dataset)
    images_dir = dataset_layout(args.dataset, args.data_dir)[0]
    if os.path.isdir(images_dir):
        seqs = [s for s in sorted(os.listdir(images_dir)) if not s.startswith(".")]
        print(f"Found {len(seqs)} sequences: {seqs}")
    channels = list(range(args.num_channels)) if args.object_channel is None else [args.object_channel]
    ncuts = np.asarray(evaluator(args, channels) if evaluator is not None else evaluate(args, channels, model), dtype=np.float64)
    frame_maas = []
    for k, channel in enumerate(channels):
        frame_maa = np.mean(-ncuts[:, k])
        print(f"frame MAA with object channel {channel}: {frame_maa * 100.:.2f}")
        frame_maas.append(frame_maa)
    best = None
    if len(channels) > 1:
        best = select_channel(frame_maas)
        print(f"The best object channel among all channels evaluated is channel {best}")
    return frame_maas, best
