"""CRF post-processing of exported masks: the last step before evaluation ("With CRF post-processing" of the reference's
README).  The driver of the reference's tools/pydenseCRF/crf.py:94-195, which crf_parallel.sh runs once per sequence, on the
HIP CRF.

For every frame {input}/{seq}/{frame}.jpg the exported mask {annotation-dir}/pred_seg_{seq}_{frame}_{step:07}.png is resized
to the frame's 854 x 480 with PIL's default filter, divided by 0.8 and clipped to a byte, refined by `refine` (unary -log of the
mask over its maximum, bilateral term only: sxy 60, srgb 5, compat 5, 50 mean-field iterations, pydensecrf's symmetric
normalisation) and saved as a mode-L PNG of 0 / 255 under the same name in a sibling directory: the mask's directory with
`_crf` appended -- or, when that directory's name is a single character (a channel directory such as `0`), its parent with
`_crf` appended and the channel directory below it.  Existing files are overwritten, as in the reference.

The reference refines one frame at a time on the CPU, one process per sequence.  Here one process takes every sequence
(`--seq` accepts several patterns), `--batch-frames` frames go through one CRF call (offline.refine_batch_u8: the bytes are
uploaded, the unary is made on the device, the only copy back is the finished u8 batch), and `--workers` threads decode the next
batch and encode the last one while the GPU works.  A frame's file depends neither on the number of workers nor on which
thread wrote it.
"""
import argparse
import os
from concurrent.futures import ThreadPoolExecutor
from glob import glob

import numpy as np

from . import maa

IMG_SIZE = maa.IMG_SIZE                          # (480, 854): crf.py:159 asserts it of every frame
REFINE_KW = dict(gk=0.1, sxy=60.0, srgb=5.0, compat=5.0, iters=50)          # crf.py:74,177-184
MAX_WORKERS = 16


def build_parser():
    ap = argparse.ArgumentParser(description="CRF post-processing of exported masks (tools/pydenseCRF/crf.py on the HIP CRF).")
    ap.add_argument("--input", help="Input directory: {input}/{seq}/{frame}.jpg")
    ap.add_argument("--output", help="Output directory (accepted and unused, as in the reference)")
    ap.add_argument("--annotation-dir", help="Annotation directory: the exported masks (required)", default=None)
    ap.add_argument("--allow_skip", action="store_true", help="Allow skipping if annotation does not exist")
    ap.add_argument("--step", default=0, type=int,
                    help="The step of export, 0 by default (masks exported with export config will have 0 as step). "
                         "Use 4320 for 20 epochs on davis.")
    ap.add_argument("--seq", type=str, nargs="+", default=["*"], help="sequence pattern(s); all sequences by default")
    ap.add_argument("--batch-frames", type=int, default=8, help="frames refined together")
    ap.add_argument("--workers", type=int, default=8, help=f"host threads that read and write files (at most {MAX_WORKERS})")
    return ap


def list_frames(input_dir, patterns):
    """the *.jpg of every pattern, sorted per pattern as crf.py:130-131 sorts its one; a frame two patterns match is taken once"""
    paths, seen = [], set()
    for pat in patterns:
        for p in sorted(glob(os.path.join(input_dir, pat, "*.jpg"))):
            if p not in seen:
                seen.add(p)
                paths.append(p)
    return paths


def annotation_path(annotation_dir, image_path, step):
    """crf.py:140,147"""
    scene, frame = os.path.normpath(image_path).split(os.sep)[-2:]
    return os.path.join(annotation_dir, f"pred_seg_{scene}_{frame[:-4]}_{step:07}.png")


def save_dir_of(annotation_dir):
    """crf.py:170-175: `_crf` goes to the directory that holds the masks, or to its parent when that directory's name is a single
    character"""
    d = os.path.normpath(annotation_dir)
    name = os.path.basename(d)
    if len(name) > 1:
        return d + "_crf"
    d = os.path.abspath(d)                        # (a relative `0`: the parent has to have a name)
    return os.path.join(os.path.dirname(d) + "_crf", os.path.basename(d))


def load_frame(image_path, mask_path):
    """crf.py:158-167 -> (image u8 [480,854,3], mask u8 [480,854]: the raw resized export, before the division by 0.8)"""
    from PIL import Image
    with Image.open(image_path) as im:            # PIL, to be consistent with evaluation (crf.py:157)
        img = np.asarray(im)
    if img.ndim != 3 or img.shape != (IMG_SIZE[0], IMG_SIZE[1], 3):
        raise ValueError(f"{image_path}: expected a 3-channel {IMG_SIZE[1]} x {IMG_SIZE[0]} image, got shape {img.shape}")
    with Image.open(mask_path) as im:
        mask = np.asarray(im.resize((img.shape[1], img.shape[0])))
    if mask.ndim == 3:
        mask = mask[..., 0]
    if mask.dtype != np.uint8:
        raise ValueError(f"{mask_path}: expected an 8-bit mask, got {mask.dtype}")
    return img, np.ascontiguousarray(mask)


def save_mask(path, u8):
    from PIL import Image
    Image.fromarray(u8).convert("L").save(path)
    return path


class Refiner:
    """(images u8 [n,480,854,3], raw resized masks u8 [n,480,854]) -> u8 [n,480,854] of 0 / 255: crf.py:169 and `refine` for a
    batch of frames, on the GPU"""

    def __init__(self, device="cuda:0"):
        self.device = device

    def __call__(self, images, masks):
        from . import offline
        return offline.refine_batch_u8(masks, images, device=self.device, prescale=True, **REFINE_KW).cpu().numpy()


def main(argv=None, refiner=None):
    """The reference script's run; returns the paths written.  `refiner(images_u8, masks_u8) -> u8 [n,H,W]`: in place of
    `Refiner` (tests)."""
    args = build_parser().parse_args(argv)
    annotation_dir = args.annotation_dir
    if annotation_dir is None:
        raise ValueError("no annotation directory: pass --annotation-dir DIR (the exported masks)")
    if not os.path.exists(annotation_dir):
        raise FileNotFoundError(f"annotation directory {annotation_dir} does not exist")
    if args.input is None:
        raise ValueError("no input directory: pass --input DIR ({input}/{seq}/{frame}.jpg)")
    print("Annotation dir:", annotation_dir)
    paths = list_frames(args.input, args.seq)
    print("seq:", " ".join(args.seq))
    print("len(paths):", len(paths))
    skipped, frames = 0, []
    for p in paths:
        a = annotation_path(annotation_dir, p, args.step)
        if os.path.exists(a):
            frames.append((p, a))
        elif args.allow_skip:
            skipped += 1
        else:
            raise FileNotFoundError(a)
    save_dir = save_dir_of(annotation_dir)
    written = []
    if frames:
        if refiner is None:
            refiner = Refiner()
        os.makedirs(save_dir, exist_ok=True)       # exist_ok: several runs may share it, one per sequence (crf.py:187)
        bf = max(1, int(args.batch_frames))
        chunks = [frames[i:i + bf] for i in range(0, len(frames), bf)]
        with ThreadPoolExecutor(max_workers=min(MAX_WORKERS, max(1, int(args.workers)))) as pool:
            load = lambda chunk: [pool.submit(load_frame, p, a) for p, a in chunk]
            ahead, saves = load(chunks[0]), []
            for i, chunk in enumerate(chunks):
                loaded = [f.result() for f in ahead]
                ahead = load(chunks[i + 1]) if i + 1 < len(chunks) else []        # decoded while this batch is refined
                images, masks = np.stack([im for im, _ in loaded]), np.stack([m for _, m in loaded])
                out = np.asarray(refiner(images, masks))
                assert out.dtype == np.uint8 and out.shape == masks.shape, (out.dtype, out.shape)
                saves += [pool.submit(save_mask, os.path.join(save_dir, os.path.basename(a)), u8) for (_, a), u8 in zip(chunk, out)]
            written = [f.result() for f in saves]                                 # in frame order
    if skipped > 0:
        print(f"Skipped {skipped} frames (this number does not include the ones in training set if val_seq is True)")
    return written
