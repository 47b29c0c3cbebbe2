"""Pillow's 8-bit `Image.resize` on the device, bit for bit (csrc/pil_resample.hip).

The reference's SegTrackv2 / FBMS59 tool (tools/STv2-FBMS59-evaluation/eval_tool.py) resizes every exported mask with
Pillow's default filter and thresholds the result, so its figures depend on every rounding step of Pillow's resampler
(src/libImaging/Resample.c).  That resampler is integer arithmetic on two coefficient tables:

  precompute_coeffs      float64 filter weights per output position, normalised by their sequentially accumulated sum;
  normalize_coeffs_8bpc  int(+-0.5 + weight * 2**22);
  a horizontal and then a vertical pass, each clip(((1 << 21) + sum k * in) >> 22, 0, 255) in int32, the horizontal
  result rounded to u8 before the vertical pass; an axis that keeps its size is skipped.

`coeff_tables` transcribes the first two in Python floats (IEEE doubles, the same operations in the same order); the kernel
does the passes.  Only filters whose weights are polynomials are offered: Lanczos and Hamming go through sin / cos, whose
last bit differs between C libraries.  `resize_ref_np` is the same arithmetic in numpy: what `resize_u8` falls back to
for a reduction beyond the kernel's window, and what the CPU tests compare with Pillow.
"""
import functools

import numpy as np
import torch

from . import _lib
from .ops import _p, _stream

PRECISION_BITS = 32 - 8 - 2          # Resample.c
MAX_TAPS = 256                       # include/rcf_hip.h RCF_PIL_MAX_TAPS: vertical taps per output row the kernel takes


def _box(x):
    return 1.0 if -0.5 < x <= 0.5 else 0.0


def _bilinear(x):
    if x < 0.0:
        x = -x
    return 1.0 - x if x < 1.0 else 0.0


def _bicubic(x):
    a = -0.5
    if x < 0.0:
        x = -x
    if x < 1.0:
        return ((a + 2.0) * x - (a + 3.0)) * x * x + 1
    if x < 2.0:
        return (((x - 5) * x + 8) * x - 4) * a
    return 0.0


FILTERS = {"box": (_box, 0.5), "bilinear": (_bilinear, 1.0), "bicubic": (_bicubic, 2.0)}     # name -> (weight, support)


@functools.lru_cache(maxsize=256)
def coeff_tables(in_size, out_size, filter="bicubic"):
    """Pillow's tables of one axis: (k int32 [out_size, ksize], bounds int32 [out_size, 2] = first tap, tap count); read-only"""
    if filter not in FILTERS:
        raise ValueError(f"filter {filter!r}: only {sorted(FILTERS)} are reproducible to the bit")
    in_size, out_size = int(in_size), int(out_size)
    if in_size <= 0 or out_size <= 0:
        raise ValueError(f"sizes must be positive, got {in_size} -> {out_size}")
    weight, fsupport = FILTERS[filter]
    filterscale = scale = float(in_size) / out_size
    if filterscale < 1.0:
        filterscale = 1.0
    support = fsupport * filterscale
    ksize = int(np.ceil(support)) * 2 + 1
    k = np.zeros((out_size, ksize), dtype=np.int32)
    bounds = np.zeros((out_size, 2), dtype=np.int32)
    ss = 1.0 / filterscale
    one = float(1 << PRECISION_BITS)
    for xx in range(out_size):
        center = 0.0 + (xx + 0.5) * scale
        xmin = int(center - support + 0.5)
        if xmin < 0:
            xmin = 0
        xmax = int(center + support + 0.5)
        if xmax > in_size:
            xmax = in_size
        xmax -= xmin
        ww = 0.0
        row = []
        for x in range(xmax):
            w = weight((x + xmin - center + 0.5) * ss)
            row.append(w)
            ww += w
        for x in range(xmax):
            v = row[x] / ww if ww != 0.0 else row[x]
            k[xx, x] = int(-0.5 + v * one) if v < 0 else int(0.5 + v * one)
        bounds[xx] = (xmin, xmax)
    k.setflags(write=False)
    bounds.setflags(write=False)
    return k, bounds


def _tables(in_size, out_size, filter):
    """None for an axis that keeps its size (Pillow skips the pass)"""
    return None if in_size == out_size else coeff_tables(in_size, out_size, filter)


def _pass_np(a, tables, axis):
    """one pass over int64 [N, h, w] along `axis` (1 rows, 2 columns)"""
    k, bounds = tables
    shape = list(a.shape)
    shape[axis] = k.shape[0]
    out = np.empty(shape, dtype=np.int64)
    for i in range(k.shape[0]):
        f, c = int(bounds[i, 0]), int(bounds[i, 1])
        kk = k[i, :c].astype(np.int64)
        if axis == 2:
            acc = (a[:, :, f:f + c] * kk).sum(axis=2)
            out[:, :, i] = acc
        else:
            acc = (a[:, f:f + c, :] * kk[None, :, None]).sum(axis=1)
            out[:, i, :] = acc
    return np.clip((out + (1 << (PRECISION_BITS - 1))) >> PRECISION_BITS, 0, 255)


def _frames_np(frames):
    a = frames.detach().cpu().numpy() if isinstance(frames, torch.Tensor) else np.asarray(frames)
    if a.dtype != np.uint8 or a.ndim not in (3, 4) or (a.ndim == 4 and a.shape[3] != 3):
        raise ValueError(f"frames must be u8 [N,h,w] or [N,h,w,3], got {a.dtype} {a.shape}")
    return a


def resize_ref_np(frames, size, filter="bicubic"):
    """frames u8 [N,h,w] or [N,h,w,3] (channel 0 is taken), size (H, W) -> u8 numpy [N,H,W]: the numpy restatement of
    np.array(Image.fromarray(frame).resize((W, H), resample)) -- no device, no Pillow"""
    a = _frames_np(frames)
    if a.ndim == 4:
        a = a[..., 0]
    H, W = int(size[0]), int(size[1])
    _, h, w = a.shape
    tx, ty = _tables(w, W, filter), _tables(h, H, filter)
    a = a.astype(np.int64)
    if tx is not None:
        a = _pass_np(a, tx, 2)
    if ty is not None:
        a = _pass_np(a, ty, 1)
    return a.astype(np.uint8)


def iou_counts_np(resized, gt, pred_min):
    """int64 [N,2]: (intersection, union) of resized >= pred_min and gt != 0"""
    p, g = np.asarray(resized) >= pred_min, np.asarray(gt) != 0
    return np.stack([(p & g).sum(axis=(1, 2)), (p | g).sum(axis=(1, 2))], axis=1).astype(np.int64)


def tile_rows(h, H, ksy):
    """output rows per block the kernel would use (32 ... 1); 0: the call would be refused (ksy > MAX_TAPS)"""
    return int(_lib.load().rcf_pil_resample_tile_rows(int(h), int(H), int(ksy)))


def device_ok(h, H, filter="bicubic"):
    """whether the kernel takes this vertical resize (its LDS window holds the source rows of one output row)"""
    return h == H or coeff_tables(h, H, filter)[0].shape[1] <= MAX_TAPS


@functools.lru_cache(maxsize=64)
def _device_tables(in_size, out_size, filter, device):
    k, b = coeff_tables(in_size, out_size, filter)
    return torch.from_numpy(k.copy()).to(device), torch.from_numpy(b.copy()).to(device), k.shape[1]


def _from_numpy(a):
    a = np.ascontiguousarray(np.asarray(a))
    return torch.from_numpy(a if a.flags.writeable else a.copy())      # torch refuses to wrap a read-only array quietly


def _frames_dev(frames, device=None):
    t = frames if isinstance(frames, torch.Tensor) else _from_numpy(frames)
    if t.dtype != torch.uint8 or t.dim() not in (3, 4) or (t.dim() == 4 and t.shape[3] != 3):
        raise ValueError(f"frames must be u8 [N,h,w] or [N,h,w,3], got {t.dtype} {tuple(t.shape)}")
    if device is None:
        device = t.device if t.is_cuda else torch.device("cuda", torch.cuda.current_device())
    return t.to(device).contiguous()


def _launch(src, size, filter, dst, gt, pred_min, counts):
    """src u8 device [N,h,w] / [N,h,w,3]; one rcf_pil_resample_u8 call on the current stream"""
    N, h, w = src.shape[:3]
    H, W = size
    dev = src.device
    kx = bx = ky = by = None
    ksx = ksy = 0
    if w != W:
        kx, bx, ksx = _device_tables(w, W, filter, dev)
    if h != H:
        ky, by, ksy = _device_tables(h, H, filter, dev)
    with torch.cuda.device(dev):
        _lib.call("rcf_pil_resample_u8", _p(src), N, h, w, 3 if src.dim() == 4 else 1, _p(kx), _p(bx), ksx, _p(ky), _p(by), ksy,
                  H, W, _p(dst), _p(gt), int(pred_min), _p(counts), _stream())


def resize_u8(frames, size, filter="bicubic"):
    """frames u8 [N,h,w] or [N,h,w,3] (torch or numpy; RGB is read in place, channel 0), size (H, W) -> u8 device tensor
    [N,H,W] equal to np.array(Image.fromarray(frame).resize((W, H), resample)) (channel 0 for RGB).  Equal sizes give a
    copy.  A vertical reduction beyond the kernel's window goes through resize_ref_np on the host."""
    if filter not in FILTERS:
        raise ValueError(f"filter {filter!r}: only {sorted(FILTERS)} are reproducible to the bit")
    src = _frames_dev(frames)
    H, W = int(size[0]), int(size[1])
    N, h, w = src.shape[:3]
    if (h, w) == (H, W):
        return (src[..., 0] if src.dim() == 4 else src).clone()
    if not device_ok(h, H, filter):
        return torch.from_numpy(resize_ref_np(src.cpu().numpy(), (H, W), filter)).to(src.device)
    dst = torch.empty((N, H, W), dtype=torch.uint8, device=src.device)
    _launch(src, (H, W), filter, dst, None, 0, None)
    return dst


def resize_iou_counts(frames, gt, pred_min, filter="bicubic"):
    """frames as resize_u8, gt [N,H,W] u8 / bool (nonzero = on; its size is the target size) -> int64 numpy [N,2]: per frame
    the (intersection, union) of (resized frame >= pred_min) and gt.  The resized frames are not written anywhere."""
    if filter not in FILTERS:
        raise ValueError(f"filter {filter!r}: only {sorted(FILTERS)} are reproducible to the bit")
    src = _frames_dev(frames)
    g = gt if isinstance(gt, torch.Tensor) else _from_numpy(gt)
    if g.dim() != 3 or g.shape[0] != src.shape[0]:
        raise ValueError(f"gt must be [N,H,W] with N = {src.shape[0]}, got {tuple(g.shape)}")
    if g.dtype != torch.uint8:
        g = g != 0
    g = g.to(device=src.device, dtype=torch.uint8).contiguous()
    pred_min = int(pred_min)
    if pred_min < 0 or pred_min > 256:
        raise ValueError(f"pred_min {pred_min} is outside [0, 256]")
    N, H, W = g.shape
    h = src.shape[1]
    if not device_ok(h, H, filter):
        return iou_counts_np(resize_ref_np(src.cpu().numpy(), (H, W), filter), g.cpu().numpy(), pred_min)
    counts = torch.zeros((N, 2), dtype=torch.int64, device=src.device)
    _launch(src, (H, W), filter, None, g, pred_min, counts)
    return counts.cpu().numpy()
