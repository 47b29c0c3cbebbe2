"""Offline 480x854 CRF callers of the reference on the HIP mean-field CRF:

* `refine` / `refine_batch`: the post-processor of tools/pydenseCRF/crf.py:57-89 (Gaussian pre-blur of the u8 mask,
  normalise by its maximum, clip, unary = -log, bilateral pairwise term only, 50 iterations, MAP), same signature.
* `refine_batch_u8`: `refine_batch` from u8 masks to the u8 image the post-processing driver saves (rcf_amd.postprocess): the
  bytes are uploaded and the unary comes from a table on the device (rcf_crf_unary_lut_u8), bit-identical to the host's.
* `double_crf_merge`: the CRF / NCut-CRF merge of tools/SemanticConstraintsAndMAA/semantic_constraints.py:299-324
  (`crf_head_single`, crf_scale 0.7, on the input mask; `crf_head`, crf_scale 0.5, on the refined mask; product, or
  the single-CRF mask when the two disagree by more than `umi_th`).
* `double_crf_merge_u8`: the same for a batch of frames, ending in the u8 image the driver saves (rcf_mask_merge_u8: the
  disagreement counts and the bytes on the device, no host round trip); the route of rcf_amd.semantic.

`refine` reproduces pydensecrf's arithmetic: DenseCRF2D.addPairwiseBilateral's default SYMMETRIC kernel normalisation
(N^1/2 K N^1/2, Kraehenbuehl & Koltun's densecrf), selected in the HIP kernel by rcf_crf_soft_ex(normalization=1); the
merge uses tools/torchCRF's (the reference's `CRFHead.crf`).  pydensecrf is not importable in this environment and is not
vendored by the reference: the symmetric mode is checked against oracle/crf_ref.c's restatement of the published
algorithm (parity-unpinned; tests/test_crf_gpu.py, tests/test_crf_oracle_cpu.py).
"""
import numpy as np
import torch

from .crf import crf_soft_batched


def _unary_from_u8(mask, gk):
    """tools/pydenseCRF/crf.py:60-68 on the host (an offline tool; the reference does the same in numpy)"""
    U = mask.astype(np.float64)
    if int(4.0 * gk + 0.5) > 0:                       # scipy's default truncate: sigma 0.1 -> a 1-tap kernel
        from scipy.ndimage import gaussian_filter
        U = gaussian_filter(mask, sigma=gk).astype(np.float64)
    U = U / (np.amax(U) + 1e-8)
    U = np.clip(U, 1e-6, 1.0 - 1e-6)
    UU = np.stack([-np.log(1.0 - U), -np.log(U)], axis=-1)          # [H, W, 2]: label-minor, as the C ABI wants it
    return np.float32(UU).reshape(-1, 2)


def refine_batch(masks, images, gk=0.1, sxy=60.0, srgb=5.0, compat=5.0, iters=50, device="cuda:0", symmetric=True):
    """masks u8 [n,H,W] (0..255), images u8 [n,H,W,3] -> float32 [n,H,W] of 0/1 (one library call for all frames).
    symmetric=True is pydensecrf's normalisation (what tools/pydenseCRF/crf.py runs); False is tools/torchCRF's."""
    masks, images = np.asarray(masks), np.ascontiguousarray(images)
    n, H, W = masks.shape
    unary = torch.from_numpy(np.stack([_unary_from_u8(m, gk) for m in masks])).to(device)
    rgb = torch.from_numpy(images).to(device)
    out = crf_soft_batched(rgb, unary, W, H, 0.0, 0.0, float(compat), float(sxy), float(srgb), int(iters),
                           symmetric=symmetric)
    return out.float().cpu().numpy()


PRESCALE = 0.8          # tools/pydenseCRF/crf.py:169: the driver divides the resized export by it before `refine`
_TABLES = {}


def prescale_u8(mask):
    """tools/pydenseCRF/crf.py:169 on u8: (mask / 0.8).clip(0, 255).astype(uint8), a monotone map of bytes"""
    return (np.asarray(mask) / PRESCALE).clip(min=0, max=255).astype(np.uint8)


def unary_table(prescale=False):
    """float32 [256, 256, 2]: [a, v] = the unary `_unary_from_u8` (gk with a 1-tap blur) gives a pixel of value v in a frame whose
    maximum is a, computed with its float64 expressions and rounded to fp32 as there.  Those steps see the two bytes only, so the
    table IS the function, bit for bit (v > a never occurs in a frame; the entry is the same formula).  prescale: a and v are
    bytes of the raw resized export and `prescale_u8` comes first -- monotone, so the scaled frame's maximum is the scaled
    maximum."""
    s = prescale_u8(np.arange(256, dtype=np.uint8)) if prescale else np.arange(256, dtype=np.uint8)
    U = s.astype(np.float64)[None, :] / (s.astype(np.float64)[:, None] + 1e-8)
    U = np.clip(U, 1e-6, 1.0 - 1e-6)
    return np.float32(np.stack([-np.log(1.0 - U), -np.log(U)], axis=-1))


def _device_table(device, prescale):
    key = (str(device), bool(prescale))
    if key not in _TABLES:
        _TABLES[key] = torch.from_numpy(unary_table(prescale)).to(device)          # 512 KB, once per device
    return _TABLES[key]


def unary_from_u8_device(masks, prescale=False):
    """u8 [n,H,W] on the device -> unary float32 [n,H*W,2] = `_unary_from_u8` of every frame (after `prescale_u8` with
    prescale), by rcf_crf_unary_lut_u8: the per-frame maximum, then a gather from the table"""
    from . import _lib
    from .ops import _p, _stream
    if not masks.is_cuda or masks.dtype != torch.uint8 or masks.dim() != 3:
        raise RuntimeError("masks must be a uint8 [n,H,W] CUDA tensor")
    masks = masks.contiguous()
    n, H, W = masks.shape
    unary = torch.empty((n, H * W, 2), dtype=torch.float32, device=masks.device)
    scratch = torch.empty(n, dtype=torch.int32, device=masks.device)
    _lib.call("rcf_crf_unary_lut_u8", _p(masks), n, H * W, _p(_device_table(masks.device, prescale)), _p(unary), _p(scratch),
              _stream())
    return unary


@torch.no_grad()
def refine_batch_u8(masks, images, gk=0.1, sxy=60.0, srgb=5.0, compat=5.0, iters=50, device="cuda:0", symmetric=True,
                    prescale=False):
    """`refine_batch` from bytes to bytes: masks u8 [n,H,W], images u8 [n,H,W,3] (numpy or tensors) -> u8 [n,H,W] of 0 / 255 ON
    THE DEVICE, the (new_mask * 255).astype(uint8) tools/pydenseCRF/crf.py:190 saves; the caller makes the only copy to the host.
    The bytes go up as they are (0.4 MB per 480x854 mask instead of 3.3 MB of fp32 unary) and the unary is made there
    (`unary_from_u8_device`), bit-identical to the host's.  prescale=False: masks as `refine` takes them; True: the raw resized
    exports, crf.py:169's division by 0.8 composed into the table.  A gk whose blur has more than one tap takes the host route
    (no reference caller uses one)."""
    if int(4.0 * gk + 0.5) > 0:
        m = prescale_u8(_host(masks)) if prescale else _host(masks)
        out = refine_batch(m, _host(images), gk, sxy, srgb, compat, iters, device, symmetric)
        return torch.from_numpy((out * 255.).astype(np.uint8)).to(device)
    m, rgb = _to_device(masks, device), _to_device(images, device)
    if m.dtype != torch.uint8 or rgb.dtype != torch.uint8:
        raise RuntimeError("refine_batch_u8 takes uint8 masks and images")
    n, H, W = m.shape
    unary = unary_from_u8_device(m, prescale)
    out = crf_soft_batched(rgb, unary, W, H, 0.0, 0.0, float(compat), float(sxy), float(srgb), int(iters), symmetric=symmetric)
    return out.to(torch.uint8) * 255


def _to_device(x, device):
    t = x if torch.is_tensor(x) else torch.from_numpy(np.ascontiguousarray(x))
    return t.to(device).contiguous()


def _host(x):
    return x.cpu().numpy() if torch.is_tensor(x) else np.asarray(x)


def refine(mask, image, gk, sxy, srgb, compat, gtmask, iters=50, device="cuda:0", symmetric=True):
    """tools/pydenseCRF/crf.py:57 `refine(mask, image, gk, sxy, srgb, compat, gtmask)`"""
    new_mask = refine_batch(mask[None], image[None], gk, sxy, srgb, compat, iters, device, symmetric)[0]
    if gtmask is not None:
        gt, bm = gtmask > 0.1, new_mask > 0.1
        return new_mask, np.float32(np.sum(gt & bm)) / np.float32(np.sum(gt | bm))
    return new_mask


def umi(a, b):
    """semantic_constraints.py:271-277: union minus intersection (nan for two empty masks)"""
    i, u = a & b, a | b
    if u.sum() == 0:
        return float("nan")
    return u.sum() - i.sum()


@torch.no_grad()
def double_crf_merge(crf_head_single, crf_head, images, masks, refined_masks, umi_th=None):
    """semantic_constraints.py:303-322.  images [n,H,W,3] in [0,1] (`unstandardize=False`), masks / refined_masks
    [n,H,W] in [0,1] -> merged masks [n,H,W]"""
    a = crf_head_single(images, masks, unstandardize=False)
    b = crf_head(images, refined_masks, unstandardize=False)
    if umi_th is None:
        return a * b
    out = a * b
    for i in range(a.shape[0]):
        if umi(a[i].cpu().numpy() > 0.5, b[i].cpu().numpy() > 0.5) > umi_th:
            out[i] = a[i]                                # likely captures different things: keep the single CRF
    return out


@torch.no_grad()
def double_crf_merge_u8(crf_head_single, crf_head, images, masks, refined_masks, umi_th=None, return_counts=False):
    """`double_crf_merge` as the u8 image the driver saves, (merged * 255).astype(uint8) of semantic_constraints.py:335-336: u8
    [n,H,W] on the device.  Both CRFs run batched and rcf_mask_merge_u8 counts the union minus the intersection of every frame
    and writes the bytes: nothing goes to the host.  `return_counts`: also int64 [n], the counts."""
    from . import _lib
    from .ops import _p, _stream
    a = crf_head_single(images, masks, unstandardize=False).contiguous()
    b = crf_head(images, refined_masks, unstandardize=False).contiguous()
    n, H, W = a.shape
    out = torch.empty((n, H, W), dtype=torch.uint8, device=a.device)
    counts = torch.empty(n, dtype=torch.int64, device=a.device)
    _lib.call("rcf_mask_merge_u8", _p(a), _p(b), n, H * W, -1 if umi_th is None else int(umi_th), _p(out), _p(counts), _stream())
    return (out, counts) if return_counts else out
