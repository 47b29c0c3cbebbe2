"""GPU: the CRF post-processing on the device -- the unary pass (rcf_crf_unary_lut_u8) bit for bit against a numpy restatement
of tools/pydenseCRF/crf.py:60-68 and :169, offline.refine_batch_u8 byte for byte against the host-unary route it replaces
(offline.refine_batch), and the driver end to end at 480 x 854.

Bars: the unary pass copies table entries, so its fp32 bits ARE the host's (np.array_equal, no tolerance); with bit-identical
unaries and a CRF that is run-to-run bit-identical (tests/test_crf_gpu.py) the two routes give the same bytes on the same batch;
between different batch sizes the MAP bar of tests/test_crf_gpu.py between equally valid evaluations applies, >= 99.9 % of a
frame's pixels."""
import os
import shutil

import numpy as np
import pytest
import torch

import rcf_amd
from rcf_amd import offline, postprocess, synth

pytestmark = pytest.mark.gpu
DEV = "cuda:0"


def reference_prescale(mask):
    """tools/pydenseCRF/crf.py:169"""
    return (mask / 0.8).clip(min=0, max=255).astype(np.uint8)


def reference_unary(mask):
    """tools/pydenseCRF/crf.py:60-69 (gaussian_filter with sigma 0.1 on u8 is the identity: scipy's radius is int(4 * 0.1 + 0.5) = 0)
    -> float32 [H*W, 2], label-minor as the C ABI takes it"""
    U = mask / (np.amax(mask) + 1e-8)
    U = np.clip(U, 1e-6, 1.0 - 1e-6)
    UU = np.zeros((2, mask.shape[0], mask.shape[1]))
    UU[1, :, :] = U
    UU[0, :, :] = 1.0 - U
    return np.ascontiguousarray(np.float32(-np.log(UU)).reshape((2, -1)).T)


def _masks(frames, H, W):
    """random u8 frames with different maxima; with three frames: one all zero, one with a raw maximum of 255, one whose raw
    maximum stays below 204 (its scaled maximum below 255)"""
    g = np.random.default_rng(1000 * frames + H)
    tops = {1: [231], 2: [255, 97], 3: [0, 255, 150]}[frames]
    out = np.stack([g.integers(0, t + 1, (H, W), dtype=np.uint8) for t in tops])
    for m, t in zip(out, tops):
        m[H // 2, W // 3] = t
    return out


@pytest.mark.parametrize("prescale", [False, True])
@pytest.mark.parametrize("frames,H,W", [(1, 7, 9), (3, 37, 53), (2, 96, 130)])
def test_unary_pass_is_bit_exact(frames, H, W, prescale):
    masks = _masks(frames, H, W)
    want = np.stack([reference_unary(reference_prescale(m) if prescale else m) for m in masks])
    got = offline.unary_from_u8_device(torch.from_numpy(masks).to(DEV), prescale).cpu().numpy()
    assert got.shape == (frames, H * W, 2) and got.dtype == np.float32
    assert np.array_equal(got.view(np.uint32), want.view(np.uint32))
    if frames == 3:
        assert np.array_equal(got[0], np.broadcast_to(np.float32([1.0000005e-06, 13.815511]), (H * W, 2)))      # the all-zero frame
        assert reference_prescale(masks[2]).max() < 255
    # wherever the batch starts: every 16-byte phase of the first frame's address
    buf = torch.zeros(frames * H * W + 16, dtype=torch.uint8, device=DEV)
    for lead in (1, 5, 15):
        buf.fill_(255)                                                          # bytes around the batch that must not leak in
        view = buf[lead:lead + frames * H * W].view(frames, H, W)
        view.copy_(torch.from_numpy(masks))
        assert view.data_ptr() % 16 == (buf.data_ptr() + lead) % 16
        got = offline.unary_from_u8_device(view, prescale).cpu().numpy()
        assert np.array_equal(got.view(np.uint32), want.view(np.uint32)), lead


def _batch(n, H, W, seed=5200):
    images = np.stack([synth.smooth_rgb(H, W, seed + i) for i in range(n)])
    tops = [255, 180, 131]
    masks = np.stack([(synth.soft_blob_mask(H, W, seed + i) * tops[i % 3]).astype(np.uint8) for i in range(n)])
    return masks, images


@pytest.mark.parametrize("iters", [10, 50])
def test_refine_batch_u8_equals_refine_batch(iters, report):
    masks, images = _batch(3, 96, 130)
    want = (offline.refine_batch(masks, images, iters=iters) * 255.).astype(np.uint8)
    got = offline.refine_batch_u8(masks, images, iters=iters)
    assert got.is_cuda and got.dtype == torch.uint8 and tuple(got.shape) == masks.shape
    got = got.cpu().numpy()
    assert set(np.unique(got)) <= {0, 255} and 0 < (got == 255).mean() < 1
    report(f"refine_batch_u8 vs refine_batch, 3 x 96x130, T={iters}: differing bytes {int((got != want).sum())}")
    assert np.array_equal(got, want)
    # the raw export: crf.py:169 composed into the table against the same step on the host
    want_raw = (offline.refine_batch(reference_prescale(masks), images, iters=iters) * 255.).astype(np.uint8)
    got_raw = offline.refine_batch_u8(torch.from_numpy(masks).to(DEV), torch.from_numpy(images).to(DEV), iters=iters, prescale=True)
    assert np.array_equal(got_raw.cpu().numpy(), want_raw)


def test_a_wider_blur_takes_the_host_route():
    masks, images = _batch(1, 40, 52)
    want = (offline.refine_batch(masks, images, gk=0.5, iters=5) * 255.).astype(np.uint8)          # radius int(4 * 0.5 + 0.5) = 2
    got = offline.refine_batch_u8(masks, images, gk=0.5, iters=5)
    assert got.is_cuda and np.array_equal(got.cpu().numpy(), want)


SEQS = [("bear", ("00000", "00001")), ("swan", ("00003", "00004"))]
STEP = 4320


@pytest.fixture(scope="module")
def tree(tmp_path_factory):
    """two sequences of two 854 x 480 JPEG frames, their masks exported at half size; -> (root, the driver's inputs per two-frame
    group, what offline.refine_batch makes of each group)"""
    from PIL import Image
    root = str(tmp_path_factory.mktemp("postprocess_gpu"))
    H, W = postprocess.IMG_SIZE
    os.makedirs(os.path.join(root, "export"))
    k = 0
    for seq, frames in SEQS:
        os.makedirs(os.path.join(root, "images", seq))
        for f in frames:
            Image.fromarray(synth.smooth_rgb(H, W, 6100 + k)).save(os.path.join(root, "images", seq, f + ".jpg"), quality=95)
            top = (255, 190, 140, 230)[k]                                        # raw maxima on both sides of 204
            m = (synth.soft_blob_mask(H // 2, W // 2, 6100 + k) * top).astype(np.uint8)
            Image.fromarray(m).save(os.path.join(root, "export", f"pred_seg_{seq}_{f}_{STEP:07}.png"))
            k += 1
    groups, want = [], []
    for seq, frames in SEQS:
        loaded = [postprocess.load_frame(os.path.join(root, "images", seq, f + ".jpg"),
                                         os.path.join(root, "export", f"pred_seg_{seq}_{f}_{STEP:07}.png")) for f in frames]
        images, masks = np.stack([a for a, _ in loaded]), np.stack([b for _, b in loaded])
        groups.append((images, masks))
        want.append((offline.refine_batch(reference_prescale(masks), images) * 255.).astype(np.uint8))
    return root, groups, np.concatenate(want)


def _run(root, *more):
    from PIL import Image
    shutil.rmtree(os.path.join(root, "export_crf"), ignore_errors=True)
    written = postprocess.main(["--input", os.path.join(root, "images"), "--output", "unused", "--annotation-dir",
                                os.path.join(root, "export"), "--step", str(STEP), *more])
    assert written == [os.path.join(root, "export_crf", f"pred_seg_{seq}_{f}_{STEP:07}.png") for seq, frames in SEQS for f in frames]
    images = [Image.open(p) for p in written]
    assert all(im.mode == "L" and im.size == (854, 480) for im in images)
    return [open(p, "rb").read() for p in written], np.stack([np.asarray(im) for im in images])


def test_driver_end_to_end_at_480x854(tree, report):
    root, groups, want = tree
    files1, got = _run(root, "--batch-frames", "2", "--workers", "1")
    report(f"crf_postprocess 4 x 480x854, --batch-frames 2: bytes differing from offline.refine_batch on the same groups "
           f"{int((got != want).sum())}")
    assert np.array_equal(got, want)
    files4, got4 = _run(root, "--batch-frames", "2", "--workers", "4")
    assert files4 == files1
    _, got_b4 = _run(root, "--batch-frames", "4", "--seq", "bear", "swan")
    diff = [int((a != b).sum()) for a, b in zip(got_b4, want)]
    # what the CRF did: against the input's own labelling, U > 0.5 of the unary (the scaled mask over its maximum)
    masks = np.concatenate([reference_prescale(m) for _, m in groups])
    before = np.stack([np.where(m / (m.max() + 1e-8) > 0.5, 255, 0).astype(np.uint8) for m in masks])
    changed = [int((a != b).sum()) for a, b in zip(got, before)]
    report(f"crf_postprocess 4 x 480x854: pixels differing between --batch-frames 4 and 2 per frame {diff} of {got[0].size}; "
           f"pixels the CRF changed per frame {changed}")
    assert all(d <= 0.001 * got[0].size for d in diff)
    assert all(c > 0 for c in changed)
    assert set(np.unique(got)) <= {0, 255}
