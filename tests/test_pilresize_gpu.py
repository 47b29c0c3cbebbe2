"""GPU: Pillow's 8-bit resize on the device (rcf_amd.pilresize, csrc/pil_resample.hip) against Pillow itself, bit for bit:
the CPU case list (tests/pilresize_cases.py) plus shapes taken from the kernel's own constants (64-column tiles, the tile
heights 32 ... 1, the 256-row window and its cap), the skipped passes, both pixel strides, the IoU counts, batching and a
non-default stream.  Every comparison is exact: no tolerance, no excluded elements."""
import ctypes

import numpy as np
import pytest
import torch

import rcf_amd
from rcf_amd import _lib, pilresize as pr
from rcf_amd.ops import _p, _stream

import pilresize_cases as pc

pytestmark = pytest.mark.gpu


def _check(a, size, filter="bicubic", ref=None):
    """resize_u8 of RGB frames a == Pillow (channel 0); returns Pillow's planes"""
    if ref is None:
        ref = pc.pillow_resize(a, size, filter)[..., 0]
    got = pr.resize_u8(a, size, filter)
    assert got.is_cuda and got.dtype == torch.uint8 and tuple(got.shape) == ref.shape
    nbad = int((got.cpu().numpy() != ref).sum())
    assert nbad == 0, f"{a.shape[1:3]} -> {size} {filter}: {nbad} of {ref.size} pixels differ from Pillow"
    return ref


@pytest.mark.parametrize("filter", pc.FILTERS)
def test_cpu_case_list_equals_pillow(filter, report):
    for i, (h, w, H, W) in enumerate(pc.CASES):
        for kind in pc.KINDS:
            _check(pc.case_data(i, kind), (H, W), filter, pc.case_ref(i, filter, kind)[..., 0])
    report(f"pil resize {filter}: {len(pc.CASES)} cases x {len(pc.KINDS)} kinds of data, 0 pixels differ from Pillow")


@pytest.mark.parametrize("W", [63, 64, 65, 129])
@pytest.mark.parametrize("H", [31, 32, 33])
def test_tile_edges(H, W):
    """output widths around the 64-column tile and heights around the 32-row tile, enlarging and reducing"""
    for h, w in ((20, 50), (47, 150)):
        assert pr.tile_rows(h, H, pc.bicubic_taps(h, H)) == 32
        _check(pc.frames(h, w, "bytes", seed=H * 1000 + W), (H, W))


# (h, H): vertical bicubic reductions by 2, 8, 16, 30, 50, 63 and 63.5 -- one per tile height the host can choose, the
# last one the largest the window admits (255 taps)
TILE_HEIGHT_SHAPES = [(32, 80, 40), (16, 160, 20), (8, 160, 10), (4, 180, 6), (2, 250, 5), (1, 252, 4), (1, 127, 2)]


@pytest.mark.parametrize("tile,h,H", TILE_HEIGHT_SHAPES)
def test_each_tile_height(tile, h, H):
    assert pr.tile_rows(h, H, pc.bicubic_taps(h, H)) == tile
    assert H > tile and (H % tile or tile == 1)                      # several blocks per column, the last tile partial
    _check(pc.frames(h, 70, "bytes", seed=h), (H, 65))
    _check(pc.frames(h, 9, "mask", seed=h + 1, N=1), (H, 9))         # vertical pass only


def test_past_the_cap_refused_and_fallback():
    """128 -> 2 rows is 257 bicubic taps: the entry point refuses, resize_u8 and resize_iou_counts go through the host"""
    h, w, H, W = 128, 12, 2, 7
    assert pc.bicubic_taps(h, H) == pr.MAX_TAPS + 1 and not pr.device_ok(h, H)
    a = pc.frames(h, w, "bytes", seed=5)
    src = torch.from_numpy(a).cuda()
    dst = torch.full((2, H, W), 7, dtype=torch.uint8, device="cuda")
    with pytest.raises(_lib.RcfHipError, match="bad argument"):
        pr._launch(src, (H, W), "bicubic", dst, None, 0, None)
    kx, bx, ksx = pr._device_tables(w, W, "bicubic", src.device)
    ky, by, ksy = pr._device_tables(h, H, "bicubic", src.device)
    assert ksy == 257
    rc = _lib.load().rcf_pil_resample_u8(_p(src), 2, h, w, 3, _p(kx), _p(bx), ksx, _p(ky), _p(by), ksy, H, W, _p(dst), None, 0,
                                         None, _stream())
    assert rc == -1
    torch.cuda.synchronize()
    assert (dst == 7).all()                                         # nothing was launched
    ref = _check(a, (H, W))
    gt = pc.frames(H, W, "mask", seed=6)[..., 1]
    assert np.array_equal(pr.resize_iou_counts(a, gt, 90), pr.iou_counts_np(ref, gt, 90))
    _check(pc.frames(127, w, "bytes", seed=7), (2, W))              # the largest reduction the device takes


@pytest.mark.parametrize("N", [1, 3])
def test_skipped_passes_and_pixel_strides(N):
    """kx only, ky only, neither; packed L planes and channel 0 of RGB read in place give the same bytes"""
    h, w = 45, 70
    a = pc.frames(h, w, "bytes", seed=40 + N, N=N)
    plane = np.ascontiguousarray(a[..., 0])
    for H, W in ((h, 131), (h, 33), (101, w), (17, w), (h, w), (60, 90), (30, 50)):
        ref = pc.pillow_resize(plane, (H, W))
        for src in (a, plane, torch.from_numpy(a).cuda(), torch.from_numpy(plane)):
            got = pr.resize_u8(src, (H, W))
            assert tuple(got.shape) == (N, H, W) and np.array_equal(got.cpu().numpy(), ref), (H, W)
        # through the kernel itself also where resize_u8 copies (neither pass)
        for s in (torch.from_numpy(a).cuda(), torch.from_numpy(plane).cuda()):
            dst = torch.zeros((N, H, W), dtype=torch.uint8, device="cuda")
            pr._launch(s, (H, W), "bicubic", dst, None, 0, None)
            assert np.array_equal(dst.cpu().numpy(), ref), (H, W, s.dim())
    t = torch.from_numpy(plane).cuda()
    c = pr.resize_u8(t, (h, w))
    assert c.data_ptr() != t.data_ptr() and torch.equal(c, t)       # equal sizes: a copy


@pytest.mark.parametrize("pred_min", [1, 90, 255])
def test_iou_counts_equal_numpy_on_pillows_result(pred_min):
    g = np.random.Generator(np.random.PCG64(pred_min))
    for h, w, H, W in ((48, 80, 97, 150), (120, 200, 45, 67), (60, 90, 60, 90), (64, 96, 64, 130), (90, 140, 40, 131),
                       (33, 17, 1, 1), (250, 9, 5, 65)):
        kind = "cluster" if pred_min == 90 else "bytes" if pred_min == 1 else "mask"
        a = pc.frames(h, w, kind, seed=h + W, N=3)
        a[1] = 0                                                    # frame 1: empty prediction ...
        gt = (g.integers(0, 3, size=(3, H, W)) == 0).astype(np.uint8) * g.integers(1, 256, size=(3, H, W)).astype(np.uint8)
        gt[1] = 0                                                   # ... and empty annotation: an empty union
        ref = pc.pillow_resize(a, (H, W))[..., 0]
        want = pr.iou_counts_np(ref, gt, pred_min)
        assert want[1].tolist() == [0, 0] and want[0, 1] > 0
        got = pr.resize_iou_counts(a, gt, pred_min)
        assert got.dtype == np.int64 and np.array_equal(got, want), (h, w, H, W)
        assert np.array_equal(pr.resize_iou_counts(torch.from_numpy(a).cuda(), torch.from_numpy(gt != 0).cuda(), pred_min), want)
        # counts together with dst: one launch writes the planes and adds to the counts
        src, gd = torch.from_numpy(a).cuda(), torch.from_numpy(gt).cuda()
        dst = torch.zeros((3, H, W), dtype=torch.uint8, device="cuda")
        counts = torch.zeros((3, 2), dtype=torch.int64, device="cuda")
        pr._launch(src, (H, W), "bicubic", dst, gd, pred_min, counts)
        assert np.array_equal(dst.cpu().numpy(), ref) and np.array_equal(counts.cpu().numpy(), want)
    with pytest.raises(ValueError):
        pr.resize_iou_counts(a, gt, 257)
    with pytest.raises(ValueError):
        pr.resize_iou_counts(a, gt[:2], 90)


def test_pred_min_extremes():
    a = pc.frames(20, 30, "bytes", seed=1, N=1)
    gt = np.zeros((1, 25, 35), dtype=np.uint8)
    assert pr.resize_iou_counts(a, gt, 0).tolist() == [[0, 25 * 35]]          # every pixel predicted on
    assert pr.resize_iou_counts(a, gt, 256).tolist() == [[0, 0]]              # none


def test_batched_equals_per_frame_and_stream_invariance():
    h, w, H, W = 60, 100, 45, 130
    a = pc.frames(h, w, "cluster", seed=77, N=5)
    gt = pc.frames(H, W, "mask", seed=78, N=5)[..., 2]
    whole = pr.resize_u8(a, (H, W)).cpu().numpy()
    counts = pr.resize_iou_counts(a, gt, 90)
    for n in range(5):
        assert np.array_equal(pr.resize_u8(a[n:n + 1], (H, W)).cpu().numpy()[0], whole[n])
        assert np.array_equal(pr.resize_iou_counts(a[n:n + 1], gt[n:n + 1], 90)[0], counts[n])
    s = torch.cuda.Stream()
    with torch.cuda.stream(s):
        other = pr.resize_u8(a, (H, W))
        counts_s = pr.resize_iou_counts(a, gt, 90)
    s.synchronize()
    assert np.array_equal(other.cpu().numpy(), whole) and np.array_equal(counts_s, counts)


def test_any_table_with_taps_inside_the_frame():
    """the kernel knows no filter: a hand-made vertical table whose consecutive rows read opposite ends of a 600-row frame
    (no tile of it fits the 256-row window, so the block walks its rows in several runs) and a mirrored horizontal one"""
    N, h, w, H, W = 2, 600, 40, 37, 40
    g = np.random.Generator(np.random.PCG64(8))
    a = g.integers(0, 256, size=(N, h, w), dtype=np.uint8)
    ksy = 3
    by = np.zeros((H, 2), dtype=np.int32)
    ky = np.zeros((H, ksy), dtype=np.int32)
    for y in range(H):
        first = (7 * y) % 50 if y % 2 == 0 else h - ksy - (11 * y) % 50
        by[y] = (first, 1 + y % ksy)
        ky[y, :by[y, 1]] = g.integers(-(1 << 20), 1 << 21, size=by[y, 1])      # 3 * 255 * 2^21 < 2^31
    bx = np.stack([w - 1 - np.arange(W), np.ones(W)], axis=1).astype(np.int32)        # a mirror: one tap of weight one
    kx = np.full((W, 1), 1 << 22, dtype=np.int32)
    mirrored = pr._pass_np(a.astype(np.int64), (kx, bx), 2)        # the restatement's pass takes any table
    ref = pr._pass_np(mirrored, (ky, by), 1).astype(np.uint8)
    assert np.array_equal(mirrored, a[:, :, ::-1]) and 0 < ref.mean() < 255
    dev = lambda t: torch.from_numpy(t).cuda()
    src, dst = dev(a), torch.zeros((N, H, W), dtype=torch.uint8, device="cuda")
    tabs = [dev(kx), dev(bx), dev(ky), dev(by)]
    _lib.call("rcf_pil_resample_u8", _p(src), N, h, w, 1, _p(tabs[0]), _p(tabs[1]), 1, _p(tabs[2]), _p(tabs[3]), ksy, H, W,
              _p(dst), None, 0, None, _stream())
    assert np.array_equal(dst.cpu().numpy(), ref)


def test_entry_point_rejects_bad_arguments_with_real_buffers():
    """null pointers, non-positive sizes, pix_stride outside {1, 3}, neither dst nor counts, ... : RCF_EINVAL and no launch"""
    buf = torch.zeros(4096, dtype=torch.uint8, device="cuda")
    good, bad = pc.refused_calls(ctypes.c_void_p(buf.data_ptr()))
    lib = _lib.load()
    for why, args in bad:
        assert lib.rcf_pil_resample_u8(*args) == -1, why
    torch.cuda.synchronize()
    assert not buf.any()
