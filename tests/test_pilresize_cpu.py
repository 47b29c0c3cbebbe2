"""CPU: rcf_amd.pilresize's host side -- the coefficient tables transcribed from Pillow's Resample.c and the numpy
restatement of its two 8-bit passes (resize_ref_np) against Pillow itself, bit for bit, over the shared case list
(tests/pilresize_cases.py); the tables' shapes, bounds and int32 headroom; the argument checks of rcf_pil_resample_u8 and the
tile-height rule (no GPU work)."""
import ctypes

import numpy as np
import pytest

import rcf_amd
from rcf_amd import _lib, pilresize as pr

import pilresize_cases as pc


@pytest.mark.parametrize("filter", pc.FILTERS)
def test_ref_np_equals_pillow(filter):
    """every case x 3 kinds of data: the restatement == Image.resize on RGB (channel 0) and on the L plane of channel 0"""
    assert len(pc.CASES) >= 40
    for i, (h, w, H, W) in enumerate(pc.CASES):
        for kind in pc.KINDS:
            a = pc.case_data(i, kind)
            got = pr.resize_ref_np(a, (H, W), filter)
            assert got.dtype == np.uint8 and got.shape == (a.shape[0], H, W)
            ref_rgb = pc.case_ref(i, filter, kind)[..., 0]
            ref_l = pc.pillow_resize(np.ascontiguousarray(a[..., 0]), (H, W), filter)
            assert np.array_equal(ref_rgb, ref_l), (i, kind)                 # Pillow's RGB path = its L path per channel
            nbad = int((got != ref_rgb).sum())
            assert nbad == 0, f"case {i} {h}x{w} -> {H}x{W} {filter} {kind}: {nbad} pixels differ from Pillow"
            assert np.array_equal(pr.resize_ref_np(np.ascontiguousarray(a[..., 0]), (H, W), filter), got)


def test_default_filter_is_pillows_default():
    """eval_tool.py calls Image.resize without a filter: that is the bicubic one for L and RGB"""
    from PIL import Image
    a = pc.frames(37, 53, "bytes", seed=99, N=1)
    for size in ((20, 31), (80, 97)):
        ref = np.array(Image.fromarray(a[0]).resize((size[1], size[0])))[..., 0]
        assert np.array_equal(pr.resize_ref_np(a, size)[0], ref)


def test_equal_sizes_copy_and_bad_inputs():
    a = pc.frames(8, 9, "bytes", seed=3)
    out = pr.resize_ref_np(a, (8, 9))
    assert np.array_equal(out, a[..., 0]) and not np.shares_memory(out, a)
    with pytest.raises(ValueError):
        pr.coeff_tables(10, 5, "lanczos")
    with pytest.raises(ValueError):
        pr.coeff_tables(10, 5, "hamming")
    with pytest.raises(ValueError):
        pr.coeff_tables(0, 5)
    with pytest.raises(ValueError):
        pr.resize_ref_np(a.astype(np.float32), (4, 4))
    with pytest.raises(ValueError):
        pr.resize_ref_np(a[..., :2], (4, 4))


def test_tables_shapes_bounds_and_int32_headroom():
    """every table the case list builds, on both axes: shape, taps inside the input, zero padding past the tap count, rows
    that sum to ~2^22, and 255 * sum |k| < 2^31 (the passes accumulate in int32)"""
    seen = 0
    for filter in pc.FILTERS:
        support = pr.FILTERS[filter][1]
        for h, w, H, W in pc.CASES:
            for n_in, n_out in ((h, H), (w, W)):
                k, b = pr.coeff_tables(n_in, n_out, filter)
                ksize = int(np.ceil(support * max(n_in / n_out, 1.0))) * 2 + 1
                assert k.dtype == np.int32 and b.dtype == np.int32
                assert k.shape == (n_out, ksize) and b.shape == (n_out, 2)
                assert (b[:, 0] >= 0).all() and (b[:, 1] >= 1).all() and (b[:, 1] <= ksize).all()
                assert (b[:, 0] + b[:, 1] <= n_in).all()
                assert (np.diff(b[:, 0]) >= 0).all()                         # what the kernel's tile-height rule relies on
                for i in range(n_out):
                    assert not k[i, b[i, 1]:].any()
                assert (255 * np.abs(k.astype(np.int64)).sum(axis=1) < 2 ** 31).all()
                assert (np.abs(k.astype(np.int64).sum(axis=1) - (1 << 22)) <= ksize).all()
                seen += 1
    assert seen == 6 * len(pc.CASES)
    k, b = pr.coeff_tables(480, 360)
    assert pr.coeff_tables(480, 360)[0] is k                                 # cached per (in, out, filter)
    assert not k.flags.writeable and not b.flags.writeable


def test_first_tap_spacing_bound():
    """rcf_pil_resample_tile_rows assumes t output rows read at most ksize + ceil((t - 1) in / out) + 1 input rows"""
    for filter in pc.FILTERS:
        for n_in, n_out in ((480, 360), (240, 480), (127, 2), (252, 4), (300, 13), (97, 33), (1000, 7)):
            k, b = pr.coeff_tables(n_in, n_out, filter)
            for t in (1, 2, 4, 8, 16, 32):
                for y0 in range(0, n_out, t):
                    rows = b[y0:y0 + t]
                    span = int((rows[:, 0] + rows[:, 1]).max() - rows[:, 0].min())
                    assert span <= k.shape[1] + -(-(t - 1) * n_in // n_out) + 1


def test_tile_rows_rule():
    assert pr.MAX_TAPS == 256
    assert pr.tile_rows(480, 360, pc.bicubic_taps(480, 360)) == 32
    assert pr.tile_rows(240, 480, pc.bicubic_taps(240, 480)) == 32
    assert pr.tile_rows(100, 100, 0) == 32                                   # no vertical pass
    assert pr.tile_rows(160, 20, pc.bicubic_taps(160, 20)) == 16
    assert pr.tile_rows(160, 10, pc.bicubic_taps(160, 10)) == 8
    assert pr.tile_rows(180, 6, pc.bicubic_taps(180, 6)) == 4
    assert pr.tile_rows(250, 5, pc.bicubic_taps(250, 5)) == 2
    assert pr.tile_rows(252, 4, pc.bicubic_taps(252, 4)) == 1
    assert pc.bicubic_taps(127, 2) == 255 and pr.tile_rows(127, 2, 255) == 1
    assert pr.tile_rows(512, 2, 256) == 1                                    # the cap itself
    assert pc.bicubic_taps(128, 2) == 257 and pr.tile_rows(128, 2, 257) == 0
    assert pr.device_ok(127, 2) and not pr.device_ok(128, 2) and pr.device_ok(128, 128)
    assert pr.device_ok(300, 2, "box")                                       # support 0.5: 151 taps
    assert pr.tile_rows(0, 4, 5) == 0 and pr.tile_rows(4, 0, 5) == 0 and pr.tile_rows(4, 4, -1) == 0


def test_entry_point_rejects_bad_arguments():
    lib = _lib.load()
    fake = ctypes.c_void_p(64)                  # never dereferenced: every call below is refused before any launch
    _, bad = pc.refused_calls(fake)
    assert len(bad) >= 25
    for why, args in bad:
        assert lib.rcf_pil_resample_u8(*args) == -1, why
    with pytest.raises(_lib.RcfHipError):
        _lib.call("rcf_pil_resample_u8", *bad[0][1])
