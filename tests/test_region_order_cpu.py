"""csrc/region_order.h built for the host: the two enumerations of a frame region's pixels and the conservative tap test of the
forward / data-gradient tile kernel, against brute force."""
import ctypes
import os
import shutil
import subprocess

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HEADER = os.path.join(ROOT, "rcf-unsupvideoseg_amd", "csrc", "region_order.h")
FRAMES = [(30, 37, 13), (30, 37, 7), (120, 214, 13), (5, 5, 2), (30, 37, 0), (7, 9, 0), (9, 8, 3)]

SRC = r"""
#include "region_order.h"
extern "C" void region_all(int rr, int ry0, int rx0, int rh, int rw, int t, int order, int *yx) {
    for (int p = 0; p < rr; ++p) rcf_region_yx(p, ry0, rx0, rh, rw, t, order, yx[2 * p], yx[2 * p + 1]);
}
extern "C" void row_taps_all(int n, const int *ay, const int *ax, int R, int S, int step, int Hs, int Ws, int band, unsigned *out) {
    for (int i = 0; i < n; ++i) out[i] = rcf_row_taps(ay[i], ax[i], R, S, step, Hs, Ws, band);
}
"""


@pytest.fixture(scope="module")
def lib(tmp_path_factory):
    cxx = next((c for c in (shutil.which("c++"), shutil.which("g++"), shutil.which("clang++"),
                            os.environ.get("HIPCC", "/opt/rocm/bin/hipcc")) if c and os.path.exists(c)), None)
    assert cxx is not None, "no C++ compiler to build csrc/region_order.h for the host"
    d = tmp_path_factory.mktemp("region_order")
    src, so = str(d / "region_order.cpp"), str(d / "libregion_order.so")
    with open(src, "w") as f:
        f.write(SRC)
    subprocess.run([cxx, "-x", "c++", "-std=c++17", "-O1", "-shared", "-fPIC", "-I", os.path.dirname(HEADER), src, "-o", so], check=True,
                   capture_output=True, timeout=300)
    return ctypes.CDLL(so)


def pixels(rh, rw, t):
    return 2 * t * rw + 2 * t * (rh - 2 * t) if t > 0 else rh * rw


def enumerate_region(lib, rh, rw, t, order, ry0=0, rx0=0):
    rr = pixels(rh, rw, t)
    yx = np.zeros((rr, 2), dtype=np.int32)
    lib.region_all(rr, ry0, rx0, rh, rw, t, order, yx.ctypes.data_as(ctypes.c_void_p))
    return yx


def region_yx_before(pix, ry0, rx0, rh, rw, t):
    """the enumeration the kernels used before there were two (igemm_conv.hip region_yx, transcribed)"""
    if t <= 0:
        return pix // rw + ry0, pix % rw + rx0
    strip = t * rw
    if pix < 2 * strip:
        bottom = pix >= strip
        q = pix - (strip if bottom else 0)
        return ry0 + q // rw + (rh - t if bottom else 0), rx0 + q % rw
    q = pix - 2 * strip
    side = t * (rh - 2 * t)
    right = q >= side
    q -= side if right else 0
    return ry0 + t + q // t, rx0 + q % t + (rw - t if right else 0)


@pytest.mark.parametrize("frame", FRAMES)
def test_orders_visit_every_pixel_once(lib, frame):
    rh, rw, t = frame
    ry0, rx0 = 2, 3
    want = {(y + ry0, x + rx0) for y in range(rh) for x in range(rw) if t <= 0 or y < t or y >= rh - t or x < t or x >= rw - t}
    assert len(want) == pixels(rh, rw, t)
    for order in (0, 1):
        yx = enumerate_region(lib, rh, rw, t, order, ry0, rx0)
        got = [tuple(int(v) for v in p) for p in yx]
        assert len(set(got)) == len(got) == len(want) and set(got) == want
    old = enumerate_region(lib, rh, rw, t, 0, ry0, rx0)
    assert [tuple(int(v) for v in p) for p in old] == [region_yx_before(p, ry0, rx0, rh, rw, t) for p in range(len(old))]


def test_by_depth_runs_share_their_depth(lib):
    """what the order is for: outside the corners, 128 consecutive pixels of the 13-frame of 120 x 214 span at most 3 depths"""
    rh, rw, t = 120, 214, 13
    yx = enumerate_region(lib, rh, rw, t, 1)
    depth = np.minimum(np.minimum(yx[:, 0], rh - 1 - yx[:, 0]), np.minimum(yx[:, 1], rw - 1 - yx[:, 1]))
    body = pixels(rh, rw, t) - 4 * t * t
    for p0 in range(0, body - 128, 128):
        assert len(set(depth[p0:p0 + 128].tolist())) <= 3


# (rows' region, conv geometry): decode_head2's band -- the data gradient (13-frame of the input, dy on the 7-frame, taps step back
# by the dilation from y + pad) and the forward (7-frame of the output, taps step forward from y - pad) -- and a whole tensor
GEOMETRIES = [
    ("dgrad", (30, 37, 13), 6, 7), ("dgrad", (120, 214, 13), 6, 7), ("fwd", (30, 37, 7), 6, 0), ("fwd", (120, 214, 7), 6, 0),
    ("dgrad", (5, 5, 2), 1, 1), ("fwd", (10, 40, 0), 6, 0), ("dgrad", (10, 40, 0), 6, 0), ("dgrad", (9, 8, 3), 2, 2),
]


@pytest.mark.parametrize("geo", GEOMETRIES)
def test_tile_tap_list_is_conservative(lib, geo):
    """for every tile of 128 rows (two images back to back, an M tail), in both orders: a tap the tile's list drops has no
    valid source in any row of the tile -- sources judged by brute force here"""
    kind, (rh, rw, t), d, band = geo
    H, W, N = rh, rw, 2
    off, step = (d, -d) if kind == "dgrad" else (-d, d)
    kept = total = 0
    for order in (0, 1):
        yx = enumerate_region(lib, rh, rw, t, order)
        rows = np.concatenate([yx] * N)
        ay = np.ascontiguousarray(rows[:, 0] + off, dtype=np.int32)
        ax = np.ascontiguousarray(rows[:, 1] + off, dtype=np.int32)
        got = np.zeros(len(rows), dtype=np.uint32)
        lib.row_taps_all(len(rows), ay.ctypes.data_as(ctypes.c_void_p), ax.ctypes.data_as(ctypes.c_void_p), 3, 3, step, H, W, band,
                         got.ctypes.data_as(ctypes.c_void_p))
        # brute force: per row and tap, is the source pixel inside the image and (band > 0) on the frame?
        want = np.zeros(len(rows), dtype=np.uint32)
        for r in range(3):
            for s in range(3):
                ty, tx = ay.astype(np.int64) + r * step, ax.astype(np.int64) + s * step
                ok = (ty >= 0) & (ty < H) & (tx >= 0) & (tx < W)
                if band > 0:
                    ok &= (ty < band) | (ty >= H - band) | (tx < band) | (tx >= W - band)
                want |= ok.astype(np.uint32) << np.uint32(3 * r + s)
        for m0 in range(0, len(rows), 128):
            tile = np.bitwise_or.reduce(got[m0:m0 + 128])
            need = np.bitwise_or.reduce(want[m0:m0 + 128])
            assert need & ~tile == 0, f"{geo} order {order} tile at row {m0} drops a tap some row reads"
            if order == 1:
                kept += bin(int(tile)).count("1")
                total += 9
    assert kept <= total
    if geo == ("dgrad", (120, 214, 13), 6, 7):
        assert kept < 0.6 * total          # the geometry's promise: a tile of the band's data gradient drops over 40 % of its taps
