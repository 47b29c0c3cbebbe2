// Region pixel enumeration and the conservative tap test of the forward / data-gradient conv kernels.  Plain C++ (no HIP
// types), so that a host build can check both against brute force (tests/test_region_order_cpu.py); included by rcf_common.h.
#pragma once

#if defined(__HIPCC__) || defined(__CUDACC__)
#define RCF_HD __host__ __device__
#else
#define RCF_HD
#endif

// Order of a frame's pixels.
// RCF_REGION_ROWMAJOR: the top strip (t x rw), the bottom strip, then the left and right strips (each (rh - 2t) x t), all row-major
// -- the weight gradients' summation order.
// RCF_REGION_BYDEPTH: the strips without the corners -- top and bottom middle (t x (rw - 2t)) line by line, left and right
// ((rh - 2t) x t) COLUMN by column -- then the four t x t corners.  Consecutive pixels then share their distance to the nearest
// edge, so a 128-row tile shares the taps that leave the image (or the source frame) and its K loop can drop them.
constexpr int RCF_REGION_ROWMAJOR = 0, RCF_REGION_BYDEPTH = 1;

// pixel `pix` (0 <= pix < rr) of a region -> image coordinates.  Rectangle (t <= 0): row-major in either order.
RCF_HD inline void rcf_region_yx(int pix, int ry0, int rx0, int rh, int rw, int t, int order, int &y, int &x) {
    if (t <= 0) {
        const int yr = pix / rw;
        y = yr + ry0;
        x = pix - yr * rw + rx0;
        return;
    }
    if (order == RCF_REGION_ROWMAJOR) {
        const int strip = t * rw;
        if (pix < 2 * strip) {
            const int bottom = pix >= strip;
            const int q = pix - (bottom ? strip : 0);
            const int yr = q / rw;
            y = ry0 + yr + (bottom ? rh - t : 0);
            x = rx0 + q - yr * rw;
        } else {
            int q = pix - 2 * strip;
            const int side = t * (rh - 2 * t);
            const int right = q >= side;
            q -= right ? side : 0;
            const int yr = q / t;
            y = ry0 + t + yr;
            x = rx0 + q - yr * t + (right ? rw - t : 0);
        }
        return;
    }
    const int wm = rw - 2 * t, hm = rh - 2 * t;
    const int strip = t * wm, side = t * hm;
    if (pix < 2 * strip) {
        const int bottom = pix >= strip;
        const int q = pix - (bottom ? strip : 0);
        const int yr = q / wm;
        y = ry0 + yr + (bottom ? rh - t : 0);
        x = rx0 + t + q - yr * wm;
    } else if (pix < 2 * strip + 2 * side) {
        int q = pix - 2 * strip;
        const int right = q >= side;
        q -= right ? side : 0;
        const int xc = q / hm;
        y = ry0 + t + q - xc * hm;
        x = rx0 + xc + (right ? rw - t : 0);
    } else {
        int q = pix - 2 * strip - 2 * side;
        const int k = q / (t * t);
        q -= k * t * t;
        const int yr = q / t;
        y = ry0 + yr + ((k & 2) ? rh - t : 0);
        x = rx0 + q - yr * t + ((k & 1) ? rw - t : 0);
    }
}

// Which taps of a GEMM row can read a value that is not zero by construction?  (ay, ax): the source coordinates of tap (0, 0);
// tap (r, s) reads (ay + r step, ax + s step), valid inside [0, Hs) x [0, Ws) -- and, band > 0, only on the border frame of that
// thickness (the source is taken as zero off it).  Bit r * S + s of the result; R * S <= 32.  Exact per row, so the OR over a tile's
// rows never drops a tap that some row needs.
RCF_HD inline unsigned rcf_row_taps(int ay, int ax, int R, int S, int step, int Hs, int Ws, int band) {
    const int lo = band > 0 ? band : (1 << 30);      // no frame: every valid source counts
    unsigned m = 0u;
    int bit = 0;
    for (int r = 0; r < R; ++r) {
        const int ty = ay + r * step;
        const bool vy = (unsigned)ty < (unsigned)Hs, fy = ty < lo || ty >= Hs - lo;
        for (int s = 0; s < S; ++s, ++bit) {
            const int tx = ax + s * step;
            const bool vx = (unsigned)tx < (unsigned)Ws, fx = tx < lo || tx >= Ws - lo;
            m |= (unsigned)(vy && vx && (fy || fx)) << bit;
        }
    }
    return m;
}
