// PWC-Lite's cost volume and its two gradients.  Reference: models/amd/correlation_native.py:6-23 (pad x2 by d, the D x D = (2d+1)^2
// shifted products x1 * x2[.., i:i+H, j:j+W], mean over the channels, concatenated with the row displacement i outermost) followed
// by the LeakyReLU(0.1) of models/amd/pwc_lite.py:202-203 (slope != 1), and what autograd makes of the two.  Planar NCHW fp32.
//
//   out[b, i D + j, y, x] = act( (1/C) sum_c x1[b,c,y,x] x2z[b,c, y+i-d, x+j-d] )
//   dx1[b, c, y, x]       = (1/C) sum_ij g[b, i D + j, y, x]         x2z[b,c, y+i-d, x+j-d]
//   dx2[b, c, y, x]       = (1/C) sum_ij g[b, i D + j, y-i+d, x-j+d] x1z[b,c, y-i+d, x-j+d]
//
// x2z / x1z: the operand with real zeros outside the image (the zeros are multiplied, an infinite partner makes NaN as F.pad's
// zeros do; a g whose source pixel lies outside the image is dropped, as the pad's backward drops it).  The reference runs ~165
// launches forward and several hundred backward for this; all three results are the same gather, and one kernel template does
// them: a thread owns one pixel of an 8 x 32 tile and keeps D x D values in registers (forward: the sums; gradients: g), the
// workgroup stages COR_CK channels of the OTHER operand's tile plus a d-wide halo in LDS -- the next trip's values are already
// on their way in registers while the current ones are multiplied -- and walks the channels.  No atomics: every sum runs in one
// thread in a fixed order (channels ascending; (i, j) row-major), so all three results are bit-reproducible.
// LDS rows are read by 32 consecutive lanes at consecutive dwords (conflict-free at any row pitch); d = 4 stages
// 8 x 16 x 40 floats = 20 KB.  Register / LDS / scratch figures: LABNOTES.md.
#include "rcf_common.h"

namespace {

constexpr int COR_TH = 8, COR_TW = 32, COR_CK = 8;     // tile rows, tile columns (TH * TW = 256 threads), channels staged per trip
enum { COR_FWD = 0, COR_DX1 = 1, COR_DX2 = 2 };

template <int d> struct CorTile {
    static constexpr int D = 2 * d + 1, TH2 = COR_TH + 2 * d, TW2 = COR_TW + 2 * d, PLANE = TH2 * TW2, N = COR_CK * PLANE;
    static constexpr int PER = (N + 255) / 256;         // staged values per thread and trip
};

// channels [c0, c0 + COR_CK) of the window [ty0 - d, ty0 + TH + d) x [tx0 - d, tx0 + TW + d) of image `src` ([C][H][W]) into
// registers, zeros outside the image and past the last channel
template <int d>
__device__ __forceinline__ void cor_fetch(float (&pre)[CorTile<d>::PER], const float *__restrict__ src, int c0, int C, int H,
                                          int W, int ty0, int tx0) {
    using T = CorTile<d>;
#pragma unroll
    for (int k = 0; k < T::PER; ++k) {
        const int idx = (int)threadIdx.x + 256 * k;
        const int cc = idx / T::PLANE, rem = idx - cc * T::PLANE;
        const int ly = rem / T::TW2, lx = rem - ly * T::TW2;
        const int gy = ty0 - d + ly, gx = tx0 - d + lx, c = c0 + cc;
        const bool ok = idx < T::N && c < C && gy >= 0 && gy < H && gx >= 0 && gx < W;
        float v = 0.f;
        if (ok) v = src[((long)c * H + gy) * W + gx];
        pre[k] = v;
    }
}

// MODE COR_FWD: res = out, staged operand x2.  COR_DX1: res = dx1, staged x2.  COR_DX2: res = dx2, staged x1, taps mirrored.
// act: the forward's output when slope != 1 (the gradients' LeakyReLU mask), else null.
template <int d, int MODE>
__global__ void __launch_bounds__(256) correlation_kernel(const float *__restrict__ x1, const float *__restrict__ x2,
                                                          const float *__restrict__ dout, const float *__restrict__ act,
                                                          float *__restrict__ res, int C, int H, int W, float slope,
                                                          int tiles_x, int tiles_y) {
    using T = CorTile<d>;
    constexpr int D = T::D;
    __shared__ float tile[T::N];
    int bid = (int)blockIdx.x;
    const int txi = bid % tiles_x;
    bid /= tiles_x;
    const int tyi = bid % tiles_y, b = bid / tiles_y;
    const int lx = (int)threadIdx.x % COR_TW, ly = (int)threadIdx.x / COR_TW;
    const int y0 = tyi * COR_TH, x0 = txi * COR_TW, y = y0 + ly, x = x0 + lx;
    const bool live = y < H && x < W;
    const long HW = (long)H * W, pix = (long)y * W + x;
    const float *staged = (MODE == COR_DX2 ? x1 : x2) + (long)b * C * HW;
    const float fC = (float)C;

    float r[D * D];
    if (MODE == COR_FWD) {
#pragma unroll
        for (int k = 0; k < D * D; ++k) r[k] = 0.f;
    } else {
        const float *gb = dout + (long)b * (D * D) * HW;
        const float *ab = act ? act + (long)b * (D * D) * HW : nullptr;
#pragma unroll
        for (int i = 0; i < D; ++i)
#pragma unroll
            for (int j = 0; j < D; ++j) {
                const int k = i * D + j;
                const int ys = MODE == COR_DX2 ? y - i + d : y, xs = MODE == COR_DX2 ? x - j + d : x;
                const bool ok = live && ys >= 0 && ys < H && xs >= 0 && xs < W;
                float g = 0.f;
                if (ok) {
                    const long q = k * HW + (long)ys * W + xs;
                    g = gb[q];
                    if (ab) g = ab[q] > 0.f ? g : g * slope;
                }
                r[k] = g;
            }
    }

    float pre[T::PER];
    cor_fetch<d>(pre, staged, 0, C, H, W, y0, x0);
    const float *t0 = tile + ly * T::TW2 + lx;
    for (int c0 = 0; c0 < C; c0 += COR_CK) {
#pragma unroll
        for (int k = 0; k < T::PER; ++k) {
            const int idx = (int)threadIdx.x + 256 * k;
            if (idx < T::N) tile[idx] = pre[k];
        }
        __syncthreads();
        if (c0 + COR_CK < C) cor_fetch<d>(pre, staged, c0 + COR_CK, C, H, W, y0, x0);
        const int n = min(COR_CK, C - c0);
        if (MODE == COR_FWD) {
            const float *a = x1 + ((long)b * C + c0) * HW + pix;
            float va[COR_CK];
#pragma unroll
            for (int cc = 0; cc < COR_CK; ++cc) {
                va[cc] = 0.f;
                if (live && cc < n) va[cc] = a[cc * HW];
            }
#pragma unroll
            for (int cc = 0; cc < COR_CK; ++cc) {
                if (cc < n) {                       // the same in every lane
                    const float *t = t0 + cc * T::PLANE;
#pragma unroll
                    for (int i = 0; i < D; ++i)
#pragma unroll
                        for (int j = 0; j < D; ++j) r[i * D + j] += va[cc] * t[i * T::TW2 + j];
                }
            }
        } else {
            float *o = res + ((long)b * C + c0) * HW + pix;
            for (int cc = 0; cc < n; ++cc) {
                const float *t = t0 + cc * T::PLANE;
                float s = 0.f;
#pragma unroll
                for (int i = 0; i < D; ++i)
#pragma unroll
                    for (int j = 0; j < D; ++j) {
                        const int ii = MODE == COR_DX2 ? 2 * d - i : i, jj = MODE == COR_DX2 ? 2 * d - j : j;
                        s += r[i * D + j] * t[ii * T::TW2 + jj];
                    }
                if (live) o[cc * HW] = s / fC;
            }
        }
        __syncthreads();
    }
    if (MODE == COR_FWD && live) {
        float *o = res + (long)b * (D * D) * HW + pix;
#pragma unroll
        for (int k = 0; k < D * D; ++k) {
            float v = r[k] / fC;
            if (slope != 1.f) v = v > 0.f ? v : slope * v;
            o[k * HW] = v;
        }
    }
}

// sizes, the displacement range, and every tensor (the D x D-plane one included) under 2^31 elements
inline bool cor_shape_ok(int B, int C, int H, int W, int d) {
    if (B <= 0 || C <= 0 || H <= 0 || W <= 0 || d < 1 || d > 4) return false;
    const long lim = 1L << 31, D2 = (long)(2 * d + 1) * (2 * d + 1);
    long n = (long)B * H;
    if (n >= lim) return false;
    n *= W;
    if (n >= lim) return false;
    return n * C < lim && n * D2 < lim;
}

template <int MODE>
int cor_launch(const float *x1, const float *x2, const float *dout, const float *act, float *res, int B, int C, int H, int W, int d,
               float slope, hipStream_t st) {
    const int tx = rcf_cdiv(W, COR_TW), ty = rcf_cdiv(H, COR_TH);
    const dim3 grid((unsigned)((long)B * tx * ty)), block(256);
#define COR_GO(dd)                                                                                                              \
    hipLaunchKernelGGL((correlation_kernel<dd, MODE>), grid, block, 0, st, x1, x2, dout, act, res, C, H, W, slope, tx, ty)
    switch (d) {
    case 1: COR_GO(1); break;
    case 2: COR_GO(2); break;
    case 3: COR_GO(3); break;
    default: COR_GO(4); break;
    }
#undef COR_GO
    RCF_LAUNCH_CHECK();
    return 0;
}

}  // namespace

extern "C" int rcf_correlation_geometry(int which) {
    return which == 0 ? COR_TH : which == 1 ? COR_TW : which == 2 ? COR_CK : 0;
}

extern "C" int rcf_correlation_fwd_f32(const float *x1, const float *x2, float *out, int B, int C, int H, int W, int max_disp,
                                       float slope, void *stream) {
    if (!cor_shape_ok(B, C, H, W, max_disp)) return RCF_EINVAL;
    if (!x1 || !x2 || !out) return RCF_EINVAL;
    return cor_launch<COR_FWD>(x1, x2, nullptr, nullptr, out, B, C, H, W, max_disp, slope, rcf_stream(stream));
}

extern "C" int rcf_correlation_bwd_f32(const float *x1, const float *x2, const float *dout, const float *out, float *dx1,
                                       float *dx2, int B, int C, int H, int W, int max_disp, float slope, void *stream) {
    if (!cor_shape_ok(B, C, H, W, max_disp)) return RCF_EINVAL;
    if (!x1 || !x2 || !dout || (!dx1 && !dx2) || (slope != 1.f && !out)) return RCF_EINVAL;
    const float *act = slope != 1.f ? out : nullptr;
    if (dx1) {
        const int rc = cor_launch<COR_DX1>(x1, x2, dout, act, dx1, B, C, H, W, max_disp, slope, rcf_stream(stream));
        if (rc) return rc;
    }
    if (dx2) return cor_launch<COR_DX2>(x1, x2, dout, act, dx2, B, C, H, W, max_disp, slope, rcf_stream(stream));
    return 0;
}
