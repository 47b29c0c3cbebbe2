// The one copy of what the flow family (csrc/warp.hip, csrc/unflow.hip) shares on the device: the sample position of
// utils/warp_utils.py's flow_warp (mesh_grid + norm_grid + grid_sample, align_corners True) in the reference's float order, the
// bilinear taps and their blend, the derivative of a sample by its position, and the fixed-order block sum of doubles.  The library is
// compiled without contraction, so the same lines give the same bits in every kernel that includes them.
#pragma once
#include "rcf_common.h"

namespace {

// The sample position of one axis, as tests/warp_cases.py::sample_pos, in two steps so that a caller does the arithmetic of both
// axes before the clips' branches (the two IEEE divisions then overlap):
// norm_grid (utils/warp_utils.py:17-24), then grid_sampler_unnormalize(align_corners=True) ...
__device__ __forceinline__ float grid_pos(float p, int size) {
    const float d = (float)(size - 1);
    const float g = 2.0f * p / d - 1.0f;
    return ((g + 1.f) / 2.f) * d;
}
// ... and border mode's clip_coordinates; returns whether the gradient wrt the coordinate survives the clip
__device__ __forceinline__ bool clip_pos(float &i, int size) {
    const float d = (float)(size - 1);
    if (!(i > 0.f)) { i = 0.f; return false; }
    if (i >= d) { i = d; return false; }
    return true;
}

struct Taps {
    int x0, y0;
    float wx, wy;     // fractional parts
    bool inx0, inx1, iny0, iny1;
    bool gx_live, gy_live;   // gradient wrt coordinate survives clipping
};

// pad_mode 0 = border, 1 = zeros
__device__ __forceinline__ Taps make_taps(float px, float py, int W, int H, int pad_mode) {
    Taps t;
    float ix = grid_pos(px, W), iy = grid_pos(py, H);
    t.gx_live = t.gy_live = true;
    if (pad_mode == 0) {
        t.gx_live = clip_pos(ix, W);
        t.gy_live = clip_pos(iy, H);
    }
    const float fx = floorf(ix), fy = floorf(iy);
    t.wx = ix - fx;
    t.wy = iy - fy;
    // huge |flow| -> keep the int conversion defined
    t.x0 = (int)fminf(fmaxf(fx, -2.f), (float)W + 1.f);
    t.y0 = (int)fminf(fmaxf(fy, -2.f), (float)H + 1.f);
    t.inx0 = t.x0 >= 0 && t.x0 < W;
    t.inx1 = t.x0 + 1 >= 0 && t.x0 + 1 < W;
    t.iny0 = t.y0 >= 0 && t.y0 < H;
    t.iny1 = t.y0 + 1 >= 0 && t.y0 + 1 < H;
    return t;
}

// same order of operations as grid_sample's accumulation: row 0 (x0, x0+1), then row 1
__device__ __forceinline__ float blend4(float v00, float v01, float v10, float v11, float w00, float w01, float w10, float w11) {
    float v = 0.f;
    v += v00 * w00 + v01 * w01;
    v += v10 * w10 + v11 * w11;
    return v;
}

// d sample / d (x, y) from the four tap values
__device__ __forceinline__ void sample_dpos(float v00, float v01, float v10, float v11, const Taps &t, float &dx, float &dy) {
    const float ex = 1.f - t.wx, ey = 1.f - t.wy;
    dx = ey * (v01 - v00) + t.wy * (v11 - v10);
    dy = ex * (v10 - v00) + t.wx * (v11 - v01);
}

typedef float f32x2_a4 __attribute__((ext_vector_type(2), aligned(4)));   // 8-byte load, dword aligned

// Branch-free bilinear sample: the two horizontal taps of a row are adjacent, so each row is ONE 8-byte load at a
// clamped (always valid) position; taps that fall outside the image get weight 0 through selects, never through
// control flow -- all tap loads of a pixel (2 per channel) issue back to back.
struct Sampler {
    int off0, off1;          // float offsets of the two row loads inside a plane
    float w00, w01, w10, w11;   // weights of (row0: x0, x0+1), (row1: x0, x0+1); 0 for taps outside
    bool s00, s01;           // which element of the loaded pair is tap x0 / x0+1 (false = [0], true = [1])
};
__device__ __forceinline__ Sampler make_sampler(const Taps &t, int W, int H) {
    Sampler s;
    const int xb = min(max(t.x0, 0), W - 2);                 // pair base: both elements inside the row
    const int y0c = min(max(t.y0, 0), H - 1), y1c = min(max(t.y0 + 1, 0), H - 1);
    s.off0 = y0c * W + xb;
    s.off1 = y1c * W + xb;
    s.s00 = t.x0 != xb;                                       // x0 == xb + 1 (only when x0 == W-1)
    s.s01 = t.x0 + 1 != xb;                                   // false only when x0 == -1
    const float ex = 1.f - t.wx, ey = 1.f - t.wy;
    const float m0 = t.inx0 ? 1.f : 0.f, m1 = t.inx1 ? 1.f : 0.f, r0 = t.iny0 ? 1.f : 0.f, r1 = t.iny1 ? 1.f : 0.f;
    s.w00 = ey * ex * m0 * r0;
    s.w01 = ey * t.wx * m1 * r0;
    s.w10 = t.wy * ex * m0 * r1;
    s.w11 = t.wy * t.wx * m1 * r1;
    return s;
}
__device__ __forceinline__ float sample(const float *__restrict__ plane, const Sampler &s) {
    const f32x2_a4 a = *reinterpret_cast<const f32x2_a4 *>(plane + s.off0);
    const f32x2_a4 b = *reinterpret_cast<const f32x2_a4 *>(plane + s.off1);
    return blend4(s.s00 ? a[1] : a[0], s.s01 ? a[1] : a[0], s.s00 ? b[1] : b[0], s.s01 ? b[1] : b[0], s.w00, s.w01, s.w10, s.w11);
}

// sums of K doubles over the 256 threads in a fixed order, ((w0 + w1) + w2) + w3 over the wavefronts; every thread gets the totals.
// sh: 4 K doubles of LDS
template <int K> __device__ __forceinline__ void block_sum_d(double (&v)[K], double *sh) {
    const int lane = threadIdx.x & 63, wv = threadIdx.x >> 6;
#pragma unroll
    for (int k = 0; k < K; ++k) v[k] = wave_sum_d(v[k]);         // all K reductions before the one branch: their shuffles overlap
    if (lane == 0) {
#pragma unroll
        for (int k = 0; k < K; ++k) sh[wv * K + k] = v[k];
    }
    __syncthreads();
#pragma unroll
    for (int k = 0; k < K; ++k) v[k] = ((sh[k] + sh[K + k]) + sh[2 * K + k]) + sh[3 * K + k];
    __syncthreads();
}

}  // namespace
