// The seam of the AMD baseline (models/amd/amd_model.py) between the segmentation network on the tape and the flow network under
// torch autograd: the mask softmax that turns decode_head2's NHWC logits into the planar frame-major masks PWCLite.forward takes, its
// backward into NHWC logit gradients, and the de-normalised, resized frame pair of models/fcn_head.py:160-170.  All fp32 tensors;
// streaming kernels of 256 threads, one pixel (softmax) or one output element (frame pair) per thread, no atomics, no sums across
// threads: the same bits on every call.
//
// Error against exact arithmetic on the same inputs, per element, is k 2^-24 mass; k is the number of roundings on the longest path
// plus 2:
//   softmax forward    k = 3    mass = the mask value p_c itself.  The differences x_c - max, the exponentials, their sum (c upwards) and
//                               the quotient are taken in fp64 (rounding 2^-29 of fp32's; M exponentials per pixel on tensors of a few
//                               MB), one rounding to float; below FLT_MIN the spacing 2^-149 takes over.  So the bound does not grow
//                               with the spread of the logits.
//   softmax backward   k = 3    mass = |p_c| (|dp_c| + sum_k |p_k dp_k|).  p_c (dp_c - sum_k p_k dp_k): the products of two floats are
//                               exact in fp64, the sum (k upwards), the difference and the last product are fp64, one rounding to float.
//   frame pair         k = 19   mass = the same bilinear blend of (|x| std_c + mean_c) / 255.  Three roundings de-normalise a tap
//                               (product, sum, IEEE division, the reference's order on the CPU), then the blend of
//                               rcf_resize_bilinear_nchw_f32 (k = 16, csrc/resize_pos.h) on float32 source positions.
// A NaN or +inf logit makes every mask of its pixel NaN, as torch's softmax does (inf - inf); -inf gives 0.
#include "resize_pos.h"

namespace {

constexpr int AM_PIX = 256;        // pixels of one image per workgroup of the softmax kernels
constexpr int AM_MAXM = 8;         // masks (live logit channels) per pixel
constexpr int AM_MAXI = 8;         // frames per sample

struct AmFrames { const float *g[AM_MAXI]; };      // the frames' mask gradients, NULL = zeros

// logits[n][p][0 .. M) of image n = b I + i (batch-major, as the network sees the frames) -> masks[i][b][m][p] (frame-major, planar).
// CV float4 reads per pixel, M stores that are contiguous along the pixels of a wavefront.
template <int CV>
__global__ void __launch_bounds__(256) am_softmax_fwd_kernel(const float *__restrict__ logits, int pitch, float *__restrict__ masks, int I,
                                                             int B, int M, int hw) {
    const int p = (int)blockIdx.x * AM_PIX + (int)threadIdx.x, n = (int)blockIdx.y;
    if (p >= hw) return;
    const int b = n / I, i = n - b * I;
    const float *src = logits + ((long)n * hw + p) * pitch;
    float v[4 * CV];
#pragma unroll
    for (int q = 0; q < CV; ++q) {
        const f32x4 t = ld4(src + 4 * q);
#pragma unroll
        for (int e = 0; e < 4; ++e) v[4 * q + e] = t[e];
    }
    float mx = v[0];
#pragma unroll
    for (int c = 1; c < 4 * CV; ++c)
        if (c < M) mx = v[c] > mx ? v[c] : mx;
    double ex[4 * CV], sum = 0;
#pragma unroll
    for (int c = 0; c < 4 * CV; ++c) {
        if (c < M) {
            ex[c] = exp((double)v[c] - (double)mx);
            sum = c == 0 ? ex[c] : sum + ex[c];
        }
    }
    float *dst = masks + (((long)i * B + b) * M) * hw + p;
#pragma unroll
    for (int c = 0; c < 4 * CV; ++c)
        if (c < M) dst[(long)c * hw] = (float)(ex[c] / sum);
}

// dlogits[n][p][c] = p_c (dp_c - sum_k p_k dp_k) for c < M, 0 for M <= c < 4 CV; channels from 4 CV up to the pitch are left alone
template <int CV>
__global__ void __launch_bounds__(256) am_softmax_bwd_kernel(const float *__restrict__ masks, AmFrames dmasks, float *__restrict__ dlogits,
                                                             int pitch, int I, int B, int M, int hw) {
    const int p = (int)blockIdx.x * AM_PIX + (int)threadIdx.x, n = (int)blockIdx.y;
    if (p >= hw) return;
    const int b = n / I, i = n - b * I;
    const float *dp = dmasks.g[i];
    float *dst = dlogits + ((long)n * hw + p) * pitch;
    f32x4 out[CV];
#pragma unroll
    for (int q = 0; q < CV; ++q) out[q] = f32x4{0.f, 0.f, 0.f, 0.f};
    if (dp) {
        const float *pm = masks + (((long)i * B + b) * M) * hw + p;
        dp += ((long)b * M) * hw + p;
        float pv[4 * CV], dv[4 * CV];
        double dot = 0;
#pragma unroll
        for (int c = 0; c < 4 * CV; ++c) {
            if (c < M) {
                pv[c] = pm[(long)c * hw];
                dv[c] = dp[(long)c * hw];
                const double t = (double)pv[c] * (double)dv[c];
                dot = c == 0 ? t : dot + t;
            }
        }
#pragma unroll
        for (int c = 0; c < 4 * CV; ++c)
            if (c < M) out[c / 4][c % 4] = (float)((double)pv[c] * ((double)dv[c] - dot));
    }
#pragma unroll
    for (int q = 0; q < CV; ++q) st4(dst + 4 * q, out[q]);
}

// mean and std of the reference's de-normalisation (models/fcn_head.py:160-161), rounded to float as its float32 tensors take them
__device__ __forceinline__ float am_denorm(float v, int c) {
    const float mean = c == 0 ? 123.675f : (c == 1 ? 116.28f : 103.53f);
    const float std = c == 0 ? 58.395f : (c == 1 ? 57.12f : 57.375f);
    return (v * std + mean) / 255.0f;
}

// frames [B][2][3][Hi][Wi] = 6 B planes -> two_frame [B][6][Ho][Wo]: de-normalise the four taps, then the blend of
// resize_nchw_kernel (csrc/spatial.hip) at align_corners = True
__global__ void __launch_bounds__(256) am_frame_pair_kernel(const float *__restrict__ x, float *__restrict__ y, int planes, int Hi, int Wi,
                                                            int Ho, int Wo, float sh, float sw) {
    const long total = (long)planes * Ho * Wo;
    const long step = (long)gridDim.x * blockDim.x;
    for (long i = (long)blockIdx.x * blockDim.x + threadIdx.x; i < total; i += step) {
        const int xo = (int)(i % Wo);
        const long t = i / Wo;
        const int yo = (int)(t % Ho);
        const long pl = t / Ho;
        const int c = (int)(pl % 3);
        int y0, y1, x0, x1;
        float ly, lx;
        src_index(yo, sh, 1, Hi, y0, y1, ly);
        src_index(xo, sw, 1, Wi, x0, x1, lx);
        const float *b = x + pl * Hi * Wi;
        y[i] = blend(1.f - ly, ly, 1.f - lx, lx, am_denorm(b[(long)y0 * Wi + x0], c), am_denorm(b[(long)y0 * Wi + x1], c),
                     am_denorm(b[(long)y1 * Wi + x0], c), am_denorm(b[(long)y1 * Wi + x1], c));
    }
}

inline bool am_softmax_ok(int pitch, int I, int B, int M, int Cp, int hw) {
    if (I < 1 || I > AM_MAXI || B < 1 || B > 65535 || (long)I * B > 65535 || M < 1 || M > AM_MAXM || hw <= 0 || hw >= (1 << 30)) return false;
    if ((Cp != 4 && Cp != 8) || M > Cp || pitch < Cp || pitch % 4) return false;
    return (long)I * B * hw * pitch < (1L << 40);
}

}  // namespace

extern "C" int rcf_amd_geometry(int which) { return which == 0 ? AM_PIX : which == 1 ? AM_MAXM : which == 2 ? AM_MAXI : 0; }

extern "C" int rcf_amd_mask_softmax_fwd_f32(const float *logits, int pitch, float *masks, int I, int B, int M, int Cp, int hw,
                                            void *stream) {
    if (!am_softmax_ok(pitch, I, B, M, Cp, hw)) return RCF_EINVAL;
    if (!logits || !masks || !rcf_aligned16(logits)) return RCF_EINVAL;
    const dim3 grid(rcf_cdiv(hw, AM_PIX), I * B);
    if (Cp == 4)
        hipLaunchKernelGGL(am_softmax_fwd_kernel<1>, grid, dim3(256), 0, rcf_stream(stream), logits, pitch, masks, I, B, M, hw);
    else
        hipLaunchKernelGGL(am_softmax_fwd_kernel<2>, grid, dim3(256), 0, rcf_stream(stream), logits, pitch, masks, I, B, M, hw);
    RCF_LAUNCH_CHECK();
    return 0;
}

extern "C" int rcf_amd_mask_softmax_bwd_f32(const float *masks, const float *const *dmasks, float *dlogits, int pitch, int I, int B, int M,
                                            int Cp, int hw, void *stream) {
    if (!am_softmax_ok(pitch, I, B, M, Cp, hw)) return RCF_EINVAL;
    if (!masks || !dmasks || !dlogits || !rcf_aligned16(dlogits)) return RCF_EINVAL;
    AmFrames fr;
    for (int i = 0; i < AM_MAXI; ++i) fr.g[i] = i < I ? dmasks[i] : nullptr;
    const dim3 grid(rcf_cdiv(hw, AM_PIX), I * B);
    if (Cp == 4)
        hipLaunchKernelGGL(am_softmax_bwd_kernel<1>, grid, dim3(256), 0, rcf_stream(stream), masks, fr, dlogits, pitch, I, B, M, hw);
    else
        hipLaunchKernelGGL(am_softmax_bwd_kernel<2>, grid, dim3(256), 0, rcf_stream(stream), masks, fr, dlogits, pitch, I, B, M, hw);
    RCF_LAUNCH_CHECK();
    return 0;
}

extern "C" int rcf_amd_frame_pair_f32(const float *frames, float *out, int B, int Hi, int Wi, int Ho, int Wo, void *stream) {
    if (B < 1 || B > 65535 || Hi < 1 || Wi < 1 || Ho < 1 || Wo < 1 || Hi > (1 << 14) || Wi > (1 << 14) || Ho > (1 << 14) || Wo > (1 << 14))
        return RCF_EINVAL;
    if (!frames || !out) return RCF_EINVAL;
    const long total = 6L * B * Ho * Wo;
    const long blocks = (total + 255) / 256;
    hipLaunchKernelGGL(am_frame_pair_kernel, dim3((int)(blocks > 8192 ? 8192 : blocks)), dim3(256), 0, rcf_stream(stream), frames, out,
                       6 * B, Hi, Wi, Ho, Wo, host_scale(Hi, Ho, 1), host_scale(Wi, Wo, 1));
    RCF_LAUNCH_CHECK();
    return 0;
}
