// PWC-Lite's glue between the native convs, the cost volume and the warp (models/amd/pwc_lite.py): segment pooling and segment flow
// composition with their gradients, LeakyReLU backward on pitched NHWC, and the estimator's input pack.  All fp32 tensors.
//
// Segment pooling (pwc_lite.py:85-96, get_averge_feat, for all M masks at once): pooled[b][m][c] = sum_p feat mask / sum_p mask
// with feat an NHWC channel slice and mask planar.  A workgroup owns PW_CHUNK pixels of one image: its products and sums are taken in
// fp64 (a product of two floats is exact there) and go to a partials buffer, one finishing launch adds the chunks in index order
// and divides.  The composition's dgroup = sum_p mask dflow goes the same way.  Nothing here uses atomics: every value is a gather
// summed in a fixed order, the same bits on every call.
//
// Error against exact arithmetic on the same inputs, per element, is k 2^-24 mass (mass: the sum of the absolute terms); k is the
// number of roundings on the longest path plus 2:
//   pooled, msum, dgroup      k = 3       fp64 sums (their rounding is 2^-29 of fp32's), one rounding to float
//   pool dmask                k = 3       (sum_c feat dpooled - sum_c pooled dpooled) / msum in fp64, one rounding to float
//   pool dfeat                k = M + 4   dpooled / msum, times mask, M - 1 additions, the addition onto dfeat (beta)
//   flow                      k = M + 2   a product and M - 1 additions
//   compose dmask             k = 5       two products, their sum, the addition onto dmask (beta)
//   leaky backward            k = 3       one product
// A zero mask sum divides by zero as the reference does: there is no guard.
#include "flow_sample.h"

namespace {

constexpr int PW_CHUNK = 1024;     // pixels of one image per workgroup in the pooled sums
constexpr int PW_MAXM = 8;         // masks (segments) per image
constexpr int PW_MAXC = 256;       // channels of the pooled slice
constexpr int PW_TILE = 64;        // pixels per workgroup of the pack / unpack transposes
constexpr int PW_MAXPACK = 128;    // channels one pack writes

// ------------------------------------------------------------------------------------------------------------ segment pooling
// P[b][chunk][m][c] = sum over the chunk's pixels of feat mask, S[b][chunk][m] = sum of mask.  Thread t: channel vector t % CV of the
// pixels lane, lane + L, ... (L = 256 / CV lanes); the lanes are added in lane order.
__global__ void __launch_bounds__(256) pw_pool_fwd_kernel(const float *__restrict__ feat, int pitch, const float *__restrict__ mask,
                                                          double *__restrict__ P, double *__restrict__ S, int M, int C, int hw,
                                                          int nchunks) {
    __shared__ double sh[1024];
    __shared__ double shs[256];
    const int chunk = (int)blockIdx.x, b = (int)blockIdx.y, tid = (int)threadIdx.x;
    const int CV = C / 4, L = 256 / CV;
    const int cv = tid % CV, lane = tid / CV;
    const bool active = lane < L;
    const int p0 = chunk * PW_CHUNK, p1 = min(p0 + PW_CHUNK, hw);
    double acc[PW_MAXM][4], ms[PW_MAXM];
#pragma unroll
    for (int m = 0; m < PW_MAXM; ++m) {
        ms[m] = 0;
#pragma unroll
        for (int e = 0; e < 4; ++e) acc[m][e] = 0;
    }
    if (active) {
        for (int p = p0 + lane; p < p1; p += L) {
            const f32x4 f = ld4(feat + ((long)b * hw + p) * pitch + cv * 4);
#pragma unroll
            for (int m = 0; m < PW_MAXM; ++m) {
                if (m < M) {
                    const double mk = (double)mask[((long)b * M + m) * hw + p];
#pragma unroll
                    for (int e = 0; e < 4; ++e) acc[m][e] += (double)f[e] * mk;
                    if (cv == 0) ms[m] += mk;
                }
            }
        }
    }
    const long row = (long)b * nchunks + chunk;
#pragma unroll
    for (int m = 0; m < PW_MAXM; ++m) {
        if (m < M) {
            if (active) {
#pragma unroll
                for (int e = 0; e < 4; ++e) sh[lane * C + cv * 4 + e] = acc[m][e];
                if (cv == 0) shs[lane] = ms[m];
            }
            __syncthreads();
            if (tid < C) {
                double s = 0;
                for (int l = 0; l < L; ++l) s += sh[l * C + tid];
                P[(row * M + m) * C + tid] = s;
            }
            if (tid == 0) {
                double s = 0;
                for (int l = 0; l < L; ++l) s += shs[l];
                S[row * M + m] = s;
            }
            __syncthreads();
        }
    }
}

__global__ void __launch_bounds__(256) pw_pool_finish_kernel(const double *__restrict__ P, const double *__restrict__ S,
                                                             float *__restrict__ pooled, float *__restrict__ msum, int B, int M, int C,
                                                             int nchunks) {
    const int i = (int)blockIdx.x * 256 + (int)threadIdx.x;
    if (i >= B * M * C) return;
    const int c = i % C, bm = i / C, m = bm % M, b = bm / M;
    double s = 0, t = 0;
    for (int k = 0; k < nchunks; ++k) {
        const long row = (long)b * nchunks + k;
        s += P[(row * M + m) * C + c];
        t += S[row * M + m];
    }
    pooled[i] = (float)(s / t);
    if (c == 0) msum[bm] = (float)t;
}

// dfeat[b][p][c] (+)= sum_m mask dpooled / msum;  dmask[b][m][p] = (sum_c feat dpooled - sum_c pooled dpooled) / msum.  One thread
// per pixel walks its channels; dpooled, dpooled / msum and the second sum sit in LDS.
__global__ void __launch_bounds__(256) pw_pool_bwd_kernel(const float *__restrict__ feat, int pitch, const float *__restrict__ mask,
                                                          const float *__restrict__ pooled, const float *__restrict__ msum,
                                                          const float *__restrict__ dpooled, float *__restrict__ dfeat, int dpitch,
                                                          int beta, float *__restrict__ dmask, int M, int C, int hw) {
    __shared__ float DP[PW_MAXM * PW_MAXC], Q[PW_MAXM * PW_MAXC];
    __shared__ double DOT[PW_MAXM];
    const int b = (int)blockIdx.y, tid = (int)threadIdx.x;
    for (int i = tid; i < M * C; i += 256) {
        const float d = dpooled[(long)b * M * C + i];
        DP[i] = d;
        Q[i] = d / msum[b * M + i / C];
    }
    __syncthreads();
    if (tid < M) {
        double d = 0;
        for (int c = 0; c < C; ++c) d += (double)pooled[((long)b * M + tid) * C + c] * (double)DP[tid * C + c];
        DOT[tid] = d;
    }
    __syncthreads();
    const int p = (int)blockIdx.x * 256 + tid;
    if (p >= hw) return;
    float mk[PW_MAXM];
    double dm[PW_MAXM];
#pragma unroll
    for (int m = 0; m < PW_MAXM; ++m) {
        mk[m] = m < M ? mask[((long)b * M + m) * hw + p] : 0.f;
        dm[m] = 0;
    }
    const float *src = feat + ((long)b * hw + p) * pitch;
    float *dst = dfeat + ((long)b * hw + p) * dpitch;
    for (int c = 0; c < C; c += 4) {
        const f32x4 f = ld4(src + c);
        f32x4 g = {0.f, 0.f, 0.f, 0.f};
#pragma unroll
        for (int m = 0; m < PW_MAXM; ++m) {
            if (m < M) {
#pragma unroll
                for (int e = 0; e < 4; ++e) {
                    const float t = mk[m] * Q[m * C + c + e];
                    g[e] = m == 0 ? t : g[e] + t;
                    dm[m] += (double)f[e] * (double)DP[m * C + c + e];
                }
            }
        }
        if (beta) g = ld4(dst + c) + g;
        st4(dst + c, g);
    }
#pragma unroll
    for (int m = 0; m < PW_MAXM; ++m)
        if (m < M) dmask[((long)b * M + m) * hw + p] = (float)((dm[m] - DOT[m]) / (double)msum[b * M + m]);
}

// ------------------------------------------------------------------------------------------------------ segment flow composition
// flow[b][c][p] = sum_m mask[b][m][p] group[b][m][c], m upwards
__global__ void __launch_bounds__(256) pw_flow_fwd_kernel(const float *__restrict__ mask, const float *__restrict__ group,
                                                          float *__restrict__ flow, int B, int M, int hw) {
    const long total = (long)B * hw, step = (long)gridDim.x * 256;
    for (long i = (long)blockIdx.x * 256 + threadIdx.x; i < total; i += step) {
        const long b = i / hw, p = i - b * hw;
        float f0 = 0.f, f1 = 0.f;
        for (int m = 0; m < M; ++m) {
            const float mk = mask[(b * M + m) * hw + p];
            const float t0 = mk * group[(b * M + m) * 2], t1 = mk * group[(b * M + m) * 2 + 1];
            f0 = m == 0 ? t0 : f0 + t0;
            f1 = m == 0 ? t1 : f1 + t1;
        }
        flow[(b * 2) * hw + p] = f0;
        flow[(b * 2 + 1) * hw + p] = f1;
    }
}

// dmask[b][m][p] (+)= dflow[b][0][p] group[b][m][0] + dflow[b][1][p] group[b][m][1];  G[b][chunk][m][c] = the chunk's sum of
// mask dflow (fp64)
__global__ void __launch_bounds__(256) pw_flow_bwd_kernel(const float *__restrict__ mask, const float *__restrict__ group,
                                                          const float *__restrict__ dflow, float *__restrict__ dmask, int beta,
                                                          double *__restrict__ G, int M, int hw, int nchunks) {
    __shared__ double red[4 * 2 * PW_MAXM];
    const int chunk = (int)blockIdx.x, b = (int)blockIdx.y;
    const int p0 = chunk * PW_CHUNK, p1 = min(p0 + PW_CHUNK, hw);
    double acc[2 * PW_MAXM];
#pragma unroll
    for (int k = 0; k < 2 * PW_MAXM; ++k) acc[k] = 0;
    for (int p = p0 + (int)threadIdx.x; p < p1; p += 256) {
        const float d0 = dflow[((long)b * 2) * hw + p], d1 = dflow[((long)b * 2 + 1) * hw + p];
#pragma unroll
        for (int m = 0; m < PW_MAXM; ++m) {
            if (m < M) {
                const long at = ((long)b * M + m) * hw + p;
                const float mk = mask[at];
                acc[2 * m] += (double)mk * (double)d0;
                acc[2 * m + 1] += (double)mk * (double)d1;
                if (dmask) {
                    const float g = d0 * group[(b * M + m) * 2] + d1 * group[(b * M + m) * 2 + 1];
                    dmask[at] = beta ? dmask[at] + g : g;
                }
            }
        }
    }
    block_sum_d<2 * PW_MAXM>(acc, red);
    if (threadIdx.x == 0) {
#pragma unroll
        for (int k = 0; k < 2 * PW_MAXM; ++k)
            if (k < 2 * M) G[((long)b * nchunks + chunk) * 2 * M + k] = acc[k];
    }
}

__global__ void __launch_bounds__(256) pw_flow_finish_kernel(const double *__restrict__ G, float *__restrict__ dgroup, int B, int M,
                                                             int nchunks) {
    const int i = (int)blockIdx.x * 256 + (int)threadIdx.x;
    if (i >= B * M * 2) return;
    const int k = i % (2 * M), b = i / (2 * M);
    double s = 0;
    for (int c = 0; c < nchunks; ++c) s += G[((long)b * nchunks + c) * 2 * M + k];
    dgroup[i] = (float)s;
}

// ------------------------------------------------------------------------------------------------------------- LeakyReLU backward
// g = dy (y > 0 ? 1 : slope) on rows of C channels, each tensor with its own pitch; y = +-0 takes the slope, as torch does
__global__ void __launch_bounds__(256) pw_leaky_bwd_kernel(const float *__restrict__ dy, long dy_pitch, const float *__restrict__ y,
                                                           long y_pitch, float *__restrict__ g, long g_pitch, long rows, int C,
                                                           float slope) {
    const int CV = C / 4;
    const long total = rows * CV, step = (long)gridDim.x * 256;
    for (long i = (long)blockIdx.x * 256 + threadIdx.x; i < total; i += step) {
        const long r = i / CV;
        const int c = (int)(i - r * CV) * 4;
        const f32x4 d = ld4(dy + r * dy_pitch + c), v = ld4(y + r * y_pitch + c);
        f32x4 o;
#pragma unroll
        for (int e = 0; e < 4; ++e) o[e] = v[e] > 0.f ? d[e] : d[e] * slope;
        st4(g + r * g_pitch + c, o);
    }
}

// --------------------------------------------------------------------------------------------------- estimator input pack / unpack
// buf[b][p][c0 + k] = corr[b][k][p] (k < D), flow[b][k - D][p] (k < D + 2), 0 up to the next multiple of 4: nch channels in all.  A
// workgroup moves PW_TILE pixels through LDS, so that both sides are accessed along their contiguous axis.
__global__ void __launch_bounds__(256) pw_pack_kernel(const float *__restrict__ corr, const float *__restrict__ flow,
                                                      float *__restrict__ buf, int pitch, int c0, int D, int nch, int hw) {
    __shared__ float T[PW_MAXPACK * (PW_TILE + 1)];
    const int b = (int)blockIdx.y, p0 = (int)blockIdx.x * PW_TILE;
    const int np = min(PW_TILE, hw - p0);
    for (int i = (int)threadIdx.x; i < nch * PW_TILE; i += 256) {
        const int k = i / PW_TILE, pl = i - k * PW_TILE;
        float v = 0.f;
        if (pl < np) {
            if (k < D) v = corr[((long)b * D + k) * hw + p0 + pl];
            else if (k < D + 2) v = flow[((long)b * 2 + (k - D)) * hw + p0 + pl];
        }
        T[k * (PW_TILE + 1) + pl] = v;
    }
    __syncthreads();
    for (int i = (int)threadIdx.x; i < np * nch; i += 256) {
        const int pl = i / nch, k = i - pl * nch;
        buf[((long)b * hw + p0 + pl) * pitch + c0 + k] = T[k * (PW_TILE + 1) + pl];
    }
}

// the adjoint: dcorr[b][k][p] = dbuf[b][p][c0 + k], dflow[b][c][p] = dbuf[b][p][c0 + D + c]
__global__ void __launch_bounds__(256) pw_unpack_kernel(const float *__restrict__ dbuf, int pitch, int c0, float *__restrict__ dcorr,
                                                        float *__restrict__ dflow, int D, int hw) {
    __shared__ float T[PW_MAXPACK * (PW_TILE + 1)];
    const int b = (int)blockIdx.y, p0 = (int)blockIdx.x * PW_TILE;
    const int np = min(PW_TILE, hw - p0), nch = D + 2;
    for (int i = (int)threadIdx.x; i < np * nch; i += 256) {
        const int pl = i / nch, k = i - pl * nch;
        T[k * (PW_TILE + 1) + pl] = dbuf[((long)b * hw + p0 + pl) * pitch + c0 + k];
    }
    __syncthreads();
    for (int i = (int)threadIdx.x; i < nch * PW_TILE; i += 256) {
        const int k = i / PW_TILE, pl = i - k * PW_TILE;
        if (pl >= np) continue;
        const float v = T[k * (PW_TILE + 1) + pl];
        if (k < D) dcorr[((long)b * D + k) * hw + p0 + pl] = v;
        else dflow[((long)b * 2 + (k - D)) * hw + p0 + pl] = v;
    }
}

// ---------------------------------------------------------------------------------------------------------------- host side
inline bool pw_seg_ok(int B, int M, int hw) {
    if (B <= 0 || B > 65535 || M < 1 || M > PW_MAXM || hw <= 0 || hw >= (1 << 30)) return false;
    return (long)B * M * hw < (1L << 40);
}
inline bool pw_slice_ok(int C, int pitch) { return C >= 4 && C <= PW_MAXC && C % 4 == 0 && pitch >= C && pitch % 4 == 0; }
inline int pw_chunks(int hw) { return rcf_cdiv(hw, PW_CHUNK); }
inline int pw_blocks(long total) {
    const long b = (total + 255) / 256;
    return (int)(b < 1 ? 1 : (b > 4096 ? 4096 : b));
}

}  // namespace

extern "C" int rcf_pwc_geometry(int which) {
    return which == 0 ? PW_CHUNK : which == 1 ? PW_MAXM : which == 2 ? PW_MAXC : which == 3 ? PW_TILE : which == 4 ? PW_MAXPACK : 0;
}

extern "C" long rcf_pwc_pool_partials(int B, int M, int C, int hw) {
    if (!pw_seg_ok(B, M, hw) || !pw_slice_ok(C, C)) return 0;
    return (long)B * pw_chunks(hw) * M * (C + 1);
}

extern "C" long rcf_pwc_flow_partials(int B, int M, int hw) {
    if (!pw_seg_ok(B, M, hw)) return 0;
    return (long)B * pw_chunks(hw) * M * 2;
}

extern "C" int rcf_pwc_segment_pool_fwd_f32(const float *feat, int feat_pitch, const float *mask, float *pooled, float *msum,
                                            double *partials, long partials_len, int B, int M, int C, int hw, void *stream) {
    if (!pw_seg_ok(B, M, hw) || !pw_slice_ok(C, feat_pitch)) return RCF_EINVAL;
    if (!feat || !mask || !pooled || !msum || !partials || !rcf_aligned16(feat)) return RCF_EINVAL;
    if (partials_len < rcf_pwc_pool_partials(B, M, C, hw)) return RCF_EWORKSPACE;
    const int nc = pw_chunks(hw);
    double *P = partials, *S = partials + (long)B * nc * M * C;
    hipStream_t st = rcf_stream(stream);
    hipLaunchKernelGGL(pw_pool_fwd_kernel, dim3(nc, B), dim3(256), 0, st, feat, feat_pitch, mask, P, S, M, C, hw, nc);
    RCF_LAUNCH_CHECK();
    hipLaunchKernelGGL(pw_pool_finish_kernel, dim3(rcf_cdiv((long)B * M * C, 256)), dim3(256), 0, st, (const double *)P, (const double *)S,
                       pooled, msum, B, M, C, nc);
    RCF_LAUNCH_CHECK();
    return 0;
}

extern "C" int rcf_pwc_segment_pool_bwd_f32(const float *feat, int feat_pitch, const float *mask, const float *pooled, const float *msum,
                                            const float *dpooled, float *dfeat, int dfeat_pitch, int beta, float *dmask, int B, int M,
                                            int C, int hw, void *stream) {
    if (!pw_seg_ok(B, M, hw) || !pw_slice_ok(C, feat_pitch) || !pw_slice_ok(C, dfeat_pitch) || (beta != 0 && beta != 1)) return RCF_EINVAL;
    if (!feat || !mask || !pooled || !msum || !dpooled || !dfeat || !dmask || !rcf_aligned16(feat) || !rcf_aligned16(dfeat)) return RCF_EINVAL;
    hipLaunchKernelGGL(pw_pool_bwd_kernel, dim3(rcf_cdiv(hw, 256), B), dim3(256), 0, rcf_stream(stream), feat, feat_pitch, mask, pooled,
                       msum, dpooled, dfeat, dfeat_pitch, beta, dmask, M, C, hw);
    RCF_LAUNCH_CHECK();
    return 0;
}

extern "C" int rcf_pwc_segment_flow_fwd_f32(const float *mask, const float *group, float *flow, int B, int M, int hw, void *stream) {
    if (!pw_seg_ok(B, M, hw)) return RCF_EINVAL;
    if (!mask || !group || !flow) return RCF_EINVAL;
    hipLaunchKernelGGL(pw_flow_fwd_kernel, dim3(pw_blocks((long)B * hw)), dim3(256), 0, rcf_stream(stream), mask, group, flow, B, M, hw);
    RCF_LAUNCH_CHECK();
    return 0;
}

// dmask may be NULL (a constant mask); dgroup is always made
extern "C" int rcf_pwc_segment_flow_bwd_f32(const float *mask, const float *group, const float *dflow, float *dmask, int beta,
                                            float *dgroup, double *partials, long partials_len, int B, int M, int hw, void *stream) {
    if (!pw_seg_ok(B, M, hw) || (beta != 0 && beta != 1)) return RCF_EINVAL;
    if (!mask || !group || !dflow || !dgroup || !partials) return RCF_EINVAL;
    if (partials_len < rcf_pwc_flow_partials(B, M, hw)) return RCF_EWORKSPACE;
    const int nc = pw_chunks(hw);
    hipStream_t st = rcf_stream(stream);
    hipLaunchKernelGGL(pw_flow_bwd_kernel, dim3(nc, B), dim3(256), 0, st, mask, group, dflow, dmask, beta, partials, M, hw, nc);
    RCF_LAUNCH_CHECK();
    hipLaunchKernelGGL(pw_flow_finish_kernel, dim3(rcf_cdiv((long)B * M * 2, 256)), dim3(256), 0, st, (const double *)partials, dgroup, B, M,
                       nc);
    RCF_LAUNCH_CHECK();
    return 0;
}

extern "C" int rcf_pwc_leaky_bwd_f32(const float *dy, long dy_pitch, const float *y, long y_pitch, float *g, long g_pitch, long rows,
                                     int C, float slope, void *stream) {
    if (rows <= 0 || rows >= (1L << 40) || C < 4 || C % 4 || dy_pitch < C || y_pitch < C || g_pitch < C || dy_pitch % 4 || y_pitch % 4 ||
        g_pitch % 4)
        return RCF_EINVAL;
    if (!dy || !y || !g || !rcf_aligned16(dy) || !rcf_aligned16(y) || !rcf_aligned16(g)) return RCF_EINVAL;
    hipLaunchKernelGGL(pw_leaky_bwd_kernel, dim3(pw_blocks(rows * (C / 4))), dim3(256), 0, rcf_stream(stream), dy, dy_pitch, y, y_pitch, g,
                       g_pitch, rows, C, slope);
    RCF_LAUNCH_CHECK();
    return 0;
}

static inline bool pw_pack_ok(int pitch, int c0, int D, int B, int hw) {
    if (B <= 0 || B > 65535 || hw <= 0 || hw >= (1 << 30) || D < 1 || c0 < 0 || c0 % 4 || pitch % 4) return false;
    const long end = ((long)c0 + D + 2 + 3) / 4 * 4;
    return end - c0 <= PW_MAXPACK && end <= pitch;
}

extern "C" int rcf_pwc_pack_f32(const float *corr, const float *flow, float *buf, int buf_pitch, int c0, int D, int B, int hw,
                                void *stream) {
    if (!pw_pack_ok(buf_pitch, c0, D, B, hw)) return RCF_EINVAL;
    if (!corr || !flow || !buf) return RCF_EINVAL;
    const int nch = (c0 + D + 2 + 3) / 4 * 4 - c0;
    hipLaunchKernelGGL(pw_pack_kernel, dim3(rcf_cdiv(hw, PW_TILE), B), dim3(256), 0, rcf_stream(stream), corr, flow, buf, buf_pitch, c0, D,
                       nch, hw);
    RCF_LAUNCH_CHECK();
    return 0;
}

extern "C" int rcf_pwc_unpack_f32(const float *dbuf, int buf_pitch, int c0, float *dcorr, float *dflow, int D, int B, int hw,
                                  void *stream) {
    if (!pw_pack_ok(buf_pitch, c0, D, B, hw)) return RCF_EINVAL;
    if (!dbuf || !dcorr || !dflow) return RCF_EINVAL;
    hipLaunchKernelGGL(pw_unpack_kernel, dim3(rcf_cdiv(hw, PW_TILE), B), dim3(256), 0, rcf_stream(stream), dbuf, buf_pitch, c0, dcorr, dflow,
                       D, hw);
    RCF_LAUNCH_CHECK();
    return 0;
}
