// Semantic-constraint refinement (tools/SemanticConstraintsAndMAA/semantic_constraints.py:21-75, 299-336) for a batch of
// frames: the thresholded affinity as a BIT matrix, the whole Adam refinement of the masks on it, and the CRF / NCut-CRF merge.
//
// The affinity a_ij = (G_ij > tau ? 1 : eps) has two values, so a row is n bits + its popcount: with B the bit matrix,
//     u_i = sum_j a_ij x_j = eps X + (1 - eps) sum_{j in row i} x_j   (X = sum_j x_j),    s_i = sum_j a_ij = eps n + (1 - eps) deg_i.
// rcf_affinity_pack_f32 reads the raw Gram matrix once (n^2 floats) and writes n^2 / 8 bytes; the Adam steps then re-read that
// bit matrix (5.2 MB per 6 420-token frame: it stays in L2 / Infinity Cache) instead of n^2 floats each.
// Every reduction is fp64 in an order fixed by (n, launch geometry) alone and nothing is added atomically: a frame's result
// does not depend on the batch it is in or on its position, and is the same bits on every run.
#include "rcf_common.h"

namespace {

// ---- pack ------------------------------------------------------------------------------------------------------------
// One wavefront per row, lane l tests column 64 k + l of chunk k; the 64-bit ballot of chunk k is kept by lane k % 64 and a
// full register (or the tail) goes out as one coalesced store.  Columns >= n give 0 bits: the padding of a row is zero.
__global__ void __launch_bounds__(256) affinity_pack_kernel(const float *__restrict__ gram, long pitch, int n, float tau,
                                                            unsigned long long *__restrict__ bits, int words64,
                                                            int *__restrict__ deg) {
    const int lane = threadIdx.x & 63;
    const int row = blockIdx.x * 4 + (threadIdx.x >> 6);
    if (row >= n) return;
    const long f = blockIdx.y;
    const float *g = gram + (f * n + row) * pitch;
    unsigned long long *out = bits + (f * n + row) * words64;
    unsigned long long mine = 0;
    int count = 0;
    for (int k0 = 0; k0 < words64; k0 += 64) {
        const int kend = min(k0 + 64, words64);
        int k = k0;
        for (; k + 4 <= kend; k += 4) {                                  // four independent loads in flight per lane
            float v[4];
#pragma unroll
            for (int q = 0; q < 4; ++q) {
                const int c = (k + q) * 64 + lane;
                v[q] = c < n ? g[c] : tau;                               // tau > tau is false: a zero bit
            }
#pragma unroll
            for (int q = 0; q < 4; ++q) {
                const unsigned long long b = __ballot(v[q] > tau);
                count += __popcll(b);
                if (lane == ((k + q) & 63)) mine = b;
            }
        }
        for (; k < kend; ++k) {
            const int c = k * 64 + lane;
            const float v = c < n ? g[c] : tau;
            const unsigned long long b = __ballot(v > tau);
            count += __popcll(b);
            if (lane == (k & 63)) mine = b;
        }
        if (k0 + lane < kend) out[k0 + lane] = mine;
    }
    if (lane == 0) deg[f * n + row] = count;
}

// ---- refine ----------------------------------------------------------------------------------------------------------
constexpr int RS_ROWS = 4;                     // rows per wavefront of rowsum_kernel
constexpr int RS_BLOCK_ROWS = 4 * RS_ROWS;     // rows per workgroup

// r[f][i] = sum_{j in row i} x[f][j] in fp64.  The frame's x sits in LDS (zero-filled up to a whole chunk); a wavefront takes
// RS_ROWS rows: per 64-column chunk one LDS read of x and, per row, one wave-uniform 64-bit word of the bit matrix (a scalar
// load).  Lane l adds x[64 k + l] where bit l is set; the 64 lane sums are added by a butterfly.
__global__ void __launch_bounds__(256) ncut_rowsum_kernel(const unsigned long long *__restrict__ bits, int words64, int n,
                                                          const float *__restrict__ x, double *__restrict__ r) {
    extern __shared__ float xs[];
    const long f = blockIdx.y;
    const float *xf = x + f * n;
    for (int i = threadIdx.x; i < words64 * 64; i += 256) xs[i] = i < n ? xf[i] : 0.f;
    __syncthreads();
    const int lane = threadIdx.x & 63;
    const int wv = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
    const int row0 = blockIdx.x * RS_BLOCK_ROWS + wv * RS_ROWS;
    if (row0 >= n) return;
    const unsigned long long *rowp[RS_ROWS];
#pragma unroll
    for (int q = 0; q < RS_ROWS; ++q) rowp[q] = bits + (f * n + min(row0 + q, n - 1)) * words64;
    double acc[RS_ROWS] = {};
#pragma unroll 2
    for (int k = 0; k < words64; ++k) {
        const double xv = (double)xs[k * 64 + lane];
#pragma unroll
        for (int q = 0; q < RS_ROWS; ++q) acc[q] += ((rowp[q][k] >> lane) & 1ull) ? xv : 0.0;
    }
#pragma unroll
    for (int q = 0; q < RS_ROWS; ++q) {
        const double s = wave_sum_d(acc[q]);
        if (lane == 0 && row0 + q < n) r[f * n + row0 + q] = s;
    }
}

constexpr int STEP_THREADS = 1024;

// the sums of up to 3 per-thread values over the workgroup, in a fixed order (butterfly per wavefront, then wavefront 0..15)
template <int K>
__device__ __forceinline__ void block_sum(double (&v)[K], double (*red)[STEP_THREADS / 64]) {
    const int lane = threadIdx.x & 63, wv = threadIdx.x >> 6;
    __syncthreads();                                                      // `red` may still be read from the previous call
#pragma unroll
    for (int k = 0; k < K; ++k) {
        v[k] = wave_sum_d(v[k]);
        if (lane == 0) red[k][wv] = v[k];
    }
    __syncthreads();
#pragma unroll
    for (int k = 0; k < K; ++k) {
        double t = 0;
        for (int w = 0; w < STEP_THREADS / 64; ++w) t += red[k][w];
        v[k] = t;
    }
}

struct adam_consts { float lr, b1, b2, eps, wd, bc1, bc2_sqrt; };

// One workgroup per frame: value, gradient (the closed form of rcf_ncut_value_grad_f32), Adam with coupled weight decay (the
// arithmetic of rcf_adam_step_f32) and the clamp to [0, 1].  first != 0: the moments start at zero and are not read.
__global__ void __launch_bounds__(STEP_THREADS) ncut_step_kernel(const double *__restrict__ r, const int *__restrict__ deg, int n,
                                                                 double eps, float *__restrict__ x, float *__restrict__ m,
                                                                 float *__restrict__ v, adam_consts c, int first,
                                                                 double *__restrict__ value_out, int value_stride) {
    __shared__ double red[3][STEP_THREADS / 64];
    const long f = blockIdx.x;
    r += f * n; deg += f * n; x += f * n; m += f * n; v += f * n;
    const double one_eps = 1.0 - eps, eps_n = eps * (double)n;
    double t1[2] = {0, 0};                                                // X = sum x, S = sum s
    for (int i = threadIdx.x; i < n; i += STEP_THREADS) {
        t1[0] += (double)x[i];
        t1[1] += eps_n + one_eps * (double)deg[i];
    }
    block_sum<2>(t1, red);
    const double eX = eps * t1[0], S = t1[1];
    double t2[2] = {0, 0};                                                // s.x, x.u
    for (int i = threadIdx.x; i < n; i += STEP_THREADS) {
        const double xi = (double)x[i], si = eps_n + one_eps * (double)deg[i], ui = eX + one_eps * r[i];
        t2[0] += si * xi;
        t2[1] += xi * ui;
    }
    block_sum<2>(t2, red);
    const double a = t2[0], cut = t2[0] - t2[1], b = S - t2[0];
    if (threadIdx.x == 0 && value_out) value_out[f * value_stride] = cut / a + cut / b;
    const double c1 = 1.0 / a + 1.0 / b, c2 = cut / (a * a), c3 = cut / (b * b);
    const float step_size = c.lr / c.bc1;
    for (int i = threadIdx.x; i < n; i += STEP_THREADS) {
        const double si = eps_n + one_eps * (double)deg[i], ui = eX + one_eps * r[i];
        float grad = (float)((si - 2.0 * ui) * c1 - c2 * si + c3 * si);
        const float w = x[i], m0 = first ? 0.f : m[i], v0 = first ? 0.f : v[i];
        grad = grad + c.wd * w;
        const float mi = m0 + (1.f - c.b1) * (grad - m0);
        const float vi = c.b2 * v0 + (1.f - c.b2) * grad * grad;
        m[i] = mi;
        v[i] = vi;
        const float denom = sqrtf(vi) / c.bc2_sqrt + c.eps;
        x[i] = fminf(fmaxf(w - step_size * (mi / denom), 0.f), 1.f);
    }
}

// ---- merge -----------------------------------------------------------------------------------------------------------
constexpr int MERGE_BLOCKS = 64;               // workgroups per frame

// counts[f] += |{(a > 0.5) xor (b > 0.5)}|: the union minus the intersection of the two binarised masks (integer atomics)
__global__ void __launch_bounds__(256) mask_umi_kernel(const float *__restrict__ a, const float *__restrict__ b, long npix,
                                                       unsigned long long *__restrict__ counts) {
    __shared__ unsigned red[4];
    const long f = blockIdx.y;
    a += f * npix; b += f * npix;
    unsigned c = 0;
    for (long i = (long)blockIdx.x * 256 + threadIdx.x; i < npix; i += (long)gridDim.x * 256) c += (a[i] > 0.5f) != (b[i] > 0.5f);
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) c += __shfl_xor(c, o, 64);
    if ((threadIdx.x & 63) == 0) red[threadIdx.x >> 6] = c;
    __syncthreads();
    if (threadIdx.x == 0) {
        const unsigned t = (red[0] + red[1]) + (red[2] + red[3]);
        if (t) atomicAdd(counts + f, (unsigned long long)t);
    }
}

// out = trunc((a b) 255), or trunc(a 255) for a frame whose count is above umi_th (umi_th < 0: never); fp32 products, each rounded
__global__ void __launch_bounds__(256) mask_merge_kernel(const float *__restrict__ a, const float *__restrict__ b, long npix,
                                                         const long long *__restrict__ counts, long long umi_th,
                                                         uint8_t *__restrict__ out) {
    const long f = blockIdx.y;
    a += f * npix; b += f * npix; out += f * npix;
    const bool single = umi_th >= 0 && counts[f] > umi_th;
    for (long i = (long)blockIdx.x * 256 + threadIdx.x; i < npix; i += (long)gridDim.x * 256) {
        const float p = single ? a[i] : a[i] * b[i];
        out[i] = (uint8_t)(int)(p * 255.0f);
    }
}

}  // namespace

extern "C" int rcf_affinity_pack_words(int n) { return n > 0 ? 2 * ((n + 63) / 64) : 0; }

extern "C" int rcf_affinity_pack_f32(const float *gram, long pitch, int n, int frames, float tau, uint32_t *bits, int32_t *deg,
                                     void *stream) {
    if (!gram || !bits || !deg || n <= 0 || frames <= 0 || frames > 65535 || pitch < n || (((uintptr_t)bits) & 7)) return RCF_EINVAL;
    hipLaunchKernelGGL(affinity_pack_kernel, dim3(rcf_cdiv(n, 4), frames), dim3(256), 0, rcf_stream(stream), gram, pitch, n, tau,
                       (unsigned long long *)bits, (n + 63) / 64, deg);
    RCF_LAUNCH_CHECK();
    return 0;
}

extern "C" size_t rcf_ncut_refine_packed_workspace_bytes(int frames, int n) {
    if (frames <= 0 || n <= 0 || n > RCF_NCUT_PACKED_MAX_N) return 0;
    return (size_t)frames * n * (sizeof(double) + 2 * sizeof(float));     // row sums | exp_avg | exp_avg_sq
}

extern "C" int rcf_ncut_refine_packed_f32(const uint32_t *bits, const int32_t *deg, int n, int frames, float eps, float *x,
                                          int steps, float lr, float weight_decay, double *values, void *workspace,
                                          size_t workspace_bytes, void *stream) {
    if (!bits || !deg || !x || !workspace || n <= 0 || n > RCF_NCUT_PACKED_MAX_N || frames <= 0 || frames > 65535 || steps < 0 ||
        (((uintptr_t)bits) & 7) || (((uintptr_t)workspace) & 7))
        return RCF_EINVAL;
    if (workspace_bytes < rcf_ncut_refine_packed_workspace_bytes(frames, n)) return RCF_EWORKSPACE;
    hipStream_t st = rcf_stream(stream);
    const long fn = (long)frames * n;
    double *r = (double *)workspace;
    float *m = (float *)(r + fn), *v = m + fn;
    const int words64 = (n + 63) / 64;
    const float beta1 = 0.9f, beta2 = 0.999f;
    for (int i = 0; i < steps; ++i) {
        hipLaunchKernelGGL(ncut_rowsum_kernel, dim3(rcf_cdiv(n, RS_BLOCK_ROWS), frames), dim3(256), (size_t)words64 * 64 * sizeof(float),
                           st, (const unsigned long long *)bits, words64, n, (const float *)x, r);
        // the bias corrections of rcf_adam_step_f32
        const double bc1 = 1.0 - pow((double)beta1, (double)(i + 1)), bc2 = 1.0 - pow((double)beta2, (double)(i + 1));
        const adam_consts c = {lr, beta1, beta2, 1e-8f, weight_decay, (float)bc1, (float)sqrt(bc2)};
        hipLaunchKernelGGL(ncut_step_kernel, dim3(frames), dim3(STEP_THREADS), 0, st, (const double *)r, deg, n, (double)eps, x, m, v,
                           c, i == 0, values ? values + i : nullptr, steps);
    }
    RCF_LAUNCH_CHECK();
    return 0;
}

extern "C" int rcf_mask_merge_u8(const float *a, const float *b, int frames, long npix, long long umi_th, uint8_t *out,
                                 long long *counts, void *stream) {
    if (!a || !b || !out || !counts || frames <= 0 || frames > 65535 || npix <= 0) return RCF_EINVAL;
    hipStream_t st = rcf_stream(stream);
    if (hipMemsetAsync(counts, 0, (size_t)frames * sizeof(long long), st) != hipSuccess) return (int)hipGetLastError();
    const int blocks = (int)(npix < (long)MERGE_BLOCKS * 256 ? rcf_cdiv(npix, 256) : MERGE_BLOCKS);
    hipLaunchKernelGGL(mask_umi_kernel, dim3(blocks, frames), dim3(256), 0, st, a, b, npix, (unsigned long long *)counts);
    hipLaunchKernelGGL(mask_merge_kernel, dim3(blocks, frames), dim3(256), 0, st, a, b, npix, (const long long *)counts, umi_th, out);
    RCF_LAUNCH_CHECK();
    return 0;
}
