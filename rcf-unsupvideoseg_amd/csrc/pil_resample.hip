// Pillow's 8-bit separable resampler on the device (src/libImaging/Resample.c: ImagingResampleHorizontal_8bpc and
// ImagingResampleVertical_8bpc), as tools/STv2-FBMS59-evaluation/eval_tool.py of the reference uses it through Image.resize:
// a horizontal pass and then a vertical pass over u8 planes, each an integer dot product with a row of a 22-bit fixed-point
// coefficient table that starts from 1 << 21, is shifted right by 22 and clipped to 0...255; the horizontal result is a u8
// before the vertical pass reads it.  The tables (rcf_amd.pilresize.coeff_tables) carry the filter: the kernel knows none by
// name and does no float arithmetic.  Optionally the resized planes are compared with a mask and reduced to per-frame
// (intersection, union) counts -- eval_tool.py's iou() -- without being written.
//
// One launch, one block per output tile of 64 columns x tile_h rows and frame.  The block forms the horizontal results of the
// source rows its output rows read in LDS (u8, 64 B per row, LDS_ROWS rows = 16 KB) and runs the vertical pass from there.  The
// host picks tile_h from the reduction factor so that a tile's source rows normally fit the window in one go; the block itself
// walks its rows in runs that DO fit (a single row always does: ksy <= LDS_ROWS is checked before the launch), so any table
// whose taps lie inside the frame is resampled correctly whatever the host guessed.  Tap ranges are clamped into the frame: a
// malformed table gives a wrong picture, never an access outside src or the window.
// Counts: wave shuffles, then one integer atomic per block, frame and count -- independent of the order of the blocks.
#include "rcf_common.h"

namespace {

constexpr int TILE_W = 64;                      // output columns per block: one per lane
constexpr int MAX_TILE_H = 32;                  // output rows per block: 32, 16, ..., 1 (rcf_pil_resample_tile_rows)
constexpr int LDS_ROWS = RCF_PIL_MAX_TAPS;      // horizontally resampled source rows held per block
constexpr int PRECISION_BITS = 32 - 8 - 2;      // Resample.c
constexpr int WAVES = 4;

// Pillow accumulates in int; unsigned arithmetic gives the same bits and stays defined for any table
__device__ __forceinline__ int clip8(unsigned acc) {
    const int v = (int)acc >> PRECISION_BITS;
    return v < 0 ? 0 : v > 255 ? 255 : v;
}

// taps of output row / column i of one axis, clamped into [0, in_size); no table: the pass is skipped (tap i, weight one)
__device__ __forceinline__ void taps_of(const int32_t *__restrict__ bounds, int i, int ks, int in_size, int &first, int &count) {
    if (!bounds) {
        first = i;
        count = 1;
        return;
    }
    int f = bounds[2 * i], c = bounds[2 * i + 1];
    f = f < 0 ? 0 : f > in_size ? in_size : f;
    const int room = in_size - f < ks ? in_size - f : ks;
    first = f;
    count = c < 0 ? 0 : c > room ? room : c;
}

__global__ void __launch_bounds__(256) pil_resample_kernel(const uint8_t *__restrict__ src, int N, int h, int w, int pix_stride,
                                                           const int32_t *__restrict__ kx, const int32_t *__restrict__ bx, int ksx,
                                                           const int32_t *__restrict__ ky, const int32_t *__restrict__ by, int ksy,
                                                           int H, int W, int tile_h, int tiles_x, uint8_t *__restrict__ dst,
                                                           const uint8_t *__restrict__ gt, int pred_min,
                                                           long long *__restrict__ counts) {
    __shared__ uint8_t sh[LDS_ROWS][TILE_W];
    __shared__ unsigned scnt[2];
    const int tid = threadIdx.x, lane = tid & 63, wave = __builtin_amdgcn_readfirstlane(tid >> 6);
    const int x = (blockIdx.x % tiles_x) * TILE_W + lane, y0 = (blockIdx.x / tiles_x) * tile_h;
    const int y1 = y0 + tile_h < H ? y0 + tile_h : H;
    const bool xin = x < W;
    int xf = 0, xc = 0;
    if (xin) taps_of(kx ? bx : nullptr, x, ksx, w, xf, xc);
    const int32_t *kxr = kx ? kx + (long)(xin ? x : 0) * ksx : nullptr;
    for (int n = blockIdx.y; n < N; n += gridDim.y) {
        const uint8_t *sn = src + (long)n * h * w * pix_stride;
        unsigned c_inter = 0u, c_union = 0u;
        if (tid < 2) scnt[tid] = 0u;
        for (int ya = y0; ya < y1;) {
            // output rows [ya, yb): the longest run whose source rows [lo, hi) fit the window
            int lo, cnt;
            taps_of(ky ? by : nullptr, ya, ksy, h, lo, cnt);
            int hi = lo + cnt, yb = ya + 1;
            while (yb < y1) {
                int f, c;
                taps_of(ky ? by : nullptr, yb, ksy, h, f, c);
                const int nlo = f < lo ? f : lo, nhi = f + c > hi ? f + c : hi;
                if (nhi - nlo > LDS_ROWS) break;
                lo = nlo;
                hi = nhi;
                ++yb;
            }
            __syncthreads();                    // the previous run's readers are done with the window
            for (int r = lo + wave; r < hi; r += WAVES) {
                int v = 0;
                if (xin) {
                    const uint8_t *row = sn + ((long)r * w + xf) * pix_stride;
                    if (kx) {
                        unsigned acc = 1u << (PRECISION_BITS - 1);
                        for (int j = 0; j < xc; ++j) acc += (unsigned)row[(long)j * pix_stride] * (unsigned)kxr[j];
                        v = clip8(acc);
                    } else {
                        v = row[0];
                    }
                }
                sh[r - lo][lane] = (uint8_t)v;
            }
            __syncthreads();
            for (int y = ya + wave; y < yb; y += WAVES) {
                int f, c;
                taps_of(ky ? by : nullptr, y, ksy, h, f, c);
                if (!xin) continue;
                int v;
                if (ky) {
                    const int32_t *kyr = ky + (long)y * ksy;
                    unsigned acc = 1u << (PRECISION_BITS - 1);
                    for (int j = 0; j < c; ++j) acc += (unsigned)sh[f - lo + j][lane] * (unsigned)kyr[j];
                    v = clip8(acc);
                } else {
                    v = sh[f - lo][lane];
                }
                const long o = ((long)n * H + y) * W + x;
                if (dst) dst[o] = (uint8_t)v;
                if (counts) {
                    const bool p = v >= pred_min, g = gt[o] != 0;
                    c_inter += p && g;
                    c_union += p || g;
                }
            }
            ya = yb;
        }
        if (counts) {
#pragma unroll
            for (int o = 32; o > 0; o >>= 1) {
                c_inter += __shfl_xor(c_inter, o);
                c_union += __shfl_xor(c_union, o);
            }
            if (lane == 0) {
                atomicAdd(&scnt[0], c_inter);
                atomicAdd(&scnt[1], c_union);
            }
            __syncthreads();
            if (tid < 2 && scnt[tid]) atomicAdd((unsigned long long *)(counts + (long)n * 2 + tid), (unsigned long long)scnt[tid]);
        }
        __syncthreads();                        // scnt and the window are reused by the next frame
    }
}

}  // namespace

extern "C" int rcf_pil_resample_tile_rows(int h, int H, int ksy) {
    if (h <= 0 || H <= 0 || ksy < 0 || ksy > RCF_PIL_MAX_TAPS) return 0;
    if (ksy == 0) return MAX_TILE_H;            // no vertical pass: a tile reads its own rows
    // t output rows read at most ksy + ceil((t - 1) h / H) + 1 source rows: Pillow's first tap is int(centre - support + 0.5)
    // with centres h / H apart
    for (int t = MAX_TILE_H; t > 1; t >>= 1)
        if (ksy + ((long)(t - 1) * h + H - 1) / H + 1 <= LDS_ROWS) return t;
    return 1;
}

extern "C" int rcf_pil_resample_u8(const uint8_t *src, int N, int h, int w, int pix_stride, const int32_t *kx, const int32_t *bx,
                                   int ksx, const int32_t *ky, const int32_t *by, int ksy, int H, int W, uint8_t *dst,
                                   const uint8_t *gt, int pred_min, long long *counts, void *stream) {
    if (!src || N <= 0 || h <= 0 || w <= 0 || H <= 0 || W <= 0 || (pix_stride != 1 && pix_stride != 3)) return RCF_EINVAL;
    if (!dst && !counts) return RCF_EINVAL;
    if (counts && (!gt || pred_min < 0 || pred_min > 256)) return RCF_EINVAL;
    if (kx ? (!bx || ksx <= 0) : W != w) return RCF_EINVAL;
    if (ky ? (!by || ksy <= 0) : H != h) return RCF_EINVAL;
    const int tile_h = rcf_pil_resample_tile_rows(h, H, ky ? ksy : 0);
    if (tile_h <= 0) return RCF_EINVAL;         // more vertical taps than the window has rows
    const long tiles_x = (W + TILE_W - 1) / TILE_W, tiles_y = (H + tile_h - 1) / tile_h;
    if (tiles_x * tiles_y > 0x7fffffffL) return RCF_EINVAL;
    const unsigned gy = N < 65535 ? (unsigned)N : 65535u;
    hipLaunchKernelGGL(pil_resample_kernel, dim3((unsigned)(tiles_x * tiles_y), gy), dim3(256), 0, rcf_stream(stream), src, N, h,
                       w, pix_stride, kx, bx, ksx, ky, by, ksy, H, W, tile_h, (int)tiles_x, dst, gt, pred_min, counts);
    RCF_LAUNCH_CHECK();
    return 0;
}
