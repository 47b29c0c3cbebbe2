// DAVIS region and boundary measures on the device (tools/davis2016-evaluation/davis2017/metrics.py of the reference):
// per frame the two integers of db_eval_iou (intersection, union) and the four of f_measure (boundary pixels of the
// prediction and of the annotation, and how many of each lie within the disk of radius r around a boundary pixel of the
// other).  The float64 ratios are formed on the host from these counts, with the reference's expressions.
//
// One block per 64x64 output tile and frame.  The block bit-packs the two masks (void pixels cleared) of the tile plus a
// halo of r + 1 into LDS, one 64-bit word per row and 64 columns, forms the boundary words with shifts (_seg2bmap's edge
// rules included), dilates row by row -- for a row offset dy the source row is ORed over the horizontal run
// |dx| <= floor(sqrt(r^2 - dy^2)) by log-step doubling on a 192-bit window -- and counts with popcount.  Integer atomics:
// the counts do not depend on the order of the blocks.
#include "rcf_common.h"

namespace {

constexpr int TILE_H = 64;                     // output rows per block; the tile is 64 columns wide (one word)
constexpr int RMAX = 64;                       // largest dilation radius (the host API refuses larger)
constexpr int MROWS = TILE_H + 2 * RMAX + 1;   // mask rows: boundary rows + the south neighbour row
constexpr int BROWS = TILE_H + 2 * RMAX;       // boundary rows: output rows +- r
constexpr int MW = 4;                          // mask words per row: column bases x0-64, x0, x0+64, x0+128
constexpr int BW = 3;                          // boundary words per row: column bases x0-64, x0, x0+64

typedef unsigned long long u64;

// 192-bit window (w0 = lowest columns) shifted towards lower positions by s in [0, 128]
__device__ __forceinline__ void shr3(u64 &w0, u64 &w1, u64 &w2, int s) {
    if (s >= 64) {
        w0 = w1; w1 = w2; w2 = 0ull;
        s -= 64;
    }
    if (s >= 64) {
        w0 = w1; w1 = 0ull;
        s -= 64;
    }
    if (s > 0) {
        w0 = (w0 >> s) | (w1 << (64 - s));
        w1 = (w1 >> s) | (w2 << (64 - s));
        w2 = w2 >> s;
    }
}

// bit j of the result = OR of the window's bits 64 + j + dx, |dx| <= h (h <= 64): the centre word dilated by a run of 2h+1
__device__ __forceinline__ u64 run_dilate(u64 l, u64 c, u64 r, int h) {
    if (h == 0) return c;
    const int len = 2 * h + 1;
    u64 s0 = l, s1 = c, s2 = r;                 // invariant: bit p = OR of window bits [p, p + cover)
    int cover = 1;
    while (2 * cover <= len) {
        u64 t0 = s0, t1 = s1, t2 = s2;
        shr3(t0, t1, t2, cover);
        s0 |= t0; s1 |= t1; s2 |= t2;
        cover *= 2;
    }
    if (cover < len) {
        u64 t0 = s0, t1 = s1, t2 = s2;
        shr3(t0, t1, t2, len - cover);
        s0 |= t0; s1 |= t1; s2 |= t2;
    }
    const int o = 64 - h;                       // bit j of the result is window bit o + j
    return o == 64 ? s1 : o == 0 ? s0 : (s0 >> o) | (s1 << (64 - o));
}

__global__ void __launch_bounds__(256) davis_counts_kernel(const uint8_t *__restrict__ pred, const uint8_t *__restrict__ gt,
                                                           const uint8_t *__restrict__ void_px, int N, int H, int W, int r,
                                                           int tiles_x, long long *__restrict__ counts) {
    __shared__ u64 sm[2][MROWS][MW];            // pred & !void, gt & !void; 0 outside the frame
    __shared__ u64 sb[2][BROWS][BW];            // boundary maps; 0 outside the frame
    __shared__ int shw[RMAX + 1];               // half-width of the disk's row at |dy|
    __shared__ unsigned scnt[6];
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const int x0 = (blockIdx.x % tiles_x) * 64, y0 = (blockIdx.x / tiles_x) * TILE_H;
    const int mrows = TILE_H + 2 * r + 1, brows = TILE_H + 2 * r;
    if (tid <= r) {                              // floor(sqrt(r^2 - dy^2)), exact in integers
        const int q = r * r - tid * tid;
        int h = (int)sqrtf((float)q);
        while (h * h > q) --h;
        while ((h + 1) * (h + 1) <= q) ++h;
        shw[tid] = h;
    }
    const long HW = (long)H * W;
    for (int n = blockIdx.y; n < N; n += gridDim.y) {
        if (tid < 6) scnt[tid] = 0u;
        // 1. masks -> bits: one wave per (row, word), lane = column, one ballot per mask
        const uint8_t *pn = pred + n * HW, *gn = gt + n * HW, *vn = void_px ? void_px + n * HW : nullptr;
        const int nwords = r >= 64 ? MW : MW - 1;   // the 4th word only feeds the east neighbour of column x0+127
        for (int it = wave; it < mrows * MW; it += 4) {
            const int i = it / MW, k = it % MW;
            const int y = y0 - r + i, x = x0 - 64 + 64 * k + lane;
            bool p = false, g = false;
            if (k < nwords && y >= 0 && y < H && x >= 0 && x < W) {
                const long o = (long)y * W + x;
                const bool v = vn && vn[o] != 0;
                p = pn[o] != 0 && !v;
                g = gn[o] != 0 && !v;
            }
            const u64 bp = __ballot(p), bg = __ballot(g);
            if (lane == 0) { sm[0][i][k] = bp; sm[1][i][k] = bg; }
        }
        __syncthreads();
        // 2. boundary words (_seg2bmap): interior (m^e)|(m^s)|(m^se); last row m^e; last column m^s; corner 0
        for (int it = tid; it < 2 * brows * BW; it += 256) {
            const int q = it / (brows * BW), rem = it % (brows * BW), i = rem / BW, k = rem % BW;
            const int y = y0 - r + i, base = x0 - 64 + 64 * k;
            u64 b = 0ull;
            if (y >= 0 && y < H && base < W && base + 64 > 0) {
                const u64 m = sm[q][i][k], mn = sm[q][i][k + 1], s = sm[q][i + 1][k], sn = sm[q][i + 1][k + 1];
                const u64 e = (m >> 1) | (mn << 63), se = (s >> 1) | (sn << 63);
                b = y == H - 1 ? (m ^ e) : ((m ^ e) | (m ^ s) | (m ^ se));
                const int lc = W - 1 - base;        // bit of the frame's last column in this word
                if (lc >= 0 && lc < 64) {
                    const u64 bit = 1ull << lc;
                    b = (b & ~bit) | (y == H - 1 ? 0ull : ((m ^ s) & bit));
                }
                u64 cols = ~0ull;                   // columns 0 <= x < W
                if (base < 0) cols &= ~0ull << (-base);
                if (W - base < 64) cols &= (1ull << (W - base)) - 1ull;
                b &= cols;
            }
            sb[q][i][k] = b;
        }
        __syncthreads();
        // 3. dilation + counts: thread = (output row, mask, half of the dy range)
        unsigned c_inter = 0u, c_union = 0u, c_nb = 0u, c_match = 0u;
        {
            const int yl = tid >> 2, q = (tid >> 1) & 1, half = tid & 1;
            const int dlo = half ? 1 : -r, dhi = half ? r : 0;
            u64 d = 0ull;
            for (int dy = dlo; dy <= dhi; ++dy) {
                const int i = yl + r + dy;
                d |= run_dilate(sb[q][i][0], sb[q][i][1], sb[q][i][2], shw[dy < 0 ? -dy : dy]);
            }
            d |= __shfl_xor(d, 1);                  // both halves of the dy range
            const u64 other = __shfl_xor(d, 2);     // the other mask's dilated boundary, same row
            if (half == 0) {
                const u64 b = sb[q][yl + r][1];
                c_nb = __popcll(b);
                c_match = __popcll(b & other);
                if (q == 0) {
                    const u64 mp = sm[0][yl + r][1], mg = sm[1][yl + r][1];
                    c_inter = __popcll(mp & mg);
                    c_union = __popcll(mp | mg);
                }
            }
            // lanes with q == 0 hold the prediction's (n_fg, fg_match), q == 1 the annotation's (n_gt, gt_match)
            unsigned nf = q == 0 ? c_nb : 0u, ng = q == 1 ? c_nb : 0u, fm = q == 0 ? c_match : 0u, gm = q == 1 ? c_match : 0u;
#pragma unroll
            for (int o = 32; o > 0; o >>= 1) {
                c_inter += __shfl_xor(c_inter, o);
                c_union += __shfl_xor(c_union, o);
                nf += __shfl_xor(nf, o);
                ng += __shfl_xor(ng, o);
                fm += __shfl_xor(fm, o);
                gm += __shfl_xor(gm, o);
            }
            if (lane == 0) {
                atomicAdd(&scnt[0], c_inter);
                atomicAdd(&scnt[1], c_union);
                atomicAdd(&scnt[2], nf);
                atomicAdd(&scnt[3], ng);
                atomicAdd(&scnt[4], fm);
                atomicAdd(&scnt[5], gm);
            }
        }
        __syncthreads();
        if (tid < 6 && scnt[tid]) atomicAdd((u64 *)(counts + (long)n * 6 + tid), (u64)scnt[tid]);
        __syncthreads();                            // scnt / sm / sb are reused by the next frame
    }
}

}  // namespace

extern "C" int rcf_davis_counts_u8(const uint8_t *pred, const uint8_t *gt, const uint8_t *void_px, int N, int H, int W,
                                   int radius, long long *counts, void *stream) {
    if (!pred || !gt || !counts || N <= 0 || H <= 0 || W <= 0 || radius < 0 || radius > RMAX) return RCF_EINVAL;
    const long tiles_x = (W + 63) / 64, tiles_y = (H + TILE_H - 1) / TILE_H;
    if (tiles_x * tiles_y > 0x7fffffffL) return RCF_EINVAL;
    const unsigned gy = N < 65535 ? (unsigned)N : 65535u;
    hipLaunchKernelGGL(davis_counts_kernel, dim3((unsigned)(tiles_x * tiles_y), gy), dim3(256), 0, rcf_stream(stream), pred,
                       gt, void_px, N, H, W, radius, (int)tiles_x, counts);
    RCF_LAUNCH_CHECK();
    return 0;
}
