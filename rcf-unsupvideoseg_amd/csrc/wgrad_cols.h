// Device-side pieces shared by the four weight-gradient kernels whose GEMM columns are (tap, input channel) pairs -- the device
// counterpart of conv_host.h:
//     igemm_wgrad_h2t_kernel (igemm_conv.hip)   fp32 in, split to fp16 pairs in registers, 2 LDS stages
//     igemm_wgrad_h2d_kernel (igemm_h2dw.inc)   fp16 pair planes, LDS-DMA, 3 stages
//     wgrad_bf16_kernel      (igemm_bf16.hip)   16-bit, registers, 2 stages
//     wgrad_bf16_dma_kernel  (igemm_bf16.hip)   16-bit, LDS-DMA, 3 stages
// dw[co][rs][c] = sum_m dy[m][co] * x[src(m, rs)][c]: rows i = co, cols j = rs * Cin + c (the weight's own memory order), K = the
// contributing pixels, split over gridDim.z.  Each kernel keeps what is its own: loaders and LDS image, the MFMA step, launch
// bounds, the K-loop of the register kernels (and igemm_wgrad_h2t_kernel its pixel walk).  Here: the launch parameters, the work
// item, the pixel walk, the decode of a column group, the accumulator clear, the fragment offsets of the transposing LDS read,
// the tile store, the three-stage K-loop of the two DMA kernels, and those two kernels' whole body over an operand type
// (wgrad_dma_body: their __global__ wrappers hold the LDS array and the launch bounds).
// Included by igemm_conv.hip and igemm_bf16.hip, once each, inside their unnamed namespace (so that the kernels stay file-local),
// after rcf_common.h (f32x16, rcf_wgrad_item, rcf_wgrad_tile_ij, h2_exponent, pow2f) and their u32x2 / u32x4 typedefs.  The
// asserts below turn a missing one into one message.
#pragma once
static_assert(sizeof(u32x2) == 8 && sizeof(u32x4) == 16 && sizeof(f32x16) == 64,
              "wgrad_cols.h: include after rcf_common.h and the u32x2 / u32x4 typedefs");

// T = float (fp32 tensors, fp16 pair planes typed as fp32) or bf16_t (the build's 16-bit storage type); conv_host.h fill_wgrad
// fills everything but X, DY and the ranges
template <class T>
struct WgradParamsT {
    const T *X, *DY;
    float *OUT;
    int Cout, Cin, R, S;
    int H, W, Ho, Wo, stride, pad, dil;
    int x_pitch, dy_pitch;
    long M;            // N * rr
    long chunk;        // pixels per K-split (a multiple of the kernel's K-step)
    int itiles, jtiles;
    long split_stride; // Cout*R*S*Cin
    int beta;          // only honoured when gridDim.z == 1
    int ry0, rx0, rh, rw;   // contributing output pixels = this rectangle of every image (M = N * rr)
    int rband, rr;          // frame thickness (0 = whole rectangle), pixels per image
    const unsigned *amax_a, *amax_b;   // fp16-pair kernels: max |dy|, max |x| (raw fp32 bits, device scalars)
    int xcd_map;       // rcf_wgrad_item mode (1 = an XCD's workgroups share their pixels)
    int cblocks;       // rcf_wgrad_tile_ij (> 0: column tiles per tap, tiles numbered channel-block-major)
    int Ktot;          // R*S*Cin: the GEMM columns of the tap-column kernels
};

#include "conv_rows.h"                            // CONV_OOB, oob_unless, region_yx (shared with the forward / data-gradient kernels)

// gfx950's transposing LDS read: ds_read_b64_tr_b16 gives lane c of a 16-lane group the 4 k-values of channel c0 + c when lane p
// of the group points at row k0 + p/4, channels c0 + 4 (p%4) .. +3.  No register transposes, no row permutation.
typedef short s16x4 __attribute__((__vector_size__(4 * sizeof(short))));
__device__ __forceinline__ u32x2 lds_tr16(const char *p) {
    const s16x4 v = __builtin_amdgcn_ds_read_tr16_b64_v4i16(
        (__attribute__((address_space(3))) s16x4 *)(__attribute__((address_space(3))) char *)p);
    return __builtin_bit_cast(u32x2, v);
}

// ------------------------------------------------------------------------------------------------------------ work item
// a workgroup's tile (first row i0, first column j0), its K-split and the pixels [kbeg, kbeg + klen) of it; n_first = the image
// of the first pixel: the descriptors start there, image indices of the walk are relative to it (32-bit offsets)
struct WgradItem {
    int i0, j0, split, klen, n_first;
    long kbeg;
};
template <int BM, int BN, class P>
__device__ __forceinline__ WgradItem wgrad_item(const P &p) {
    WgradItem it;
    int tile, tile_i, tile_j;
    rcf_wgrad_item(p.xcd_map, tile, it.split);
    rcf_wgrad_tile_ij(tile, p.itiles, p.jtiles, p.cblocks, tile_i, tile_j);
    it.i0 = tile_i * BM;
    it.j0 = tile_j * BN;
    it.kbeg = (long)it.split * p.chunk;
    const long kend = min(p.M, it.kbeg + p.chunk);
    it.klen = (int)(kend - it.kbeg);
    it.n_first = (int)(it.kbeg / p.rr);
    return it;
}
// the descriptors: dy from the item's first pixel (whole tensors: the contributing pixels are the rows of dy in order, no walk
// needed) or first image (REGION), x from its first image
template <bool REGION, class P>
__device__ __forceinline__ __amdgpu_buffer_rsrc_t wgrad_dy_rsrc(const P &p, const WgradItem &it) {
    const long first = REGION ? (long)it.n_first * p.Ho * p.Wo : it.kbeg;
    return __builtin_amdgcn_make_buffer_rsrc((void *)(p.DY + first * p.dy_pitch), 0, (int)CONV_OOB, 0x00020000);
}
template <class P>
__device__ __forceinline__ __amdgpu_buffer_rsrc_t wgrad_x_rsrc(const P &p, const WgradItem &it) {
    return __builtin_amdgcn_make_buffer_rsrc((void *)(p.X + (long)it.n_first * p.H * p.W * p.x_pitch), 0, (int)CONV_OOB, 0x00020000);
}

// ----------------------------------------------------------------------------------------------------------- pixel walk
// the output pixel a thread serves in the current K-step: image pn (relative to n_first), position (py, px), index ppix among the
// image's contributing pixels; advanced by STEP pixels per K-step, K-steps in order.  REGION: a rectangle / frame of every image
// (the three kernels other than igemm_wgrad_h2t_kernel, which keeps its own for its register budget; wgrad_bf16_kernel has one per
// loader pass)
template <bool REGION, int STEP>
struct WgradWalk {
    int pn, py, px, ppix;
    template <class P>
    __device__ __forceinline__ void yx(const P &p) {
        if (REGION) region_yx(ppix, p.ry0, p.rx0, p.rh, p.rw, p.rband, py, px);
        else { py = ppix / p.Wo; px = ppix - py * p.Wo; }
    }
    // at pixel kbeg + row of the work item
    template <class P>
    __device__ __forceinline__ void init(const P &p, const WgradItem &it, int row) {
        const long m = it.kbeg + row;
        pn = (int)(m / p.rr);
        ppix = (int)(m - (long)pn * p.rr);
        yx(p);
        pn -= it.n_first;
    }
    // whole tensors with Wo >= STEP: at most one row wrap per K-step (no branches, no division)
    template <class P>
    __device__ __forceinline__ void advance_rows(const P &p) {
        px += STEP;
        const bool wx = px >= p.Wo;
        px -= wx ? p.Wo : 0;
        py += wx ? 1 : 0;
        const bool wy = py == p.Ho;
        py = wy ? 0 : py;
        pn += wy ? 1 : 0;
    }
    // narrow images and regions: the walk divides
    template <class P>
    __device__ __forceinline__ void advance_div(const P &p) {
        ppix += STEP;
        while (ppix >= p.rr) { ppix -= p.rr; ++pn; }
        yx(p);
    }
};

// --------------------------------------------------------------------------------------------------- column-group decode
// GEMM column jc = rs * Cin + ch -> filter tap (r, s), channel ch inside the tap, and whether the column exists.  ONETAP: Cin is
// a multiple of the tile width, the tile's columns belong to the tap of its first column j0 (block-uniform: scalar registers)
struct WgradCol {
    int r, s, ch;
    bool act;
};
template <bool ONETAP, class P>
__device__ __forceinline__ WgradCol wgrad_col(const P &p, int j0, int jc) {
    WgradCol c;
    const int rs = (ONETAP ? j0 : jc) / p.Cin;
    c.ch = jc - rs * p.Cin;
    c.r = rs / p.S;
    c.s = rs - c.r * p.S;
    c.act = jc < p.Ktot;
    return c;
}

template <int MR, int NR>
__device__ __forceinline__ void wgrad_clear(f32x16 (&acc)[MR][NR]) {
#pragma unroll
    for (int mr = 0; mr < MR; ++mr)
#pragma unroll
        for (int nr = 0; nr < NR; ++nr)
#pragma unroll
            for (int e = 0; e < 16; ++e) acc[mr][nr][e] = 0.f;
}

// ------------------------------------------------------------------------------------------------------ fragment offsets
// Fragment addressing of ds_read_b64_tr_b16 over an LDS image [pixel][channel] of 16-bit values: 16-lane group gi = lane >> 4
// serves rows (channels) 16 (gi & 1) .. +15 of a 32-row MFMA tile and the k half gi >> 1; lane q of the group points at pixel row
// 8 (gi >> 1) + q / 4 (+ 4 for the second read), channels 4 (q % 4) .. +3 of its 16.
//
// Padded pitch (the register-staged kernels): byte offset of channel row0's fragment, + 64 per further 32-row tile.  Row pitch =
// channels * 2 + 64 bytes: the 64-byte runs that a 32-lane half reads from 4 pixel rows are 64 B apart in bank space and the second
// group of the half (channels + 16 = + 32 B) falls into the gaps: 256 distinct bytes per LDS cycle (a pitch of 32 mod 256 made
// neighbouring rows overlap by half: SQ_LDS_BANK_CONFLICT 33 % of the LDS cycles).
__device__ __forceinline__ int wgrad_frag_padded(int lane, int row0, int pitch) {
    const int gi = lane >> 4, q16 = lane & 15;
    return (8 * (gi >> 1) + (q16 >> 2)) * pitch + (row0 + 16 * (gi & 1) + 4 * (q16 & 3)) * 2;
}
// Swizzled groups (the LDS-DMA kernels): image [64-channel group][pixels][128 B], GSZ bytes per group; the 16-byte chunks of pixel
// row r are XOR-swizzled by ((r >> 1) & 1) << 2, source address (wgrad_dma_qsrc) and fragment address alike: the 4 rows x 4 chunks
// a 32-lane half reads cover all 16 chunk positions of the 256-byte bank space (SQ_LDS_BANK_CONFLICT = 0).  Offsets of the N
// 32-row tiles from channel row0 on; (+ 4 and + 16 pixel rows leave bit 1 of the pixel row alone)
template <int GSZ, int N>
__device__ __forceinline__ void wgrad_frag_swizzled(int lane, int row0, int base, int (&f)[N]) {
    const int gi = lane >> 4, q16 = lane & 15;
    const int fprow = 8 * (gi >> 1) + (q16 >> 2);
    const int swz = ((fprow >> 1) & 1) << 2;
    const int cin = 16 * (gi & 1) + 4 * (q16 & 3);             // channel inside a 32-channel tile
    const int wi = (cin & 7) * 2;
#pragma unroll
    for (int t = 0; t < N; ++t) {
        const int c = row0 + t * 32 + cin;
        f[t] = base + (c >> 6) * GSZ + fprow * 128 + ((((c >> 3) & 7) ^ swz) << 4) + wi;
    }
}
// the source chunk (8 channels) of a 64-channel group that lands at chunk position lane & 7 of pixel row prow
__device__ __forceinline__ int wgrad_dma_qsrc(int lane, int prow) { return (lane & 7) ^ (((prow >> 1) & 1) << 2); }

// ------------------------------------------------------------------------------------------------------------ tile store
// A wave's MR x NR accumulator tiles (rows from arow0, columns from brow0 of the workgroup's tile at i0, j0) into out[Cout][Ktot];
// SCALED: (acc * inv_a) * inv_b, the operands' powers of two taken back.  A tile inside the weight tensor that is a split-K
// partial or overwrites is stored with nothing to test (the general loop is ~2 300 instructions in ~250 basic blocks; a
// workgroup's K-loop is ~10 000); beta_in_kernel = beta && gridDim.z == 1: the guarded loop adds what is there.
template <int MR, int NR, bool SCALED>
__device__ __forceinline__ void wgrad_store_tile(const f32x16 (&acc)[MR][NR], float *out, int i0, int j0, int arow0, int brow0, int Cout,
                                                 int Ktot, bool beta_in_kernel, float inv_a, float inv_b) {
    const int lane = threadIdx.x & 63, l31 = lane & 31, kh = lane >> 5;
    auto value = [&](float v) { return SCALED ? (v * inv_a) * inv_b : v; };
    if (i0 + 64 * MR <= Cout && j0 + 64 * NR <= Ktot && !beta_in_kernel) {
#pragma unroll
        for (int mr = 0; mr < MR; ++mr)
#pragma unroll
            for (int e = 0; e < 16; ++e) {
                float *drow = out + (long)(i0 + arow0 + mr * 32 + 4 * kh + (e & 3) + 8 * (e >> 2)) * Ktot + j0 + brow0 + l31;
#pragma unroll
                for (int nr = 0; nr < NR; ++nr) drow[nr * 32] = value(acc[mr][nr][e]);
            }
        return;
    }
#pragma unroll
    for (int mr = 0; mr < MR; ++mr) {
        const int rbase = i0 + arow0 + mr * 32 + 4 * kh;
#pragma unroll
        for (int e = 0; e < 16; ++e) {
            const int co = rbase + (e & 3) + 8 * (e >> 2);
            if (co >= Cout) continue;
            float *drow = out + (long)co * Ktot + j0 + brow0 + l31;
#pragma unroll
            for (int nr = 0; nr < NR; ++nr) {
                if (j0 + brow0 + nr * 32 + l31 >= Ktot) continue;
                float v = value(acc[mr][nr][e]);
                if (beta_in_kernel) v += drow[nr * 32];
                drow[nr * 32] = v;
            }
        }
    }
}

// ------------------------------------------------------------------------------------------------------------ DMA K-loop
// The K-loop of the two LDS-DMA kernels: three LDS stages, one barrier per K-step, the pieces of step t + 2 issued during step t.
//   loads(kt, stage)   the NLD LDS-DMA pieces of K-step kt into `stage`, at the walk's pixel
//   advance_rows()     the walk's branch-free step;  issue(kt, stage) = loads + the walk's step, either kind
//   mma(stage)         NFRAG transposing fragment reads and NMFMA MFMAs on `stage`
// incr (whole tensors, Wo >= K-step): the steady state is ONE basic block -- the fragment reads, then one piece behind each of
// the first MFMAs.  mma's LDS pointers must be __restrict__ (see wgrad_tr_step) or the loads of later steps do not stay in flight.
template <int NLD, int NFRAG, int NMFMA, class Loads, class Advance, class Issue, class Mma>
__device__ __forceinline__ void wgrad_dma_kloop(int KT, bool incr, const Loads &loads, const Advance &advance_rows, const Issue &issue,
                                                const Mma &mma) {
    issue(0, 0);
    if (KT > 1) issue(1, 1);
    if (KT > 1) asm volatile("s_waitcnt vmcnt(%0)" ::"n"(NLD) : "memory");
    else asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
    __builtin_amdgcn_s_barrier();
    int st = 0, kt = 0;
    if (incr) {
        for (; kt + 2 < KT; ++kt) {
            const int st2 = st >= 1 ? st - 1 : 2;         // (st + 2) % 3
            mma(st);
            loads(kt + 2, st2);
            advance_rows();
            __builtin_amdgcn_sched_group_barrier(0x100, NFRAG, 0);
#pragma unroll
            for (int i = 0; i < NLD; ++i) {
                __builtin_amdgcn_sched_group_barrier(0x008, 1, 0);
                __builtin_amdgcn_sched_group_barrier(0x010, 1, 0);
            }
            __builtin_amdgcn_sched_group_barrier(0x008, NMFMA - NLD, 0);
            asm volatile("s_waitcnt vmcnt(%0) lgkmcnt(0)" ::"n"(NLD) : "memory");
            __builtin_amdgcn_s_barrier();
            st = st == 2 ? 0 : st + 1;
        }
    }
    for (; kt < KT; ++kt) {
        const int st2 = st >= 1 ? st - 1 : 2;
        if (kt + 2 < KT) issue(kt + 2, st2);
        mma(st);
        if (kt + 2 < KT) asm volatile("s_waitcnt vmcnt(%0)" ::"n"(NLD) : "memory");
        else asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
        __builtin_amdgcn_s_barrier();
        st = st == 2 ? 0 : st + 1;
    }
}

// -------------------------------------------------------------------------------------------------------------- DMA body
// The body of the two LDS-DMA kernels.  OP (the including file's operand type) says how a pixel's channels lie in memory:
//   T        element type of the tensors' pointers (bf16_t; float for fp16 pair planes, a pixel = [h: C fp16 | m: C fp16])
//   BK       pixels per K-step;  PLANES  16-bit planes per pixel (1, or 2 = the fp16 pair);  PASSES  MFMA passes per fragment pair
//   SCALED   the store takes the operands' powers of two back (amax_a, amax_b)
//   mma(S, PLA, fa, fb, acc)   one K-step on the stage at S (x image PLA bytes behind the dy image); __restrict__ inside
// LDS image per stage and operand: [plane][64-channel group][BK pixels][128 B], chunks swizzled (wgrad_frag_swizzled).  A wave's DMA
// instruction (1 KB, lane-linear) is 8 pixel rows of one group of one plane: with one plane wave w serves pixel rows 8 w .. + 7, with
// two it serves pixel half w & 1 of plane w >> 1 -- one pixel walk and one bounds test per thread and K-step in all of its pieces.
// smem: 3 stages of (GA + GB) * PLANES * BK * 128 bytes, declared by the __global__ wrapper (which also holds the launch bounds).
template <class OP, int NR, bool REGION, bool ONETAP>
__device__ __forceinline__ void wgrad_dma_body(const WgradParamsT<typename OP::T> &p, char *smem) {
    constexpr int MR = 2, BM = 64 * MR, BN = 64 * NR, BK = OP::BK, PLANES = OP::PLANES;
    constexpr int GA = BM / 64, GB = BN / 64;                  // channel groups per plane = DMA instructions per wave and K-step
    constexpr int GSZ = BK * 128;                              // bytes of one group of one plane: BK pixels x 128 B
    constexpr int PLA = PLANES * GA * GSZ, PLB = PLANES * GB * GSZ, STAGE = PLA + PLB;
    constexpr int NLD = GA + GB;

    const WgradItem it = wgrad_item<BM, BN>(p);
    const int i0 = it.i0, j0 = it.j0, klen = it.klen;
    const int tid = threadIdx.x, lane = tid & 63;
    const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);
    const int wm = wave >> 1, wn = wave & 1;
    const __amdgpu_buffer_rsrc_t rsA = wgrad_dy_rsrc<REGION>(p, it), rsB = wgrad_x_rsrc(p, it);

    // this thread's plane and pixel row of the K-step, and the source chunk of its position inside a 128-byte group row
    const int plane = PLANES == 2 ? wave >> 1 : 0, rows8 = PLANES == 2 ? wave & 1 : wave;
    const int prow = 8 * rows8 + (lane >> 3);
    const int qsrc = wgrad_dma_qsrc(lane, prow);
    const int pla_b = plane * 2 * p.dy_pitch, plb_b = plane * 2 * p.x_pitch;     // byte offset of the plane inside a pixel
    WgradWalk<REGION, BK> w;
    w.init(p, it, prow);
    const bool incr = !REGION && p.Wo >= BK;
    int cha[GA];
    bool acta[GA];
    WgradCol col[GB];
#pragma unroll
    for (int g = 0; g < GA; ++g) {
        cha[g] = i0 + 64 * g + 8 * qsrc;
        acta[g] = cha[g] < p.Cout;
    }
#pragma unroll
    for (int g = 0; g < GB; ++g) col[g] = wgrad_col<ONETAP>(p, j0, j0 + 64 * g + 8 * qsrc);
    auto loads = [&](int kt, int stage) {                  // K-steps are issued in order: the walk advances by BK each time
        char *As = smem + stage * STAGE + plane * GA * GSZ + rows8 * 1024;
        char *Bs = smem + stage * STAGE + PLA + plane * GB * GSZ + rows8 * 1024;
        const int mk = kt * BK + prow;
        const bool inb = mk < klen;
        const int dyoff = REGION ? ((w.pn * p.Ho + w.py) * p.Wo + w.px) * p.dy_pitch : mk * p.dy_pitch;
#pragma unroll
        for (int g = 0; g < GA; ++g) {
            const unsigned bo = oob_unless((unsigned)dyoff * (2u * PLANES) + (unsigned)(pla_b + cha[g] * 2), (int)inb & (int)acta[g]);
            __builtin_amdgcn_raw_ptr_buffer_load_lds(rsA, (__attribute__((address_space(3))) void *)(As + g * GSZ), 16, (int)bo, 0, 0, 0);
        }
        if constexpr (ONETAP) {
            const int sy = w.py * p.stride - p.pad + col[0].r * p.dil, sx = w.px * p.stride - p.pad + col[0].s * p.dil;
            const int v = (int)inb & (int)((unsigned)sy < (unsigned)p.H) & (int)((unsigned)sx < (unsigned)p.W);
            const int xoff = ((w.pn * p.H + sy) * p.W + sx) * p.x_pitch;
#pragma unroll
            for (int g = 0; g < GB; ++g) {
                const unsigned bo = oob_unless((unsigned)xoff * (2u * PLANES) + (unsigned)(plb_b + col[g].ch * 2), (int)v & (int)col[g].act);
                __builtin_amdgcn_raw_ptr_buffer_load_lds(rsB, (__attribute__((address_space(3))) void *)(Bs + g * GSZ), 16, (int)bo, 0, 0, 0);
            }
        } else {
#pragma unroll
            for (int g = 0; g < GB; ++g) {
                const int sy = w.py * p.stride - p.pad + col[g].r * p.dil, sx = w.px * p.stride - p.pad + col[g].s * p.dil;
                const int v = (int)inb & (int)col[g].act & (int)((unsigned)sy < (unsigned)p.H) & (int)((unsigned)sx < (unsigned)p.W);
                const unsigned bo = oob_unless((unsigned)(((w.pn * p.H + sy) * p.W + sx) * p.x_pitch) * (2u * PLANES) + (unsigned)(plb_b + col[g].ch * 2), v);
                __builtin_amdgcn_raw_ptr_buffer_load_lds(rsB, (__attribute__((address_space(3))) void *)(Bs + g * GSZ), 16, (int)bo, 0, 0, 0);
            }
        }
    };
    auto advance_rows = [&]() { w.advance_rows(p); };
    auto issue = [&](int kt, int stage) {
        loads(kt, stage);
        if (incr) w.advance_rows(p);
        else w.advance_div(p);
    };

    f32x16 acc[MR][NR];
    wgrad_clear(acc);

    const int arow0 = wm * 32 * MR, brow0 = wn * 32 * NR;
    int fa[MR], fb[NR];
    wgrad_frag_swizzled<GSZ>(lane, arow0, 0, fa);
    wgrad_frag_swizzled<GSZ>(lane, brow0, 0, fb);
    auto mma = [&](int stage) { OP::template mma<MR, NR, PLA>(smem + stage * STAGE, fa, fb, acc); };
    // per K-step: 4 transposing reads per 32-row tile (2 substeps x 2, or 2 planes x 2), PASSES x MR x NR MFMAs
    wgrad_dma_kloop<NLD, 4 * (MR + NR), OP::PASSES * MR * NR>((klen + BK - 1) / BK, incr, loads, advance_rows, issue, mma);

    float inv_a = 1.f, inv_b = 1.f;
    if constexpr (OP::SCALED) {
        inv_a = pow2f(-h2_exponent(*p.amax_a));
        inv_b = pow2f(-h2_exponent(*p.amax_b));
    }
    wgrad_store_tile<MR, NR, OP::SCALED>(acc, p.OUT + (long)it.split * p.split_stride, i0, j0, arow0, brow0, p.Cout, p.Ktot,
                                         p.beta && gridDim.z == 1, inv_a, inv_b);
}
