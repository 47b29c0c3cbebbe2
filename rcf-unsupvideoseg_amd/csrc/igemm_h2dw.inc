// igemm_wgrad_h2d_kernel -- the fp16-pair weight gradient with BOTH operands arriving as pair planes (include/rcf_hip.h
// RCF_CONV_X_PLANES + RCF_CONV_DY_PLANES: x from bn_apply, dy from bn_bwd_apply) and delivered global -> LDS by DMA: the kernel
// that splits nothing.  igemm_wgrad_h2t_kernel spends 4.2 VALU instructions per MFMA on loading, splitting and storing both of
// its operands (it is the step's largest family and power-limited: DESIGN.md); here a K-step's VALU work is one pixel walk and
// the address arithmetic of GA + GB DMA pieces per thread.  Included by igemm_conv.hip; built on wgrad_cols.h.
//
// dw[co][rs][c] = sum_m dy[m][co] * x[src(m, rs)][c]: rows i = co (128), cols j = (rs, c) (64 NR), K = pixels, 16 per step.
// LDS image per stage, operand and plane: [64-channel group][16 pixels][128 B]; a wave DMA instruction (1 KB, lane-linear) is
// 8 pixel rows of one group of one plane, so wave w serves pixel half w & 1 of plane w >> 1 in ALL of its pieces: one pixel
// walk and one bounds test per thread and K-step.  The 16-byte chunks of pixel row r are XOR-swizzled by ((r >> 1) & 1) << 2
// (source address and fragment address alike: wgrad_cols.h wgrad_frag_swizzled, as in wgrad_bf16_dma_kernel).  Three stages
// (24 KB each at NR = 4: two workgroups per CU), one barrier per K-step, the pieces of step t + 2 issued among the MFMAs of
// step t (wgrad_cols.h wgrad_dma_kloop).
// Same three partial products per (pixel, co, c) as igemm_wgrad_h2t_kernel, summed over the same pixel chunks in the same order.

// one K-step: fragments of both planes through the transposing reads, three partial products.  `S` is __restrict__ on purpose:
// inlined, the reads carry no-alias scopes against the kernel's LDS-DMA writes (see wgrad_tr_step in igemm_bf16.hip).
template <int MR, int NR, int GA, int GB, int GSZ, int PLA>
__device__ __forceinline__ void wgrad_h2d_step(const char *__restrict__ S, const int (&fa)[MR], const int (&fb)[NR],
                                               f32x16 (&acc)[MR][NR]) {
    f16x8 a[MR][2], b[NR][2];
#pragma unroll
    for (int mr = 0; mr < MR; ++mr)
#pragma unroll
        for (int pl = 0; pl < 2; ++pl) {
            const u32x2 lo = lds_tr16(S + pl * GA * GSZ + fa[mr]);
            const u32x2 hi = lds_tr16(S + pl * GA * GSZ + fa[mr] + 4 * 128);
            a[mr][pl] = __builtin_bit_cast(f16x8, u32x4{lo[0], lo[1], hi[0], hi[1]});
        }
#pragma unroll
    for (int nr = 0; nr < NR; ++nr)
#pragma unroll
        for (int pl = 0; pl < 2; ++pl) {
            const u32x2 lo = lds_tr16(S + PLA + pl * GB * GSZ + fb[nr]);
            const u32x2 hi = lds_tr16(S + PLA + pl * GB * GSZ + fb[nr] + 4 * 128);
            b[nr][pl] = __builtin_bit_cast(f16x8, u32x4{lo[0], lo[1], hi[0], hi[1]});
        }
    constexpr int HA[3] = {1, 0, 0}, HB[3] = {0, 1, 0};
#pragma unroll
    for (int t = 0; t < 3; ++t)
#pragma unroll
        for (int mr = 0; mr < MR; ++mr)
#pragma unroll
            for (int nr = 0; nr < NR; ++nr)
                acc[mr][nr] = __builtin_amdgcn_mfma_f32_32x32x16_f16(a[mr][HA[t]], b[nr][HB[t]], acc[mr][nr], 0, 0, 0);
}

struct WgradOpH2 {
    typedef float T;                                           // a pixel is 4 * pitch bytes ([h: C fp16 | m: C fp16]), like the fp32 tensor it replaces
    static constexpr int BK = 16, PLANES = 2, PASSES = 3;
    static constexpr bool SCALED = true;
    template <int MR, int NR, int PLA>
    static __device__ __forceinline__ void mma(const char *S, const int (&fa)[MR], const int (&fb)[NR], f32x16 (&acc)[MR][NR]) {
        wgrad_h2d_step<MR, NR, PLA / (2 * BK * 128), NR, BK * 128, PLA>(S, fa, fb, acc);
    }
};
template <int NR, bool REGION, bool ONETAP>
__global__ void __launch_bounds__(256, 2) igemm_wgrad_h2d_kernel(WgradParams p) {
    __shared__ __attribute__((aligned(16))) char smem[3 * (2 + NR) * 2 * WgradOpH2::BK * 128];
    wgrad_dma_body<WgradOpH2, NR, REGION, ONETAP>(p, smem);
}
