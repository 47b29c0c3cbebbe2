// conv_h2d_kernel -- forward / data gradient on fp16 pairs with BOTH operands delivered global -> LDS by DMA
// (buffer_load ... lds): no staging registers, no split, no ds_write.  Included by igemm_conv.hip.
//
// What makes that possible is the operand FORMAT, not the kernel: the activation operand arrives already split -- the batch-norm
// passes that produce a conv's input (bn_apply) and its output gradient (bn_bwd_apply) are HBM-bound with an idle vector ALU,
// so they emit x * 2^k = h + m as two fp16 planes per pixel ("pair planes": [pixel][h: C fp16 | m: C fp16], the byte size and
// pixel pitch of the fp32 tensor they replace) at a power-of-two scale from an UPPER BOUND of the tensor's range that is known
// before the pass (csrc/bn.hip).  The weight operand is the plane-separated LDS image rcf_conv_weight_pairs2_f32 already writes
// for conv_h2p_kernel.  The conv kernels then spend their issue slots and -- they are power-limited (DESIGN.md) -- their energy
// on the three MFMA passes: the K-step's VALU work is the address arithmetic of 2 + NR DMA pieces per thread.
//
// Same arithmetic as igemm_conv_x3_kernel<.., NP = 2>: the same three partial products in the same K order into the same
// accumulators, so results are bit-identical for operands whose split values agree (the split is exact in the scale: h and m of
// an element do not depend on the power of two unless m leaves fp16's normal range).
//
// Tile 128 x (64 NR), K-step 16, THREE LDS stages of (128 + 64 NR) rows x 2 planes x 32 B (24 KB at NR = 4: two workgroups per
// CU), one barrier per K-step, the pieces of step t + 2 issued among the MFMAs of step t (one basic block, counted vmcnt), as in
// conv_bf16_kernel<.., DMA, SCHED = 1>.  A wave DMA instruction writes 1 KB lane-linear = 32 tile rows of one plane; the
// 16-byte halves of a row are swapped on rows with bit 3 set (mma_x3's conflict-free fragment layout), which for the activation
// operand is applied to the SOURCE address and for the weights is already in the memory image.

template <int NR, bool STRIDED, bool DGRAD, bool BST = false>
__global__ void __launch_bounds__(256, 2) conv_h2d_kernel(IgemmParams p) {
    constexpr int MR = 2, WM = 2, WN = 2;
    constexpr int BM = 32 * MR * WM, BN = 32 * NR * WN, BKT = 16;
    constexpr int PA = BM * 32, PB = BN * 32, STAGE = 2 * (PA + PB), NST = 3, AHEAD = NST - 1;
    constexpr int NLD = 2 + NR;                               // LDS-DMA instructions per thread and K-step
    __shared__ __attribute__((aligned(16))) char smem[NST * STAGE];

    int tile_m, tile_n;
    rcf_conv_tile((int)blockIdx.x, p.mtiles8, p.ntiles, p.colmap, tile_m, tile_n);
    if (tile_m >= p.mtiles) return;
    const int m0 = tile_m * BM, n0 = tile_n * BN;

    const int tid = threadIdx.x, lane = tid & 63;
    const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);
    const int wm = wave / WN, wn = wave - wm * WN;

    const int HoWo = p.rr;
    const int n_first = m0 / HoWo;
    const __amdgpu_buffer_rsrc_t rsA = __builtin_amdgcn_make_buffer_rsrc(
        const_cast<float *>(p.A + (long)n_first * p.a_img_stride), 0, (int)CONV_OOB, 0x00020000);
    const __amdgpu_buffer_rsrc_t rsB = __builtin_amdgcn_make_buffer_rsrc(const_cast<void *>(p.b_pairs2), 0, p.b_bytes, 0x00020000);

    // ---- A: this thread serves tile row 32 wave + lane / 2 in both planes; its LDS position holds half (lane & 1), which on
    // rows with bit 3 set is the OTHER half of the K-step's 16 channels
    const int arow = 32 * wave + (lane >> 1);
    const int srch = (lane & 1) ^ ((arow >> 3) & 1);
    const int plane_b = 2 * p.a_pitch;                        // bytes from the h plane to the m plane of a pixel
    int abase, ay, ax;                                        // fp32-element offset of tap (0, 0) of the row (STRIDED: of the image)
    conv_row_origin<STRIDED>(p, m0 + arow, p.M, n_first, RCF_REGION_ROWMAJOR, ay, ax, abase);
    // ---- B: NR pieces of 32 weight rows per wave: planes {0, 1} x row blocks {wave, wave + 4, ..} (NR = 1: one piece,
    // plane wave / 2, row block wave % 2).  The memory image is the LDS image: a piece is 1 KB of consecutive bytes.
    unsigned bbase[NR];
    int bdst[NR];
#pragma unroll
    for (int i = 0; i < NR; ++i) {
        const int plane = NR >= 2 ? (i & 1) : (wave >> 1);
        const int rb = NR >= 2 ? wave + 4 * (i >> 1) : (wave & 1);
        const int j = n0 + 32 * rb + (lane >> 1);
        bbase[i] = j < p.Ncol ? ((unsigned)plane * (unsigned)p.Ncol + (unsigned)j) * 32u + (unsigned)(lane & 1) * 16u : CONV_OOB;
        bdst[i] = 2 * PA + plane * PB + rb * 1024;
    }
    const unsigned kstride = 2u * (unsigned)p.Ncol * 32u;      // bytes of one K-step of the weight operand (two planes)

    auto issue = [&](int kt, int stage) {
        char *st = smem + stage * STAGE;
        int c, dy, dx, off;                      // (the launch checks K % 16 == 0: no step runs past the end of K)
        const int rs = conv_k_tap<true>(p, kt * BKT + 8 * srch, c);
        const int tapoff = conv_tap_step<true>(p, rs, dy, dx);
        const int v = conv_tap_test<STRIDED>(p, ay, ax, abase, dy, dx, tapoff, 0, off);
        const unsigned b0 = (unsigned)off * 4u + (unsigned)c * 2u;
#pragma unroll
        for (int i = 0; i < NR; ++i)
            __builtin_amdgcn_raw_ptr_buffer_load_lds(rsB, (__attribute__((address_space(3))) void *)(st + bdst[i]), 16,
                                                     (int)(bbase[i] + (unsigned)kt * kstride), 0, 0, 0);
        __builtin_amdgcn_raw_ptr_buffer_load_lds(rsA, (__attribute__((address_space(3))) void *)(st + wave * 1024), 16,
                                                 (int)oob_unless(b0, v), 0, 0, 0);
        __builtin_amdgcn_raw_ptr_buffer_load_lds(rsA, (__attribute__((address_space(3))) void *)(st + PA + wave * 1024), 16,
                                                 (int)oob_unless(b0 + (unsigned)plane_b, v), 0, 0, 0);
    };

    f32x16 acc[MR][NR];
#pragma unroll
    for (int mr = 0; mr < MR; ++mr)
#pragma unroll
        for (int nr = 0; nr < NR; ++nr)
#pragma unroll
            for (int e = 0; e < 16; ++e) acc[mr][nr][e] = 0.f;
    const int arow0 = wm * 32 * MR, brow0 = wn * 32 * NR;
    const int KT = p.K / BKT;                                 // the launch checks K % 16 == 0

    // (This ring and conv_bf16_kernel's were tried as one function of (KT, issue, mma) in conv_rows.h: the steady-state loops came
    // out an instruction apart from the ones below in most instances of both kernels, so each kernel keeps its own.)
    // wait until the pieces of step kt + 1 have landed: those of later steps already issued stay in flight
    auto wait_next = [&](int kt) {
        const int later = min(KT - 1, kt + AHEAD) - (kt + 1);
        if (later >= 1) asm volatile("s_waitcnt vmcnt(%0)" ::"n"(NLD) : "memory");
        else asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
    };
#pragma unroll
    for (int i = 0; i < AHEAD; ++i)
        if (i < KT) issue(i, i);
    wait_next(-1);
    __builtin_amdgcn_s_barrier();
    int st = 0, kt = 0;
    // steady state as ONE basic block (unconditional issue, constant wait count): fragment reads, then one piece behind each of
    // the first MFMAs -- a piece's issue (tens of cycles) runs under the matrix pipe's work instead of ahead of it
    for (; kt + AHEAD < KT; ++kt) {
        const int stn = st + AHEAD >= NST ? st + AHEAD - NST : st + AHEAD;
        const char *As = smem + st * STAGE;
        mma_x3<MR, NR, PA, PB, false, 2, true>(As, As + 2 * PA, arow0, brow0, lane, acc);
        issue(kt + AHEAD, stn);                  // in program order BEHIND the fragment reads (LDS write after LDS reads)
        __builtin_amdgcn_sched_group_barrier(0x100, 2 * (MR + NR), 0);
#pragma unroll
        for (int i = 0; i < NLD; ++i) {
            __builtin_amdgcn_sched_group_barrier(0x008, 1, 0);
            __builtin_amdgcn_sched_group_barrier(0x010, 1, 0);
        }
        __builtin_amdgcn_sched_group_barrier(0x008, 3 * MR * NR - NLD, 0);
        // the MFMAs may sink below the barrier (registers only); the fragment reads may not: the next step's pieces overwrite
        // this stage
        asm volatile("s_waitcnt vmcnt(%0) lgkmcnt(0)" ::"n"((AHEAD - 1) * NLD) : "memory");
        __builtin_amdgcn_s_barrier();
        st = st == NST - 1 ? 0 : st + 1;
    }
    for (; kt < KT; ++kt) {
        const char *As = smem + st * STAGE;
        mma_x3<MR, NR, PA, PB, false, 2, true>(As, As + 2 * PA, arow0, brow0, lane, acc);
        wait_next(kt);
        __builtin_amdgcn_s_barrier();
        st = st == NST - 1 ? 0 : st + 1;
    }
    conv_epilogue_tr<MR, NR, WM, WN, DGRAD, 2, BST>(p, acc, smem, tile_m, m0, n0, h2_exponent(*p.amax_a), h2_exponent(*p.amax_b));
}
