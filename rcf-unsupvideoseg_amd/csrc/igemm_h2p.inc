// Persistent fp16-pair implicit-GEMM kernel ("h2p") for the wide, deep convolutions of the training step -- included by
// igemm_conv.hip inside its anonymous namespace (IgemmParams, region_yx, fast_div, split2h, h2_exponent, pow2f, CONV_OOB).
//
// Why a second kernel.  igemm_conv_x3_kernel (128 x 256 tile, 4 waves, 2 workgroups per CU) keeps the matrix pipe 54-60 %
// busy: two unsynchronised waves share each SIMD and take turns, every wave's K-step is "read fragments, 24 MFMAs, split,
// store, barrier" with nothing of the next step under its own MFMAs, and a 3.1-round grid idles a fifth of the chip in
// its last round (profiles/r02_pmc_conv_summary.txt).  This kernel is built the other way round
// (MI355X_MICROARCH.md, "one wave per SIMD ... 5 single-issue instructions hidden per MFMA"):
//   * ONE wave per SIMD, 512 registers: a wave owns (32 MR) x 64 outputs = MR x 2 accumulator tiles (MR <= 8: 256
//     registers); the four waves of a workgroup take the four 64-column quarters of a (32 MR) x 256 tile, so every wave
//     reads the whole A tile (LDS broadcast) and only its own quarter of B: (2 MR + 4) ds_read_b128 per 6 MR MFMAs;
//   * everything that is not an MFMA -- fragment reads of the NEXT row block (and, at the end, of the next K-step),
//     the fp16 split + LDS stores of the A tile two K-steps ahead, the global loads four K-steps ahead, the LDS-DMA of
//     the weight tile three K-steps ahead -- is issued between the MFMAs of the current K-step: a four-stage LDS ring
//     and ONE barrier per K-step that no MFMA waits for (the stage a step multiplies was published two barriers ago);
//   * weights arrive already split into fp16 planes in the order the LDS tile wants (`pairs2`:
//     [K/16][plane][row][32 B, halves swizzled]) and go global -> LDS by DMA (buffer_load ... lds): no registers, no VALU,
//     no ds_write for the B operand;
//   * PERSISTENT: one workgroup per CU; the GEMM rows are cut into 256 contiguous ranges of whole 32-row blocks
//     (balanced to one block: 102 720 rows = 3 210 blocks = 12 or 13 per CU, where 803 tiles of 128 rows on 512 slots are
//     1.57 rounds), each range is walked in sub-tiles of 4..8 row blocks x all column tiles (few rows but many column
//     tiles: 2, 4, .. neighbouring workgroups share a row range and split the column tiles); XCD x owns 32 consecutive
//     ranges (neighbouring rows share their dilated taps through that XCD's L2).
// Arithmetic and results: the fp16-pair scheme of igemm_conv_x3_kernel (3 partial products, fp32 accumulate, exact
// power-of-two scaling); the contraction order over k within an accumulator is the same (k ascending, m*h', h*m', h*h'
// per 16 k), so outputs are bit-identical to that kernel's (tests/test_kernels_gpu.py::test_conv_h2p_matches_x3).
// Covered: non-strided forward / data gradient, no bias / activation, Ncol % 256 == 0, K % 16 == 0; everything else
// stays on igemm_conv_x3_kernel.

constexpr int H2P_NST = 4;                 // LDS stages
constexpr int H2P_PLANE = 256 * 32;        // one fp16 plane of a 256-row operand tile: 8 KB
constexpr int H2P_STAGE = 4 * H2P_PLANE;   // A_h | A_m | B_h | B_m
constexpr int H2P_G = 256;                 // persistent workgroups = CUs

// sub-tile heights (row blocks of 32) a range of R blocks is walked in: 8s, then a remainder of 4..8 split evenly
__host__ __device__ inline int h2p_pick(int R) {
    if (R >= 12 || R == 8) return 8;
    if (R > 8) return (R + 1) / 2;          // 9..11 -> 5 + 4, 5 + 5, 6 + 5
    return R < 4 ? 4 : R;                   // 1..3: a masked 4-block tile
}
__host__ __device__ inline int h2p_subtiles(int R) {
    int n = 0;
    while (R > 0) { R -= h2p_pick(R); ++n; }
    return n;
}

__device__ __forceinline__ f16x8 h2p_frag(const char *__restrict__ lds, int off) {
    return *reinterpret_cast<const f16x8 *>(lds + off);
}

// One (32 MR) x 256 output tile: rows [row0, row_end) of the GEMM, columns [n0, n0 + 256).
template <int MR>
__device__ __forceinline__ void h2p_tile(const IgemmParams &p, char *__restrict__ smem, const int row0, const int row_end,
                                         const int n0, double *__restrict__ stats_row, const float sa, const float inv_a,
                                         const float inv_b) {
    constexpr int A_PASS = (MR + 1) / 2;                  // 64 rows per loader pass
    const int tid = threadIdx.x;
    const int lane = tid & 63;
    const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);
    const int kq = tid & 3, arow = tid >> 2;
    const int HoWo = p.rr;
    const int n_first = row0 / HoWo;                       // first image this tile touches (block-uniform)
    const __amdgpu_buffer_rsrc_t rsA = __builtin_amdgcn_make_buffer_rsrc(
        const_cast<float *>(p.A + (long)n_first * p.a_img_stride), 0, (int)CONV_OOB, 0x00020000);
    const __amdgpu_buffer_rsrc_t rsB =
        __builtin_amdgcn_make_buffer_rsrc(const_cast<void *>(p.b_pairs2), 0, p.b_bytes, 0x00020000);

    int abase[A_PASS], ay[A_PASS], ax[A_PASS];
    int st_off[A_PASS];
#pragma unroll
    for (int i = 0; i < A_PASS; ++i) {
        const int r = arow + 64 * i;
        const int m = row0 + r;
        st_off[i] = r * 32 + ((((kq >> 1) ^ ((r >> 3) & 1))) << 4) + (kq & 1) * 8;
        conv_row_origin<false>(p, m, row_end, n_first, RCF_REGION_ROWMAJOR, ay[i], ax[i], abase[i]);
    }
    // K walk of the A loads: K-steps are loaded in order (0, 1, 2, ...), Cs % 16 == 0, so a step lies inside one filter tap and
    // (tap, first channel) advance by scalar arithmetic -- no division, no per-thread work
    // K order (rcf_common.h rcf_kchunk): channel chunks of p.kch outer, the taps inside, 16 channels per step innermost; the
    // natural order is one chunk of Cs channels
    int lk = 0, lc = 0, lr = 0, ls = 0, lcb = 0;           // next step's k, channel inside the chunk, tap row / column, chunk base
    const int taps_r = p.rsch / (p.kch * p.S);             // filter rows (block-uniform)
    auto load_a = [&](f32x4 (&dst)[A_PASS]) {
        const int kv = (int)(lk < p.K);
        const int dy = lr * p.step, dx = ls * p.step;
        const int tapoff = (dy * p.Ws + dx) * p.a_pitch + lcb + lc + kq * 4;
#pragma unroll
        for (int i = 0; i < A_PASS; ++i) {
            int off;
            const int v = kv & conv_tap_test<false>(p, ay[i], ax[i], abase[i], dy, dx, tapoff, 0, off);
            dst[i] = __builtin_bit_cast(f32x4, __builtin_amdgcn_raw_buffer_load_b128(rsA, (int)oob_unless((unsigned)off * 4u, v), 0, 0));
        }
        lk += 16;
        lc += 16;
        const int wrap_c = (int)(lc >= p.kch);
        lc = wrap_c ? 0 : lc;
        ls += wrap_c;
        const int wrap_s = (int)(ls >= p.S);
        ls = wrap_s ? 0 : ls;
        lr += wrap_s;
        const int wrap_r = (int)(lr >= taps_r);
        lr = wrap_r ? 0 : lr;
        lcb += wrap_r ? p.kch : 0;
    };
    // weight tile of K-step kt: 16 pieces of 1 KB (plane, 32 rows), four per wave, global -> LDS
    const unsigned b_lane = (unsigned)n0 * 32u + (unsigned)lane * 16u;
    auto issue_b = [&](int kt, int stage) {
        const unsigned kb = (unsigned)kt * (unsigned)p.Ncol * 64u;
        char *Bs = smem + stage * H2P_STAGE + 2 * H2P_PLANE;
#pragma unroll
        for (int j = 0; j < 4; ++j) {
            const int q = 4 * wave + j, plane = q >> 3, rb = q & 7;
            const unsigned src = kb + (unsigned)plane * (unsigned)p.Ncol * 32u + (unsigned)rb * 1024u + b_lane;
            __builtin_amdgcn_raw_ptr_buffer_load_lds(rsB, (__attribute__((address_space(3))) void *)(Bs + plane * H2P_PLANE + rb * 1024),
                                                     16, (int)src, 0, 0, 0);
        }
    };
    auto store_a = [&](int stage, const f32x4 (&src)[A_PASS], int i) {
        char *As = smem + stage * H2P_STAGE;
        u32x2 h, m;
        split2h(src[i], sa, h, m);
        *reinterpret_cast<u32x2 *>(As + st_off[i]) = h;
        *reinterpret_cast<u32x2 *>(As + H2P_PLANE + st_off[i]) = m;
    };

    f32x16 acc[MR][2];
#pragma unroll
    for (int mr = 0; mr < MR; ++mr)
#pragma unroll
        for (int nr = 0; nr < 2; ++nr)
#pragma unroll
            for (int e = 0; e < 16; ++e) acc[mr][nr][e] = 0.f;

    const int l31 = lane & 31, kh = lane >> 5;
    const int fa = l31 * 32 + ((kh ^ ((l31 >> 3) & 1)) << 4);               // this lane's fragment chunk inside a 32-row block
    const int fb = 2 * H2P_PLANE + wave * 2048 + fa;                         // ... of this wave's B rows

    f32x4 ra[2][A_PASS];
    f16x8 aq[2][2], bq[2][2][2];                                             // [buffer][plane], [buffer][nr][plane]
    const int KT = (p.K + 15) >> 4;
    const int KT4 = (KT + 3) & ~3;                                           // whole rounds of the 4-stage ring (zero steps past K)

    // ---- prologue: stages 0 and 1 complete, B(2) in flight, A(2), A(3) in registers
    load_a(ra[0]);
    load_a(ra[1]);
    issue_b(0, 0);
    issue_b(1, 1);
    issue_b(2, 2);
#pragma unroll
    for (int i = 0; i < A_PASS; ++i) store_a(0, ra[0], i);
    load_a(ra[0]);
#pragma unroll
    for (int i = 0; i < A_PASS; ++i) store_a(1, ra[1], i);
    load_a(ra[1]);
    asm volatile("s_waitcnt vmcnt(%0)" ::"n"(2 * A_PASS + 4) : "memory");    // B(0), B(1) landed; B(2), A(2), A(3) may fly
    __syncthreads();
#pragma unroll
    for (int nr = 0; nr < 2; ++nr)
#pragma unroll
        for (int pl = 0; pl < 2; ++pl) bq[0][nr][pl] = h2p_frag(smem, fb + pl * H2P_PLANE + nr * 1024);
#pragma unroll
    for (int pl = 0; pl < 2; ++pl) aq[0][pl] = h2p_frag(smem, fa + pl * H2P_PLANE);

    // ---- K-step kt (stage S = kt % 4, register parity P = kt % 2), one group of 6 MFMAs per row block.  Ahead of a group:
    // the LDS reads of the NEXT group's A fragments (last group: the next step's B and first A fragments, stage S + 1,
    // published two barriers ago).  Beside a group's MFMAs (the scheduler may interleave inside a group, nothing crosses a
    // group boundary): group 0 the LDS-DMA of B(kt + 3) -> stage S + 3; groups 1 .. A_PASS the fp16 split + LDS store of one
    // 64-row pass of A(kt + 2) (registers, loaded two steps ago) -> stage S + 2; the group after them the global loads of
    // A(kt + 4) into the registers just freed.  Then: wait for B(kt + 2) (issued a step ago), barrier.
    auto kstep = [&](auto S_, auto P_, int kt) {
        constexpr int S = decltype(S_)::value, P = decltype(P_)::value;
        constexpr int A0 = (P * MR) & 1;                                     // buffer holding row block 0's A fragments
        const char *cur = smem + S * H2P_STAGE;
        const char *nxt = smem + ((S + 1) & 3) * H2P_STAGE;
#pragma unroll
        for (int mr = 0; mr < MR; ++mr) {
            const int ab = (A0 + mr) & 1;
            if (mr + 1 < MR) {
#pragma unroll
                for (int pl = 0; pl < 2; ++pl) aq[ab ^ 1][pl] = h2p_frag(cur, fa + pl * H2P_PLANE + (mr + 1) * 1024);
            } else {
#pragma unroll
                for (int nr = 0; nr < 2; ++nr)
#pragma unroll
                    for (int pl = 0; pl < 2; ++pl) bq[P ^ 1][nr][pl] = h2p_frag(nxt, fb + pl * H2P_PLANE + nr * 1024);
#pragma unroll
                for (int pl = 0; pl < 2; ++pl) aq[ab ^ 1][pl] = h2p_frag(nxt, fa + pl * H2P_PLANE);
            }
            __builtin_amdgcn_sched_barrier(0);
            if (mr == 0) issue_b(kt + 3, (S + 3) & 3);
            // m*h', h*m', h*h' (smallest partial products first), alternating the two accumulators
            constexpr int HA[3] = {1, 0, 0}, HB[3] = {0, 1, 0};
#pragma unroll
            for (int t = 0; t < 3; ++t)
#pragma unroll
                for (int nr = 0; nr < 2; ++nr)
                    acc[mr][nr] = __builtin_amdgcn_mfma_f32_32x32x16_f16(bq[P][nr][HB[t]], aq[ab][HA[t]], acc[mr][nr], 0, 0, 0);
            static_assert(A_PASS + 1 <= MR - 1, "groups 1 .. A_PASS store, group A_PASS + 1 loads");
            if (mr >= 1 && mr <= A_PASS) store_a((S + 2) & 3, ra[P], mr - 1);
            if (mr == A_PASS + 1) load_a(ra[P]);
            __builtin_amdgcn_sched_barrier(0);
        }
        asm volatile("s_waitcnt vmcnt(%0) lgkmcnt(0)" ::"n"(2 * A_PASS + 4) : "memory");
        __builtin_amdgcn_s_barrier();
    };
    using I0 = std::integral_constant<int, 0>;
    using I1 = std::integral_constant<int, 1>;
    using I2 = std::integral_constant<int, 2>;
    using I3 = std::integral_constant<int, 3>;
    for (int kt = 0; kt < KT4; kt += 4) {
        kstep(I0{}, I0{}, kt);
        kstep(I1{}, I1{}, kt + 1);
        kstep(I2{}, I0{}, kt + 2);
        kstep(I3{}, I1{}, kt + 3);
    }
    asm volatile("s_waitcnt vmcnt(0)" ::: "memory");      // trailing out-of-range pieces / loads of the steps past K
    __syncthreads();                                      // every wave is done with the ring: the next tile may refill it

    // ---- epilogue: transposed accumulators -- lane = pixel (lane & 31) of each row block, registers 4g..4g+3 = output
    // channels 8g + 4(lane >> 5) .. +3 of each 32-column block: 16-byte stores
    const bool full = p.rh == p.Ho && p.rw == p.Wo && p.rband <= 0;
    const int col0 = n0 + wave * 64 + 4 * kh;
    unsigned tmax = 0u;
    float cs[2][16], cq[2][16];
#pragma unroll
    for (int nr = 0; nr < 2; ++nr)
#pragma unroll
        for (int e = 0; e < 16; ++e) { cs[nr][e] = 0.f; cq[nr][e] = 0.f; }
    auto quads = [&](auto BETA_, auto EXTRA_) {             // BETA: accumulate; EXTRA: statistics / range wanted (not by a data gradient)
        constexpr bool BETA = decltype(BETA_)::value, EXTRA = decltype(EXTRA_)::value;
#pragma unroll
        for (int mr = 0; mr < MR; ++mr) {
            const int row = row0 + mr * 32 + l31;
            if (row >= row_end) continue;
            long lin = row;
            if (!full) {
                const int n = row / HoWo;
                int y, x;
                region_yx(row - n * HoWo, p.ry0, p.rx0, p.rh, p.rw, p.rband, y, x);
                lin = ((long)n * p.Ho + y) * p.Wo + x;
            }
            float *drow = p.Y + lin * p.y_pitch + col0;
#pragma unroll
            for (int nr = 0; nr < 2; ++nr)
#pragma unroll
                for (int g = 0; g < 4; ++g) {
                    f32x4 v = {acc[mr][nr][4 * g], acc[mr][nr][4 * g + 1], acc[mr][nr][4 * g + 2], acc[mr][nr][4 * g + 3]};
                    v = (v * inv_a) * inv_b;
                    f32x4 *dst = reinterpret_cast<f32x4 *>(drow + nr * 32 + 8 * g);
                    if (BETA) v += *dst;
                    *dst = v;
                    if (EXTRA) {
#pragma unroll
                        for (int e = 0; e < 4; ++e) {
                            tmax = max(tmax, __float_as_uint(fabsf(v[e])));
                            cs[nr][4 * g + e] += v[e];
                            cq[nr][4 * g + e] = fmaf(v[e], v[e], cq[nr][4 * g + e]);
                        }
                    }
                }
        }
    };
    const bool extra = stats_row != nullptr || p.amax_out != nullptr;
    if (p.beta) { if (extra) quads(std::true_type{}, std::true_type{}); else quads(std::true_type{}, std::false_type{}); }
    else { if (extra) quads(std::false_type{}, std::true_type{}); else quads(std::false_type{}, std::false_type{}); }
    if (stats_row) {                                      // block-uniform: column sums over this tile's pixels (= lanes)
#pragma unroll
        for (int nr = 0; nr < 2; ++nr) {
            const bool b4 = lane & 16, b3 = lane & 8, b2 = lane & 4, b1 = lane & 2;
            float s8[8], q8[8], s4[4], q4[4], s2[2], q2[2];
#pragma unroll
            for (int i = 0; i < 8; ++i) {
                s8[i] = (b4 ? cs[nr][8 + i] : cs[nr][i]) + __shfl_xor(b4 ? cs[nr][i] : cs[nr][8 + i], 16);
                q8[i] = (b4 ? cq[nr][8 + i] : cq[nr][i]) + __shfl_xor(b4 ? cq[nr][i] : cq[nr][8 + i], 16);
            }
#pragma unroll
            for (int i = 0; i < 4; ++i) {
                s4[i] = (b3 ? s8[4 + i] : s8[i]) + __shfl_xor(b3 ? s8[i] : s8[4 + i], 8);
                q4[i] = (b3 ? q8[4 + i] : q8[i]) + __shfl_xor(b3 ? q8[i] : q8[4 + i], 8);
            }
#pragma unroll
            for (int i = 0; i < 2; ++i) {
                s2[i] = (b2 ? s4[2 + i] : s4[i]) + __shfl_xor(b2 ? s4[i] : s4[2 + i], 4);
                q2[i] = (b2 ? q4[2 + i] : q4[i]) + __shfl_xor(b2 ? q4[i] : q4[2 + i], 4);
            }
            float s1 = (b1 ? s2[1] : s2[0]) + __shfl_xor(b1 ? s2[0] : s2[1], 2);
            float q1 = (b1 ? q2[1] : q2[0]) + __shfl_xor(b1 ? q2[0] : q2[1], 2);
            s1 += __shfl_xor(s1, 1);
            q1 += __shfl_xor(q1, 1);
            if ((lane & 1) == 0) {
                const int r = (b4 ? 8 : 0) + (b3 ? 4 : 0) + (b2 ? 2 : 0) + (b1 ? 1 : 0);     // accumulator register = channel
                const int ch = n0 + wave * 64 + nr * 32 + 8 * (r >> 2) + 4 * kh + (r & 3);
                stats_row[ch] = (double)s1;
                stats_row[p.Ncol + ch] = (double)q1;
            }
        }
    }
    if (p.amax_out) {                                     // block-uniform
#pragma unroll
        for (int o = 32; o > 0; o >>= 1) tmax = max(tmax, (unsigned)__shfl_xor((int)tmax, o));
        if (lane == 0 && tmax > __hip_atomic_load(p.amax_out, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT)) atomicMax(p.amax_out, tmax);
    }
}

// DGRAD only names the instantiation (forward and data-gradient launches are different kernels in a profile)
template <bool DGRAD>
__global__ void __launch_bounds__(256, 1) conv_h2p_kernel(IgemmParams p) {
    __shared__ __attribute__((aligned(1024))) char h2p_smem[H2P_NST * H2P_STAGE];
    // XCD x (= block id % 8) owns 32 consecutive positions.  p.h2p_gn consecutive positions (a power of two, chosen by the
    // host so that a workgroup gets >= 12 row blocks when the GEMM has few rows but many column tiles) share one row range
    // and split its column tiles; the 256 / gn row ranges are whole 32-row blocks, balanced to one block.
    const int pos = (blockIdx.x & 7) * (H2P_G / 8) + (blockIdx.x >> 3);
    const int gn = p.h2p_gn, gm = pos / gn, tn0 = (pos - gm * gn) * (p.ntiles / gn), tn1 = tn0 + p.ntiles / gn;
    const int GM = H2P_G / gn;
    const int RB = (p.M + 31) >> 5;
    const int base = RB / GM, extra = RB - base * GM;
    int rb = gm * base + min(gm, extra);
    int R = base + (gm < extra ? 1 : 0);
    const int ka = h2_exponent(*p.amax_a), kb = h2_exponent(*p.amax_b);
    const float sa = pow2f(ka), inv_a = pow2f(-ka), inv_b = pow2f(-kb);
    int sub = 0;
    const int nsub = p.mtiles8;                            // partial statistics rows per workgroup (host: h2p_subtiles of the longest range)
    while (R > 0) {
        const int mr = h2p_pick(R);
        const int row0 = rb * 32;
        const int row_end = min(p.M, (rb + min(mr, R)) * 32);
        double *srow = p.stats ? p.stats + ((long)gm * nsub + sub) * 2 * p.Ncol : nullptr;
        for (int tn = tn0; tn < tn1; ++tn) {
            const int n0 = tn * 256;
            switch (mr) {
                case 8: h2p_tile<8>(p, h2p_smem, row0, row_end, n0, srow, sa, inv_a, inv_b); break;
                case 7: h2p_tile<7>(p, h2p_smem, row0, row_end, n0, srow, sa, inv_a, inv_b); break;
                case 6: h2p_tile<6>(p, h2p_smem, row0, row_end, n0, srow, sa, inv_a, inv_b); break;
                case 5: h2p_tile<5>(p, h2p_smem, row0, row_end, n0, srow, sa, inv_a, inv_b); break;
                default: h2p_tile<4>(p, h2p_smem, row0, row_end, n0, srow, sa, inv_a, inv_b); break;
            }
        }
        R -= mr;
        rb += mr;
        ++sub;
    }
    if (p.stats) {                                        // ranges with fewer sub-tiles than the longest: zero rows (own columns)
        for (; sub < nsub; ++sub) {
            double *srow = p.stats + ((long)gm * nsub + sub) * 2 * p.Ncol;
            for (int c = tn0 * 256 + (int)threadIdx.x; c < tn1 * 256; c += 256) {
                srow[c] = 0.0;
                srow[p.Ncol + c] = 0.0;
            }
        }
    }
}
