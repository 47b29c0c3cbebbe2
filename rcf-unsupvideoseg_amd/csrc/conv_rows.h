// Device-side pieces shared by the forward / data-gradient conv kernels: how a GEMM row finds its source pixels.
//     igemm_conv_x3_kernel (igemm_conv.hip)   row origin (behind its pointwise shortcut), tap decode, tap test (+ its BAND term)
//     conv_h2d_kernel      (igemm_h2d.inc)    row origin, tap decode (branch-free divide), tap test
//     conv_h2p_kernel      (igemm_h2p.inc)    row origin (up to its row range's end), tap test; its K walk is incremental
//     conv_bf16_kernel     (igemm_bf16.hip)   row origin, tap decode (branch-free divide), tap test
// Each kernel keeps what is its own: loaders and LDS image, the MFMA step, the K loop and the epilogue (the LDS-DMA rings of
// conv_h2d_kernel and conv_bf16_kernel, the epilogues' row linearisation and their column-sum butterfly were tried here too and
// taken back: they moved instruction text, registers or scratch -- LABNOTES).
// igemm_conv_kernel (the fp32-MFMA test path) walks pointers, not buffer offsets: it takes fast_div only.
// P = the including file's parameter struct (IgemmParams, ConvParams): M, rr, ry0 .. rband, Ho, Wo, Hs, Ws, S, up, off, step, div,
// a_pitch, a_img_stride, kch, rsch and the magics.  Plain __device__ __forceinline__ functions; included by igemm_conv.hip and
// igemm_bf16.hip inside their unnamed namespace, after rcf_common.h (rcf_region_yx), and by wgrad_cols.h (CONV_OOB, oob_unless).
#pragma once

constexpr unsigned CONV_OOB = 0x80000000u;      // byte offset beyond every descriptor's num_records: loads return 0
// byte offset `off` if ok == 1, an out-of-range offset (the load returns zeros) if ok == 0 -- arithmetic, so that a K-step's
// loads stay in one basic block (a select on a load's address tends to become a branch)
__device__ __forceinline__ unsigned oob_unless(unsigned off, int ok) { return (off & ~CONV_OOB) | ((unsigned)(ok - 1) & CONV_OOB); }

// pixel `pix` of a region in the row-major order (region_order.h): the weight gradients (the order of their sums over pixels)
__device__ __forceinline__ void region_yx(int pix, int ry0, int rx0, int rh, int rw, int t, int &y, int &x) {
    rcf_region_yx(pix, ry0, rx0, rh, rw, t, RCF_REGION_ROWMAJOR, y, x);
}

// k / d by the magic of conv_host.h magic_of (0 when d == 1).  NB: without a branch on the (uniform) d == 1 case, which keeps a
// K-step's address arithmetic in one basic block (the DMA kernels)
template <bool NB = false>
__device__ __forceinline__ int fast_div(int k, unsigned magic) {
    if (NB) return (int)(__umulhi((unsigned)k, magic) + ((unsigned)k & (magic ? 0u : ~0u)));
    return magic ? (int)__umulhi((unsigned)k, magic) : k;
}

// Row origin: GEMM row m -> the source coordinates (ay, ax) of its tap (0, 0) and abase, the element offset of that tap from the
// descriptor base (the first image of the tile, n_first) -- STRIDED: of the row's image, the taps divide their own coordinates.
// Rows from row_end on get coordinates no tap brings into range.  order: region_order.h RCF_REGION_*
template <bool STRIDED, class P>
__device__ __forceinline__ void conv_row_origin(const P &p, int m, int row_end, int n_first, int order, int &ay, int &ax, int &abase) {
    if (m < row_end) {
        const int n = m / p.rr;
        int y, x;
        rcf_region_yx(m - n * p.rr, p.ry0, p.rx0, p.rh, p.rw, p.rband, order, y, x);
        ay = y * p.up + p.off;
        ax = x * p.up + p.off;
        abase = (n - n_first) * (int)p.a_img_stride + (STRIDED ? 0 : (ay * p.Ws + ax) * p.a_pitch);
    } else {
        abase = 0;
        ay = -(1 << 28);
        ax = -(1 << 28);
    }
}

// Tap decode: position k of the K loop = (channel chunk q, tap rs, channel inside the chunk) -> tap rs and channel c of the
// source pixel (rcf_common.h rcf_kchunk; the natural order is ONE chunk of Cs: rs * Cs + c is the natural index) ...
template <bool NB, class P>
__device__ __forceinline__ int conv_k_tap(const P &p, int k, int &c) {
    const int q = fast_div<NB>(k, p.rsch_magic);
    const int rem = k - q * p.rsch;
    const int rs = fast_div<NB>(rem, p.kch_magic);
    c = q * p.kch + (rem - rs * p.kch);
    return rs;
}
// ... and the tap's step (dy, dx) from the row origin; returns the unit-stride element offset of the tap's pixel
template <bool NB, class P>
__device__ __forceinline__ int conv_tap_step(const P &p, int rs, int &dy, int &dx) {
    const int r = fast_div<NB>(rs, p.s_magic);
    const int s = rs - r * p.S;
    dy = r * p.step;
    dx = s * p.step;
    return (dy * p.Ws + dx) * p.a_pitch;
}

// Tap test and offset: 0 / 1 (combined with bitwise ops: no short-circuit control flow) = tap (dy, dx) of the row at (ay, ax)
// reads a source pixel; off = its element offset -- abase + tapoff at unit stride; STRIDED: the pixel's own offset + c
template <bool STRIDED, class P>
__device__ __forceinline__ int conv_tap_test(const P &p, int ay, int ax, int abase, int dy, int dx, int tapoff, int c, int &off) {
    int ty = ay + dy, tx = ax + dx, v;
    if (STRIDED) {
        v = (int)(ty >= 0) & (int)(tx >= 0) & (int)(ty % p.div == 0) & (int)(tx % p.div == 0);
        ty /= p.div;
        tx /= p.div;
        v &= (int)(ty < p.Hs) & (int)(tx < p.Ws);
        off = abase + (ty * p.Ws + tx) * p.a_pitch + c;
    } else {
        v = (int)((unsigned)ty < (unsigned)p.Hs) & (int)((unsigned)tx < (unsigned)p.Ws);
        off = abase + tapoff;
    }
    return v;
}
