// Host-side launch helpers shared by the conv entry points of csrc/igemm_conv.hip (fp32 tensors) and csrc/igemm_bf16.hip
// (16-bit tensors): shape and region checks, region -> kernel parameters, and what the weight-gradient planners of the two files
// (plan_wgrad: their cost models differ) literally share -- the split-K search and tail, the one-tap rule, the launch parameters.
// No device code; included by those two files only.
#pragma once
#include <math.h>
#include "rcf_common.h"

// what check_shape of both files asks of a rcf_conv_shape before its own alignment rules
static inline int conv_check_geometry(const rcf_conv_shape *s) {
    if (!s || s->struct_bytes != sizeof(rcf_conv_shape)) return RCF_EINVAL;      // a caller built against another header
    if (s->N <= 0 || s->H <= 0 || s->W <= 0 || s->Cin <= 0 || s->Cout <= 0 || s->R <= 0 || s->S <= 0) return RCF_EINVAL;
    if (s->stride <= 0 || s->dil <= 0 || s->pad < 0) return RCF_EINVAL;
    const int ho = (s->H + 2 * s->pad - s->dil * (s->R - 1) - 1) / s->stride + 1;
    const int wo = (s->W + 2 * s->pad - s->dil * (s->S - 1) - 1) / s->stride + 1;
    if (ho != s->Ho || wo != s->Wo) return RCF_EINVAL;
    if ((long)s->N * s->Ho * s->Wo >= (1L << 31) || (long)s->N * s->H * s->W >= (1L << 31)) return RCF_EINVAL;
    return 0;
}

static inline unsigned magic_of(int d) { return d <= 1 ? 0u : (unsigned)((1ull << 32) / (unsigned)d + 1ull); }

static inline bool korder_chunked(unsigned flags) { return !(flags & RCF_CONV_KORDER_NATURAL); }

// rectangle (or frame of width `band`) of a [N, H, W] tensor; null = everything
static inline bool region_ok(const rcf_conv_region *r, int H, int W) {
    return !r || (r->y0 >= 0 && r->x0 >= 0 && r->h > 0 && r->w > 0 && r->y0 + r->h <= H && r->x0 + r->w <= W &&
                  r->band >= 0 && (r->band == 0 || (2 * r->band < r->h && 2 * r->band < r->w)));
}

static inline int region_pixels(const rcf_conv_region *r, int H, int W) {       // contributing pixels per image
    if (!r) return H * W;
    return r->band > 0 ? 2 * r->band * r->w + 2 * r->band * (r->h - 2 * r->band) : r->h * r->w;
}

// the region fields of a weight-gradient launch (WgradParamsT of wgrad_cols.h); the caller checked region_ok over Ho x Wo
template <class P>
static inline void fill_region(P &p, const rcf_conv_region *r, int N, int H, int W) {
    p.ry0 = r ? r->y0 : 0; p.rx0 = r ? r->x0 : 0; p.rh = r ? r->h : H; p.rw = r ? r->w : W;
    p.rband = r ? r->band : 0;
    p.rr = region_pixels(r, H, W);
    p.M = (decltype(p.M))N * p.rr;
}

// the same for the GEMM rows [N, H, W] of a forward or data-gradient launch (IgemmParams, ConvParams).  Returns 0 / RCF_EINVAL.
template <class P>
static inline int set_region(P &p, const rcf_conv_region *r, int N, int H, int W) {
    if (!region_ok(r, H, W) || H <= 0 || W <= 0) return RCF_EINVAL;               // (no region: the whole tensor, not an empty one)
    fill_region(p, r, N, H, W);
    return 0;
}

// The GEMM view of a forward (x -> y) or data-gradient (dy -> dx) launch (P = IgemmParams, ConvParams): rows = the pixels of y / dx,
// columns = its channels, K = (tap, source channel); source coordinate t = y * up + off + r * step, valid iff t >= 0, t % div == 0
// and t / div inside the source.  Everything but the operands, the region and the epilogue.
template <class P>
static inline void fill_gemm_view(P &p, const rcf_conv_shape *s, bool dgrad) {
    p.flags = s->flags;
    p.S = s->S;
    if (dgrad) {
        p.Ncol = s->Cin; p.K = s->R * s->S * s->Cout;
        p.Ho = s->H; p.Wo = s->W; p.Hs = s->Ho; p.Ws = s->Wo; p.Cs = s->Cout;
        p.up = 1; p.off = s->pad; p.step = -s->dil; p.div = s->stride;
        p.a_pitch = s->y_pitch; p.a_img_stride = (long)s->Ho * s->Wo * s->y_pitch; p.y_pitch = s->x_pitch;
    } else {
        p.Ncol = s->Cout; p.K = s->R * s->S * s->Cin;
        p.Ho = s->Ho; p.Wo = s->Wo; p.Hs = s->H; p.Ws = s->W; p.Cs = s->Cin;
        p.up = s->stride; p.off = -s->pad; p.step = s->dil; p.div = 1;
        p.a_pitch = s->x_pitch; p.a_img_stride = (long)s->H * s->W * s->x_pitch; p.y_pitch = s->y_pitch;
    }
}

// The K order of a forward / data-gradient launch (rcf_common.h rcf_kchunk) into the launch parameters or the plan: the channel
// chunk width (Cs = the natural order: one chunk), taps * width, and their magics.  width: RCF_KCHUNK_F32 / RCF_KCHUNK_BF16
template <class P>
static inline void fill_korder(P &p, unsigned flags, int taps, int Cs, int width) {
    const int kch = rcf_kchunk(korder_chunked(flags), taps, Cs, width);
    p.kch = kch ? kch : Cs;
    p.rsch = taps * p.kch;
    p.kch_magic = magic_of(p.kch);
    p.rsch_magic = magic_of(p.rsch);
}

// 32-bit arithmetic of the forward / data-gradient kernels: the K walk's divisions by magic (kend = K + one K-step: the
// look-ahead runs one step past the end) and the descriptor offsets of the activation operand -- the images one row tile can
// touch must lie within 2 GiB of the first one.  rr = rows per image, esize = bytes per element
static inline bool conv_offsets_fit(int kend, int rsch, int rr, long a_img_stride, int esize) {
    return (long)kend * rsch < (1L << 32) && (256 / (long)rr + 2) * a_img_stride * esize < (1L << 31);
}

// Split K (the M pixels) of a weight gradient over `c` workgroups per tile, c in 1..hi, on `slots` resident workgroups.  Cost
// model in microseconds: rounds(c) x pixels per workgroup x time per pixel (px_us) + the fixed-order reduction, which reads c
// copies of the weight gradient (wbytes each, ~2 bytes/us/1e6 effective).  Small weights on many pixels (layer1) want hundreds
// of splits, large weights on few pixels (layer4) a handful.
static inline long splitk_search(long tiles, long M, long slots, long hi, double px_us, double wbytes) {
    double best = 1e30;
    long sk = 1;
    for (long c = 1; c <= hi; ++c) {
        const double rounds = (double)((tiles * c + slots - 1) / slots);
        const double cost = rounds * (double)((M + c - 1) / c) * px_us + (c > 1 ? (double)c * wbytes / 2.0e6 + 3.0 : 0.0);
        if (cost < best - 1e-9) { best = cost; sk = c; }
    }
    return sk;
}

// 32-bit descriptor offsets: the images (and dy rows) one pixel chunk touches must span < 2 GiB.  Halves the chunk (kept a
// multiple of `unit` pixels) until they do; RR = pixels per image, esize = bytes per element.
static inline long splitk_chunk_fit(long chunk, long unit, long RR, const rcf_conv_shape *s, int esize) {
    const long img_bytes = (long)s->H * s->W * s->x_pitch * esize, dy_bytes = (long)s->Ho * s->Wo * s->y_pitch * esize;
    while (chunk > unit && ((chunk / RR + 2) * img_bytes >= (1L << 31) || (chunk / RR + 2) * dy_bytes >= (1L << 31)))
        chunk = (chunk / 2 + unit - 1) / unit * unit;
    return chunk;
}

// The tail of both weight-gradient planners (PL = the file's WgradPlan, with mr / nr / itiles / jtiles set): `sk` splits of the M
// pixels in chunks of whole K-steps (`unit` pixels; `fit`: halved until 32-bit offsets reach, splitk_chunk_fit), and the column
// tiles of one tap -- onetap: a tile's 64 nr columns lie inside one tap; cblocks > 0: tiles numbered channel-block-major
// (rcf_common.h rcf_wgrad_tile_ij).
template <class PL>
static inline void wgrad_plan_tail(PL &pl, const rcf_conv_shape *s, long M, long RR, long sk, long unit, bool fit, int esize) {
    long chunk = ((M + sk - 1) / sk + unit - 1) / unit * unit;
    if (fit) chunk = splitk_chunk_fit(chunk, unit, RR, s, esize);
    pl.chunk = chunk;
    pl.splitk = (int)((M + chunk - 1) / chunk);
    pl.onetap = s->Cin % (64 * pl.nr) == 0;
    pl.cblocks = pl.onetap && s->R * s->S > 1 && !(s->flags & RCF_CONV_NO_WGRAD_XCD) ? s->Cin / (64 * pl.nr) : 0;
}

// KERNEL<ARGS..., B> / KERNEL<ARGS..., B1, B2> picked by run-time flags, through the including file's RCF_GO(kernel) launch macro
#define RCF_GO_B(b, KERNEL, ...) do { if (b) RCF_GO(KERNEL<__VA_ARGS__, true>); else RCF_GO(KERNEL<__VA_ARGS__, false>); } while (0)
#define RCF_GO_BB(b1, b2, KERNEL, ...) \
    do { if (b1) RCF_GO_B(b2, KERNEL, __VA_ARGS__, true); else RCF_GO_B(b2, KERNEL, __VA_ARGS__, false); } while (0)

static inline size_t wgrad_workspace_bytes(int splitk, const rcf_conv_shape *s) {    // the split-K partial results
    return splitk <= 1 ? 0 : (size_t)splitk * s->Cout * s->R * s->S * s->Cin * sizeof(float);
}

// the launch parameters both weight gradients fill the same way (P = a WgradParamsT of wgrad_cols.h; X, DY and the ranges: the caller)
template <class P, class PL>
static inline void fill_wgrad(P &p, const PL &pl, const rcf_conv_shape *s, const rcf_conv_region *r, int beta, float *dw, void *workspace) {
    p.OUT = pl.splitk > 1 ? (float *)workspace : dw;
    p.Cout = s->Cout; p.Cin = s->Cin; p.R = s->R; p.S = s->S;
    p.H = s->H; p.W = s->W; p.Ho = s->Ho; p.Wo = s->Wo; p.stride = s->stride; p.pad = s->pad; p.dil = s->dil;
    p.x_pitch = s->x_pitch; p.dy_pitch = s->y_pitch;
    fill_region(p, r, s->N, s->Ho, s->Wo);
    p.chunk = pl.chunk; p.itiles = pl.itiles; p.jtiles = pl.jtiles;
    p.split_stride = (long)s->Cout * s->R * s->S * s->Cin; p.beta = beta;
    p.xcd_map = (s->flags & RCF_CONV_NO_WGRAD_XCD) ? 0 : 1;
    p.cblocks = pl.cblocks;
    p.Ktot = s->R * s->S * s->Cin;
}
