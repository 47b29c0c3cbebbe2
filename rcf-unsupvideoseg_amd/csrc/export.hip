// The image side of the evaluation export (SegModelBase._eval_outputs over export.py; models/rcf_model.py:241-273,296-315) in one
// launch per batch: every panel of the batch -- a softmax mask plane or a normalised frame, resized to Ho x Wo and rounded to bytes the
// way torchvision.utils.save_image rounds -- written as 8-bit RGB straight into the buffers the PNG / JPEG encoders read.
//
// Arithmetic.  The resize is resize_pos.h's (the float32 source positions and the blend tree of rcf_resize_bilinear_nchw_f32), a frame
// is then (v + 2) / 4, and the byte is export.to_uint8_hwc's three separately rounded float32 steps: t = v * 255, t = t + 0.5,
// clamp to [0, 255], truncate.  No contraction (the library's flag, repeated below), so a byte equals the one the torch route gives.
// A level that is not a number is written as 0, +inf and everything above 255 as 255, -inf as 0: every byte of a panel is written
// whatever the input, and the same bytes on every call.  (An infinite TAP is a NaN level wherever one of its blend weights is 0.)
//
// Mapping.  The bound is the bytes written: a panel reads a quarter (2x masks) or about as many bytes as it writes, and every tap is
// read by several neighbouring outputs, so the taps come from L2.  A thread takes EX_RUN = 4 consecutive pixels of one row = 12 bytes:
// where the run's first byte is dword aligned (a row of a contiguous [.., Ho, Wo, 3] buffer with Wo % 4 == 0, or any row whose byte
// offset is a multiple of 4) they leave as one 12-byte store, and a wave writes 768 consecutive bytes per instruction.  Otherwise:
// scalar bytes up to the next dword boundary, whole dwords, scalar tail (a window at an odd column of a canvas, a short last run).
// A workgroup takes EX_THREADS * EX_ITEMS runs of ONE panel (item = row * runs-per-row + run: no lane idles on a narrow panel),
// blockIdx.y is the panel.  No atomics, no workspace, no host synchronisation.
#pragma clang fp contract(off)
#include "resize_pos.h"

namespace {

constexpr int EX_THREADS = 256;
constexpr int EX_RUN = 4;                  // pixels of a row per thread and item
constexpr int EX_ITEMS = 4;                // items per thread
constexpr int EX_MAX_DST = 2;

struct ExGroup {
    unsigned char *base;                   // first byte of panel (sample 0, slot 0)
    long image, image_row, slot, row, pixel;
    int per_row, n_slots, panels;
    int source[RCF_EXPORT_MAX_SLOTS];
};
struct ExArgs {
    const float *masks, *frames;
    long mask_sample, frame_sample;
    int h, w, H, W, B, Ho, Wo, runs, align, n_groups;
    float msh, msw, fsh, fsw;              // host_scale of the mask and frame resizes
    ExGroup g[EX_MAX_DST];
};

// export.to_uint8_hwc: x * 255, + 0.5, clamp, truncate -- three roundings
__device__ __forceinline__ unsigned ex_quant(float v) {
    float t = v * 255.f;
    t = t + 0.5f;
    return t >= 0.f ? (t < 255.f ? (unsigned)(int)t : 255u) : 0u;       // NaN -> 0
}

typedef unsigned ex_u32x3 __attribute__((ext_vector_type(3)));
typedef ex_u32x3 ex_u32x3_a4 __attribute__((aligned(4)));

// nb = 3 n bytes (n = 1 .. 4 pixels), little-endian in w0 | w1 | w2, to p (pixel stride 3)
__device__ __forceinline__ void ex_store_run(unsigned char *p, unsigned w0, unsigned w1, unsigned w2, int nb) {
    const int mis = (int)((uintptr_t)p & 3);
    if (mis == 0 && nb == 3 * EX_RUN) {
        *reinterpret_cast<ex_u32x3_a4 *>(p) = ex_u32x3{w0, w1, w2};
        return;
    }
    int head = (4 - mis) & 3;
    if (head > nb) head = nb;
    for (int i = 0; i < head; ++i) p[i] = (unsigned char)(w0 >> (8 * i));        // head <= 3: all in w0
    const int sh = 8 * head;
    const unsigned d0 = (unsigned)((((unsigned long long)w1 << 32) | w0) >> sh);
    const unsigned d1 = (unsigned)((((unsigned long long)w2 << 32) | w1) >> sh);
    const unsigned d2 = w2 >> sh;
    const int rem = nb - head, nd = rem >> 2, tail = rem & 3;
    unsigned *q = reinterpret_cast<unsigned *>(p + head);
    if (nd > 0) q[0] = d0;
    if (nd > 1) q[1] = d1;
    if (nd > 2) q[2] = d2;
    const unsigned t = nd == 0 ? d0 : (nd == 1 ? d1 : d2);
    unsigned char *pt = p + head + 4 * nd;
    for (int i = 0; i < tail; ++i) pt[i] = (unsigned char)(t >> (8 * i));
}

__global__ void __launch_bounds__(EX_THREADS) export_panels_kernel(ExArgs a) {
    int p = (int)blockIdx.y;
    const int gi = (a.n_groups > 1 && p >= a.g[0].panels) ? 1 : 0;
    if (gi) p -= a.g[0].panels;
    const ExGroup &g = a.g[gi];
    const int slot = p / a.B, b = p - slot * a.B;
    const int src = g.source[slot];
    const int gr = b / g.per_row, gc = b - gr * g.per_row;
    unsigned char *dst = g.base + (long)gr * g.image_row + (long)gc * g.image + (long)slot * g.slot;
    const bool frame = src == RCF_EXPORT_FRAME;
    const int hi = frame ? a.H : a.h, wi = frame ? a.W : a.w;
    const float sh = frame ? a.fsh : a.msh, sw = frame ? a.fsw : a.msw;
    const long plane = (long)hi * wi;
    const float *s = frame ? a.frames + (long)b * a.frame_sample : a.masks + (long)b * a.mask_sample + (long)src * plane;
    const int items = a.Ho * a.runs;
    const int first = (int)blockIdx.x * (EX_THREADS * EX_ITEMS) + (int)threadIdx.x;
#pragma unroll 1
    for (int k = 0; k < EX_ITEMS; ++k) {
        const int item = first + k * EX_THREADS;
        if (item >= items) break;
        const int y = item / a.runs, x0 = (item - y * a.runs) * EX_RUN;
        const int n = a.Wo - x0 < EX_RUN ? a.Wo - x0 : EX_RUN;
        int y0, y1;
        float ly;
        src_index(y, sh, a.align, hi, y0, y1, ly);
        const float hy = 1.f - ly;
        unsigned lev[EX_RUN][3];
#pragma unroll
        for (int e = 0; e < EX_RUN; ++e) {
            const int xo = x0 + e < a.Wo ? x0 + e : a.Wo - 1;       // lanes past the row's end repeat its last pixel (never stored)
            int c0, c1;
            float lx;
            src_index(xo, sw, a.align, wi, c0, c1, lx);
            const float hx = 1.f - lx;
            const float *r0 = s + (long)y0 * wi, *r1 = s + (long)y1 * wi;
            if (frame) {
#pragma unroll
                for (int c = 0; c < 3; ++c) {
                    const float v = blend(hy, ly, hx, lx, r0[c * plane + c0], r0[c * plane + c1], r1[c * plane + c0], r1[c * plane + c1]);
                    lev[e][c] = ex_quant((v + 2.0f) / 4.0f);
                }
            } else {
                const unsigned q = ex_quant(blend(hy, ly, hx, lx, r0[c0], r0[c1], r1[c0], r1[c1]));
                lev[e][0] = lev[e][1] = lev[e][2] = q;
            }
        }
        unsigned char *o = dst + (long)y * g.row + (long)x0 * g.pixel;
        if (g.pixel == 3) {
            const unsigned w0 = lev[0][0] | (lev[0][1] << 8) | (lev[0][2] << 16) | (lev[1][0] << 24);
            const unsigned w1 = lev[1][1] | (lev[1][2] << 8) | (lev[2][0] << 16) | (lev[2][1] << 24);
            const unsigned w2 = lev[2][2] | (lev[3][0] << 8) | (lev[3][1] << 16) | (lev[3][2] << 24);
            ex_store_run(o, w0, w1, w2, 3 * n);
        } else {
#pragma unroll
            for (int e = 0; e < EX_RUN; ++e)
                if (e < n) {
                    unsigned char *pe = o + (long)e * g.pixel;
                    pe[0] = (unsigned char)lev[e][0], pe[1] = (unsigned char)lev[e][1], pe[2] = (unsigned char)lev[e][2];
                }
        }
    }
}

}  // namespace

extern "C" int rcf_export_geometry(int which) {
    return which == 0 ? EX_RUN : which == 1 ? EX_THREADS : which == 2 ? EX_ITEMS : which == 3 ? EX_MAX_DST : 0;
}

extern "C" int rcf_export_panels_u8(const float *masks, long mask_sample, int C, int h, int w, const float *frames, long frame_sample,
                                    int H, int W, const rcf_export_layout *dst, int n_dst, int B, int Ho, int Wo, int align_corners,
                                    void *stream) {
    const int lim = 1 << 14;
    if (!dst || n_dst < 1 || n_dst > EX_MAX_DST || B < 1 || B > 65535 || Ho < 1 || Wo < 1 || Ho > lim || Wo > lim) return RCF_EINVAL;
    ExArgs a{};
    bool any_mask = false, any_frame = false;
    long panels = 0;
    for (int i = 0; i < n_dst; ++i) {
        const rcf_export_layout &l = dst[i];
        if (!l.base || l.n_slots < 1 || l.n_slots > RCF_EXPORT_MAX_SLOTS || l.per_row < 1 || l.x < 0 || l.y < 0) return RCF_EINVAL;
        if (l.image < 0 || l.image_row < 0 || l.slot < 0 || l.row < 0 || l.pixel < 3 || l.bytes < 0) return RCF_EINVAL;
        ExGroup &g = a.g[i];
        for (int j = 0; j < l.n_slots; ++j) {
            const int src = l.source[j];
            if (src == RCF_EXPORT_FRAME) any_frame = true;
            else if (src >= 0 && src < C) any_mask = true;
            else return RCF_EINVAL;
            g.source[j] = src;
        }
        // the last byte any panel of this layout writes must lie inside the caller's buffer
        const long cols = B < l.per_row ? B : l.per_row, rows = (B - 1) / l.per_row + 1;
        const long last = (long)l.y * l.row + (long)l.x * l.pixel + (rows - 1) * l.image_row + (cols - 1) * l.image +
                          (long)(l.n_slots - 1) * l.slot + (long)(Ho - 1) * l.row + (long)(Wo - 1) * l.pixel + 2;
        if (last >= l.bytes) return RCF_EINVAL;
        g.base = l.base + (long)l.y * l.row + (long)l.x * l.pixel;
        g.image = l.image, g.image_row = l.image_row, g.slot = l.slot, g.row = l.row, g.pixel = l.pixel;
        g.per_row = l.per_row, g.n_slots = l.n_slots, g.panels = l.n_slots * B;
        panels += g.panels;
    }
    if (panels > 65535) return RCF_EINVAL;
    if (any_mask && (!masks || C < 1 || h < 1 || w < 1 || h > lim || w > lim || mask_sample < (long)C * h * w)) return RCF_EINVAL;
    if (any_frame && (!frames || H < 1 || W < 1 || H > lim || W > lim || frame_sample < 3L * H * W)) return RCF_EINVAL;
    a.masks = masks, a.frames = frames, a.mask_sample = mask_sample, a.frame_sample = frame_sample;
    a.h = h, a.w = w, a.H = H, a.W = W, a.B = B, a.Ho = Ho, a.Wo = Wo, a.runs = rcf_cdiv(Wo, EX_RUN);
    a.align = align_corners != 0, a.n_groups = n_dst;
    if (any_mask) a.msh = host_scale(h, Ho, a.align), a.msw = host_scale(w, Wo, a.align);
    if (any_frame) a.fsh = host_scale(H, Ho, a.align), a.fsw = host_scale(W, Wo, a.align);
    const int blocks = rcf_cdiv((long)Ho * a.runs, EX_THREADS * EX_ITEMS);
    hipLaunchKernelGGL(export_panels_kernel, dim3(blocks, (unsigned)panels), dim3(EX_THREADS), 0, rcf_stream(stream), a);
    RCF_LAUNCH_CHECK();
    return 0;
}
