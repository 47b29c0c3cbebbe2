// Middlebury flow colours on the device: what flow_vis.flow_to_color computes on the host for the training visualisation grids
// (models/rcf_model.py:222-234,562-575, models/amd/amd_model.py:213-262), for all flow images of a grid in one call.
//
// Per image: rad = sqrt(u^2 + v^2), m = max rad, (u, v) / (m + 1e-5), rad again, a = atan2(-v, -u) / pi, fk = (a + 1) / 2 * 54,
// k0 = floor(fk), k1 = k0 + 1 (55 -> 0), f = fk - k0, per channel col = (1 - f) wheel[k0] + f wheel[k1] (wheel / 255),
// col = 1 - rad (1 - col), byte = floor(255 col).
//
// Arithmetic.  Everything up to f and rad is float32 with IEEE square roots and divisions, as numpy runs it on float32 flows; the
// interpolation tail is fp64, which is what the package's float64 wheel table promotes it to (f = fk - k0 is exact in either type).
// So against a float64 evaluation only the roundings before the tail remain; tests/flowvis_cases.py derives the bound.
// The package's second branch (col * 0.75 where rad > 1) is never taken: after the division by the maximum it is dead in exact
// arithmetic, and float32 can only reach 1 + 2^-23 on the largest-flow pixels, where the radius is taken as 1.
// A level that is not a number (NaN / inf flows, or magnitudes whose squares overflow) is written as 0: every byte of the window
// is written whatever the input, and the same bytes on every call.
//
// Launches.  Images of at most FV_ONE_WG_PIXELS pixels: ONE launch, a workgroup per image, two passes over the image (the second
// read hits the cache).  Larger images: a maximum launch (workgroups of FV_TILE_PIXELS pixels, atomicMax on the bit pattern of the
// non-negative radius -- order-independent, so still the same bits on every call -- into a workspace word per image that is zeroed
// in-stream) and a colour launch.  Neither count depends on the number of images; there is no host synchronisation.
// A thread takes FV_VEC consecutive pixels of a row: 16-byte loads per channel and one 4-byte (u8) or 16-byte (f32) store per plane
// where the layout allows it, scalar accesses otherwise (a window at an odd column, [h, w, 2] flows, [h, w, 3] colours).
// The wheel is a 165-byte __constant__ table; a workgroup expands it into LDS (/ 255 in fp64) once, since k0 differs between lanes.
#include "rcf_common.h"

namespace {

constexpr int FV_THREADS = 256;
constexpr int FV_VEC = 4;                               // pixels of a row per thread
constexpr int FV_TILE_PIXELS = FV_THREADS * FV_VEC;     // per workgroup of the two-launch form
constexpr int FV_ONE_WG_PIXELS = 4096;                  // largest image of the one-launch form
constexpr int FV_NCOLS = 55;

struct FvWheel { unsigned char c[FV_NCOLS][3]; };

// RY 15, YG 6, GC 4, CB 11, BM 13, MR 6: one channel ramps as floor(255 i / len) (or 255 minus that), one is held at 255
constexpr FvWheel fv_make_wheel() {
    FvWheel t{};
    const int len[6] = {15, 6, 4, 11, 13, 6};
    const int held[6] = {0, 1, 1, 2, 2, 0}, ramp[6] = {1, 0, 2, 1, 0, 2};
    int col = 0;
    for (int s = 0; s < 6; ++s)
        for (int i = 0; i < len[s]; ++i, ++col) {
            const int r = 255 * i / len[s];
            t.c[col][held[s]] = 255;
            t.c[col][ramp[s]] = (unsigned char)(s % 2 == 0 ? r : 255 - r);
        }
    return t;
}
__constant__ FvWheel fv_wheel = fv_make_wheel();

struct FvLayout { long image, member, channel, row, col; };
struct FvArgs {
    const float *flow;
    void *out;
    FvLayout s, d;
    int group, h, w, quads;        // quads: FV_VEC-pixel items per row
    int bgr, src_vec, dst_vec;
    float clip;
};

__device__ __forceinline__ long fv_image_offset(const FvLayout &l, int n, int group) {
    const int g = n / group;
    return (long)g * l.image + (long)(n - g * group) * l.member;
}

// the FV_VEC pixels (y, x0 ..) of one image; lanes beyond the row's end stay 0 (radius 0: no effect on the maximum)
__device__ __forceinline__ void fv_load(const FvArgs &a, const float *img, int y, int x0, float *u, float *v) {
    const float *p = img + (long)y * a.s.row + (long)x0 * a.s.col;
    if (a.src_vec && x0 + FV_VEC <= a.w) {
        const f32x4 tu = ld4(p), tv = ld4(p + a.s.channel);
#pragma unroll
        for (int e = 0; e < FV_VEC; ++e) u[e] = tu[e], v[e] = tv[e];
    } else {
#pragma unroll
        for (int e = 0; e < FV_VEC; ++e) {
            const bool in = x0 + e < a.w;
            u[e] = in ? p[(long)e * a.s.col] : 0.f;
            v[e] = in ? p[(long)e * a.s.col + a.s.channel] : 0.f;
        }
    }
    if (a.clip >= 0.f) {
#pragma unroll
        for (int e = 0; e < FV_VEC; ++e) {
            u[e] = fminf(fmaxf(u[e], 0.f), a.clip);
            v[e] = fminf(fmaxf(v[e], 0.f), a.clip);
        }
    }
}

__device__ __forceinline__ unsigned fv_rad_bits(float u, float v) {
    return __float_as_uint(__fsqrt_rn(u * u + v * v)) & 0x7fffffffu;       // a NaN keeps a bit pattern above every number's
}

// maximum over the workgroup, returned to every thread
__device__ __forceinline__ unsigned fv_block_max(unsigned m, unsigned *lds) {
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) {
        const unsigned t = (unsigned)__shfl_xor((int)m, o, 64);
        m = t > m ? t : m;
    }
    const int wave = (int)threadIdx.x >> 6;
    if ((threadIdx.x & 63) == 0) lds[wave] = m;
    __syncthreads();
    m = lds[0];
#pragma unroll
    for (int i = 1; i < FV_THREADS / 64; ++i) m = lds[i] > m ? lds[i] : m;
    return m;
}

__device__ __forceinline__ void fv_wheel_to_lds(double (*w)[3]) {
    if (threadIdx.x < FV_NCOLS * 3) {
        const int k = (int)threadIdx.x / 3, c = (int)threadIdx.x - 3 * k;
        w[k][c] = (double)fv_wheel.c[k][c] / 255.0;
    }
}

// levels 0 .. 255 of one pixel's three channels (wheel order: red, green, blue)
__device__ __forceinline__ void fv_pixel(float u, float v, float denom, const double (*wheel)[3], int *level) {
    const float un = __fdiv_rn(u, denom), vn = __fdiv_rn(v, denom);
    const float rad = fminf(__fsqrt_rn(un * un + vn * vn), 1.f);      // never above 1 in exact arithmetic
    const float a = __fdiv_rn(atan2f(-vn, -un), 3.14159274f);
    const float fk = (a + 1.f) / 2.f * (float)(FV_NCOLS - 1);
    // 0 <= fk <= 54 for every finite flow; a NaN angle takes row 0 (its levels are NaN -> 0 below)
    const int k0 = fk >= 0.f ? (fk < (float)(FV_NCOLS - 1) ? (int)floorf(fk) : FV_NCOLS - 1) : 0;
    const int k1 = k0 + 1 == FV_NCOLS ? 0 : k0 + 1;
    const double f = (double)(fk - (float)k0);
#pragma unroll
    for (int c = 0; c < 3; ++c) {
        double col = (1.0 - f) * wheel[k0][c] + f * wheel[k1][c];
        col = 1.0 - (double)rad * (1.0 - col);
        const double t = 255.0 * col;
        level[c] = t >= 0.0 ? (t < 255.0 ? (int)floor(t) : 255) : 0;
    }
}

template <typename T> __device__ __forceinline__ T fv_value(int level);
template <> __device__ __forceinline__ unsigned char fv_value<unsigned char>(int level) { return (unsigned char)level; }
template <> __device__ __forceinline__ float fv_value<float>(int level) { return __fdiv_rn((float)level, 255.f); }

template <typename T>
__device__ __forceinline__ void fv_color_item(const FvArgs &a, const float *img, T *dst, int item, float denom, const double (*wheel)[3]) {
    const int y = item / a.quads, x0 = (item - y * a.quads) * FV_VEC;
    float u[FV_VEC], v[FV_VEC];
    fv_load(a, img, y, x0, u, v);
    int level[FV_VEC][3];
#pragma unroll
    for (int e = 0; e < FV_VEC; ++e) fv_pixel(u[e], v[e], denom, wheel, level[e]);
    T *p = dst + (long)y * a.d.row + (long)x0 * a.d.col;
#pragma unroll
    for (int c = 0; c < 3; ++c) {
        T *pc = p + (long)(a.bgr ? 2 - c : c) * a.d.channel;
        if (a.dst_vec && x0 + FV_VEC <= a.w) {
            if constexpr (sizeof(T) == 1) {
                *reinterpret_cast<unsigned *>(pc) = (unsigned)level[0][c] | ((unsigned)level[1][c] << 8) | ((unsigned)level[2][c] << 16) |
                                                    ((unsigned)level[3][c] << 24);
            } else {
                st4(pc, f32x4{fv_value<float>(level[0][c]), fv_value<float>(level[1][c]), fv_value<float>(level[2][c]),
                              fv_value<float>(level[3][c])});
            }
        } else {
#pragma unroll
            for (int e = 0; e < FV_VEC; ++e)
                if (x0 + e < a.w) pc[(long)e * a.d.col] = fv_value<T>(level[e][c]);
        }
    }
}

// one launch: workgroup n takes image n whole
template <typename T>
__global__ void __launch_bounds__(FV_THREADS) fv_one_kernel(FvArgs a) {
    __shared__ double wheel[FV_NCOLS][3];
    __shared__ unsigned red[FV_THREADS / 64];
    const int n = (int)blockIdx.x, items = a.h * a.quads;
    const float *img = a.flow + fv_image_offset(a.s, n, a.group);
    fv_wheel_to_lds(wheel);
    unsigned m = 0;
    for (int item = (int)threadIdx.x; item < items; item += FV_THREADS) {
        const int y = item / a.quads, x0 = (item - y * a.quads) * FV_VEC;
        float u[FV_VEC], v[FV_VEC];
        fv_load(a, img, y, x0, u, v);
#pragma unroll
        for (int e = 0; e < FV_VEC; ++e) {
            const unsigned b = fv_rad_bits(u[e], v[e]);
            m = b > m ? b : m;
        }
    }
    m = fv_block_max(m, red);                      // (its barrier also publishes the wheel)
    const float denom = __uint_as_float(m) + 1e-5f;
    T *dst = reinterpret_cast<T *>(a.out) + fv_image_offset(a.d, n, a.group);
    for (int item = (int)threadIdx.x; item < items; item += FV_THREADS) fv_color_item<T>(a, img, dst, item, denom, wheel);
}

// two launches: workgroup (n, tile) of FV_THREADS items
__global__ void __launch_bounds__(FV_THREADS) fv_max_kernel(FvArgs a, int tiles, unsigned *__restrict__ maxima) {
    __shared__ unsigned red[FV_THREADS / 64];
    const int n = (int)blockIdx.x / tiles, tile = (int)blockIdx.x - n * tiles;
    const int item = tile * FV_THREADS + (int)threadIdx.x;
    unsigned m = 0;
    if (item < a.h * a.quads) {
        const int y = item / a.quads, x0 = (item - y * a.quads) * FV_VEC;
        float u[FV_VEC], v[FV_VEC];
        fv_load(a, a.flow + fv_image_offset(a.s, n, a.group), y, x0, u, v);
#pragma unroll
        for (int e = 0; e < FV_VEC; ++e) {
            const unsigned b = fv_rad_bits(u[e], v[e]);
            m = b > m ? b : m;
        }
    }
    m = fv_block_max(m, red);
    if (threadIdx.x == 0) atomicMax(maxima + n, m);
}

template <typename T>
__global__ void __launch_bounds__(FV_THREADS) fv_color_kernel(FvArgs a, int tiles, const unsigned *__restrict__ maxima) {
    __shared__ double wheel[FV_NCOLS][3];
    const int n = (int)blockIdx.x / tiles, tile = (int)blockIdx.x - n * tiles;
    const int item = tile * FV_THREADS + (int)threadIdx.x;
    fv_wheel_to_lds(wheel);
    __syncthreads();
    if (item >= a.h * a.quads) return;
    const float denom = __uint_as_float(maxima[n]) + 1e-5f;
    fv_color_item<T>(a, a.flow + fv_image_offset(a.s, n, a.group), reinterpret_cast<T *>(a.out) + fv_image_offset(a.d, n, a.group), item, denom,
                     wheel);
}

inline bool fv_layout_ok(const rcf_flow_layout *l) {
    return l && l->image >= 0 && l->member >= 0 && l->channel >= 0 && l->row >= 0 && l->col >= 1;
}
inline bool fv_mult4(const FvLayout &l) { return l.image % 4 == 0 && l.member % 4 == 0 && l.channel % 4 == 0 && l.row % 4 == 0; }
inline bool fv_shape_ok(int n_images, int group, int h, int w) {
    if (n_images < 1 || n_images > (1 << 20) || group < 1 || n_images % group) return false;
    if (h < 1 || w < 1 || h > (1 << 14) || w > (1 << 14)) return false;
    const long tiles = rcf_cdiv((long)h * rcf_cdiv(w, FV_VEC), FV_THREADS);
    return tiles * n_images < (1L << 31);
}

}  // namespace

extern "C" int rcf_flow_color_geometry(int which) { return which == 0 ? FV_ONE_WG_PIXELS : which == 1 ? FV_TILE_PIXELS : 0; }

extern "C" size_t rcf_flow_color_workspace_bytes(int n_images, int group, int h, int w) {
    if (!fv_shape_ok(n_images, group, h, w)) return 0;
    return (long)h * w <= FV_ONE_WG_PIXELS ? 0 : sizeof(unsigned) * (size_t)n_images;
}

extern "C" int rcf_flow_color_f32(const float *flow, const rcf_flow_layout *src, void *out, const rcf_flow_layout *dst, int out_type,
                                  int n_images, int group, int h, int w, int convert_to_bgr, float clip, void *workspace,
                                  size_t workspace_bytes, void *stream) {
    if (!fv_shape_ok(n_images, group, h, w) || (out_type != RCF_FLOW_COLOR_U8 && out_type != RCF_FLOW_COLOR_F32)) return RCF_EINVAL;
    if (!fv_layout_ok(src) || !fv_layout_ok(dst) || clip != clip) return RCF_EINVAL;
    if (!flow || !out) return RCF_EINVAL;
    const bool one = (long)h * w <= FV_ONE_WG_PIXELS;
    if (!one) {
        if (!workspace) return RCF_EINVAL;
        if (workspace_bytes < sizeof(unsigned) * (size_t)n_images || ((uintptr_t)workspace & 3)) return RCF_EWORKSPACE;
    }
    FvArgs a;
    a.flow = flow, a.out = out;
    a.s = FvLayout{src->image, src->member, src->channel, src->row, src->col};
    a.d = FvLayout{dst->image, dst->member, dst->channel, dst->row, dst->col};
    a.group = group, a.h = h, a.w = w, a.quads = rcf_cdiv(w, FV_VEC);
    a.bgr = convert_to_bgr != 0, a.clip = clip;
    a.src_vec = a.s.col == 1 && rcf_aligned16(flow) && fv_mult4(a.s);
    if (out_type == RCF_FLOW_COLOR_U8)
        a.dst_vec = a.d.col == 1 && ((uintptr_t)out & 3) == 0 && fv_mult4(a.d);
    else
        a.dst_vec = a.d.col == 1 && rcf_aligned16(out) && fv_mult4(a.d);
    hipStream_t st = rcf_stream(stream);
    if (one) {
        if (out_type == RCF_FLOW_COLOR_U8)
            hipLaunchKernelGGL(fv_one_kernel<unsigned char>, dim3(n_images), dim3(FV_THREADS), 0, st, a);
        else
            hipLaunchKernelGGL(fv_one_kernel<float>, dim3(n_images), dim3(FV_THREADS), 0, st, a);
        RCF_LAUNCH_CHECK();
        return 0;
    }
    const int tiles = rcf_cdiv((long)h * a.quads, FV_THREADS);
    unsigned *maxima = (unsigned *)workspace;
    const hipError_t e = hipMemsetAsync(maxima, 0, sizeof(unsigned) * (size_t)n_images, st);
    if (e != hipSuccess) return (int)e;
    hipLaunchKernelGGL(fv_max_kernel, dim3(tiles * n_images), dim3(FV_THREADS), 0, st, a, tiles, maxima);
    RCF_LAUNCH_CHECK();
    if (out_type == RCF_FLOW_COLOR_U8)
        hipLaunchKernelGGL(fv_color_kernel<unsigned char>, dim3(tiles * n_images), dim3(FV_THREADS), 0, st, a, tiles, maxima);
    else
        hipLaunchKernelGGL(fv_color_kernel<float>, dim3(tiles * n_images), dim3(FV_THREADS), 0, st, a, tiles, maxima);
    RCF_LAUNCH_CHECK();
    return 0;
}
