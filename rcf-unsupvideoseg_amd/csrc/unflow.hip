// unFlowLoss (models/amd/flow_loss.py, models/amd/loss_blocks.py) as fused passes with gradients to the flow.  Planar NCHW fp32.
//
// One direction of one pyramid level, with rec = flow_warp(other, flow, 'border'), x = rec occ, y = im occ:
//   photo = ( w_l1 mean_{B,3,h,w} |im - rec| occ + w_ssim mean_{B,3,h-2md,w-2md} SSIM_dist(x, y, md)
//             + w_ternary mean_{B,1,h,w} Ternary(x, y) ) / mean_{B,1,h,w} occ
// The images and the mask are constants; the gradient goes to the flow alone.  occ is the LEVEL-0 mask [B][1][H0][W0], read through
// torch's `nearest` rule (source index min(floor(dst * float(H0) / h), H0 - 1), float32 as torch computes it); H0 = h reads it as is.
//
// Forward: a workgroup owns an 8 x 32 tile, computes rec for the tile plus a halo of md, stages x and y (3 channels each) in LDS
// -- (8 + 2 md) x (32 + 2 md) x 6 floats, 12.8 KB at md = 3, rows at an odd pitch -- and every thread forms its pixel's terms out
// of LDS.  The four sums of a workgroup go in fp64 into a partials buffer, a one-workgroup finishing kernel adds them in index
// order.  Backward: x, y on a halo of 2 md, the three SSIM coefficient planes per channel on a halo of md (40 KB at md = 3), then a
// box sum out of LDS; neither rec nor d rec reaches HBM.  Every result is a gather summed in a fixed order: no atomics, the same
// bits on every call.  The sample position, the blend, the derivative of a sample by its position and the block sum are the
// ones csrc/warp.hip uses (csrc/flow_sample.h); the library is compiled without contraction.
//
// SSIM window sums are taken about the window's centre value (d = x - x_c): the variances then carry the rounding of the
// differences, not of x^2 ~ 0.25, and a constant window gives sigma = 0 exactly.
#include "flow_sample.h"

namespace {

constexpr int UF_TH = 8, UF_TW = 32, UF_MAXMD = 3;      // tile rows, tile columns (256 threads), largest SSIM half-window
constexpr float UF_C1 = 0.01f * 0.01f, UF_C2 = 0.03f * 0.03f;
constexpr float UF_GR = 0.2989f, UF_GG = 0.5870f, UF_GB = 0.1140f;

__device__ __forceinline__ int uf_near(int dst, float scale, int in) { return min((int)floorf((float)dst * scale), in - 1); }

struct UfImg {
    const float *im, *other, *flow, *occ0;      // of this image: [3][h w], [3][h w], [2][h w], [H0 W0]
    int h, w, H0, W0;
    float sy, sx;                               // float(H0) / h, float(W0) / w
};

// rec, im and occ of pixel (gy, gx) (inside the image); v[c][k]: the four tap values
__device__ __forceinline__ void uf_pixel(const UfImg &g, int gy, int gx, Taps &t, float (&v)[3][4], float (&rec)[3], float (&imv)[3],
                                         float &o) {
    const int hw = g.h * g.w, p = gy * g.w + gx;
    t = make_taps((float)gx + g.flow[p], (float)gy + g.flow[hw + p], g.w, g.h, 0);
    // taps are read at always-inside offsets: after the clip x0, y0 lie in [0, size - 1], and a tap at `size` has weight exactly 0
    // and is read at size - 1 (csrc/warp.hip's backward substitutes 0 for the value of a tap outside, so it gathers for itself)
    const int x1 = min(t.x0 + 1, g.w - 1), y1 = min(t.y0 + 1, g.h - 1);
    const int o00 = t.y0 * g.w + t.x0, o01 = t.y0 * g.w + x1, o10 = y1 * g.w + t.x0, o11 = y1 * g.w + x1;
    o = g.occ0[uf_near(gy, g.sy, g.H0) * g.W0 + uf_near(gx, g.sx, g.W0)];
    const float ex = 1.f - t.wx, ey = 1.f - t.wy;
#pragma unroll
    for (int c = 0; c < 3; ++c) {
        const float *pl = g.other + c * hw;
        v[c][0] = pl[o00];
        v[c][1] = pl[o01];
        v[c][2] = pl[o10];
        v[c][3] = pl[o11];
        imv[c] = g.im[c * hw + p];
    }
#pragma unroll
    for (int c = 0; c < 3; ++c) rec[c] = blend4(v[c][0], v[c][1], v[c][2], v[c][3], ey * ex, ey * t.wx, t.wy * ex, t.wy * t.wx);
}

// the window's means and (co)variances, sums taken about the centre values
template <int MD>
__device__ __forceinline__ void uf_window(const float *X, const float *Y, int pitch, float &mx, float &my, float &vx, float &vy,
                                          float &cxy) {
    constexpr int K = 2 * MD + 1;
    constexpr float inv = 1.f / (float)(K * K);
    const float xc = X[MD * pitch + MD], yc = Y[MD * pitch + MD];
    float s1 = 0.f, s2 = 0.f, s11 = 0.f, s22 = 0.f, s12 = 0.f;
#pragma unroll
    for (int i = 0; i < K; ++i)
#pragma unroll
        for (int j = 0; j < K; ++j) {
            const float a = X[i * pitch + j] - xc, b = Y[i * pitch + j] - yc;
            s1 += a;
            s2 += b;
            s11 += a * a;
            s22 += b * b;
            s12 += a * b;
        }
    const float ma = s1 * inv, mb = s2 * inv;
    mx = xc + ma;
    my = yc + mb;
    vx = s11 * inv - ma * ma;
    vy = s22 * inv - mb * mb;
    cxy = s12 * inv - ma * mb;
}

__device__ __forceinline__ float uf_gray(const float *X, int plane, int at) {
    return (X[at] * UF_GR + X[plane + at] * UF_GG + X[2 * plane + at] * UF_GB) * 255.f;
}

__device__ __forceinline__ UfImg uf_image(const float *im, const float *other, const float *flow, long flow_bs, const float *occ0,
                                          int b, int h, int w, int H0, int W0, float sy, float sx) {
    UfImg g;
    const long hw = (long)h * w;
    g.im = im + b * 3 * hw;
    g.other = other + b * 3 * hw;
    g.flow = flow + b * flow_bs;
    g.occ0 = occ0 + (long)b * H0 * W0;
    g.h = h; g.w = w; g.H0 = H0; g.W0 = W0; g.sy = sy; g.sx = sx;
    return g;
}

// ------------------------------------------------------------------------------------------------------- photometric forward
// partials[block][4]: sum |im - rec| occ, sum SSIM distance, sum ternary distance, sum occ
template <int MD>
__global__ void __launch_bounds__(256) uf_photo_fwd_kernel(const float *__restrict__ im, const float *__restrict__ other,
                                                           const float *__restrict__ flow, long flow_bs,
                                                           const float *__restrict__ occ0, double *__restrict__ partials, int h,
                                                           int w, int H0, int W0, float sy, float sx, int tiles_x, int tiles_y,
                                                           int do_ssim, int do_tern) {
    constexpr int TH2 = UF_TH + 2 * MD, TW2 = UF_TW + 2 * MD, P = TW2 | 1, PLANE = TH2 * P;
    __shared__ float X[3 * PLANE], Y[3 * PLANE];
    __shared__ double red[16];
    int bid = (int)blockIdx.x;
    const int txi = bid % tiles_x;
    bid /= tiles_x;
    const int tyi = bid % tiles_y, b = bid / tiles_y;
    const UfImg g = uf_image(im, other, flow, flow_bs, occ0, b, h, w, H0, W0, sy, sx);
    const int y0 = tyi * UF_TH - MD, x0 = txi * UF_TW - MD;
    double acc[4] = {0, 0, 0, 0};
    for (int idx = (int)threadIdx.x; idx < TH2 * TW2; idx += 256) {
        const int ly = idx / TW2, lx = idx - ly * TW2;
        const int gy = y0 + ly, gx = x0 + lx;
        float xv[3] = {0.f, 0.f, 0.f}, yv[3] = {0.f, 0.f, 0.f};
        if (gy >= 0 && gy < h && gx >= 0 && gx < w) {
            Taps t;
            float v[3][4], rec[3], imv[3], o;
            uf_pixel(g, gy, gx, t, v, rec, imv, o);
            float l1 = 0.f;
#pragma unroll
            for (int c = 0; c < 3; ++c) {
                xv[c] = rec[c] * o;
                yv[c] = imv[c] * o;
                l1 += fabsf(imv[c] - rec[c]) * o;
            }
            if (ly >= MD && ly < MD + UF_TH && lx >= MD && lx < MD + UF_TW) {      // the tile itself: each pixel counted once
                acc[0] += (double)l1;
                acc[3] += (double)o;
            }
        }
#pragma unroll
        for (int c = 0; c < 3; ++c) {
            X[c * PLANE + ly * P + lx] = xv[c];
            Y[c * PLANE + ly * P + lx] = yv[c];
        }
    }
    __syncthreads();
    const int tx = (int)threadIdx.x % UF_TW, ty = (int)threadIdx.x / UF_TW;
    const int gy = tyi * UF_TH + ty, gx = txi * UF_TW + tx;
    if (do_ssim && gy >= MD && gy < h - MD && gx >= MD && gx < w - MD) {
        float s = 0.f;
#pragma unroll
        for (int c = 0; c < 3; ++c) {
            float mx, my, vx, vy, cxy;
            uf_window<MD>(X + c * PLANE + ty * P + tx, Y + c * PLANE + ty * P + tx, P, mx, my, vx, vy, cxy);
            const float n = (2.f * mx * my + UF_C1) * (2.f * cxy + UF_C2);
            const float d = (mx * mx + my * my + UF_C1) * (vx + vy + UF_C2);
            s += fminf(fmaxf((1.f - n / d) * 0.5f, 0.f), 1.f);
        }
        acc[1] = (double)s;
    }
    if (do_tern && gy >= 1 && gy < h - 1 && gx >= 1 && gx < w - 1) {
        const int at = (ty + MD) * P + tx + MD;
        const float i1 = uf_gray(X, PLANE, at), i2 = uf_gray(Y, PLANE, at);
        float s = 0.f;
#pragma unroll
        for (int dy = -1; dy <= 1; ++dy)
#pragma unroll
            for (int dx = -1; dx <= 1; ++dx) {
                const float d1 = uf_gray(X, PLANE, at + dy * P + dx) - i1, d2 = uf_gray(Y, PLANE, at + dy * P + dx) - i2;
                const float u = d1 / sqrtf(0.81f + d1 * d1) - d2 / sqrtf(0.81f + d2 * d2);
                const float q = u * u;
                s += q / (0.1f + q);
            }
        acc[2] = (double)(s / 9.f);
    }
    block_sum_d<4>(acc, red);
    if (threadIdx.x < 4) partials[(long)blockIdx.x * 4 + threadIdx.x] = acc[threadIdx.x];
}

// partials [n][K] -> tot[K]: thread t adds rows t, t + 256, ... in order, then the fixed tree of block_sum_d
template <int K> __device__ __forceinline__ void uf_sum_partials(const double *__restrict__ partials, int n, double (&tot)[K], double *sh) {
#pragma unroll
    for (int k = 0; k < K; ++k) tot[k] = 0;
    for (int i = (int)threadIdx.x; i < n; i += 256)
#pragma unroll
        for (int k = 0; k < K; ++k) tot[k] += partials[(long)i * K + k];
    block_sum_d<K>(tot, sh);
}

// out[0] = the loss, out[1..3] = the three means (L1, SSIM, ternary), out[4] = the mask mean
__global__ void __launch_bounds__(256) uf_photo_finish_kernel(const double *__restrict__ partials, int n, float *__restrict__ out,
                                                              float w_l1, float w_ssim, float w_tern, double n_l1, double n_ssim,
                                                              double n_px) {
    __shared__ double red[16];
    double t[4];
    uf_sum_partials<4>(partials, n, t, red);
    if (threadIdx.x == 0) {
        const double l1 = t[0] / n_l1, ss = t[1] / n_ssim, te = t[2] / n_px, om = t[3] / n_px;
        double loss = 0;
        if (w_l1 > 0) loss += (double)w_l1 * l1;
        if (w_ssim > 0) loss += (double)w_ssim * ss;
        if (w_tern > 0) loss += (double)w_tern * te;
        out[0] = (float)(loss / om);
        out[1] = (float)l1;
        out[2] = (float)ss;
        out[3] = (float)te;
        out[4] = (float)om;
    }
}

// ------------------------------------------------------------------------------------------------------ photometric backward
// k_l1 = w_l1 / (3 B h w), k_ssim = w_ssim / (3 B (h - 2 md)(w - 2 md)), k_tern = w_ternary / (9 B h w); 0 switches a term off.
// dflow [B][2][h][w] = (dloss[0] / stats[4]) * sum_c d rec_c * d sample / d position, 0 on a clipped coordinate.
template <int MD>
__global__ void __launch_bounds__(256) uf_photo_bwd_kernel(const float *__restrict__ im, const float *__restrict__ other,
                                                           const float *__restrict__ flow, long flow_bs,
                                                           const float *__restrict__ occ0, const float *__restrict__ dloss,
                                                           const float *__restrict__ stats, float *__restrict__ dflow, int h, int w,
                                                           int H0, int W0, float sy, float sx, int tiles_x, int tiles_y, float k_l1,
                                                           float k_ssim, float k_tern) {
    constexpr int K = 2 * MD + 1;
    constexpr int TH4 = UF_TH + 4 * MD, TW4 = UF_TW + 4 * MD, P4 = TW4 | 1, PL4 = TH4 * P4;       // x, y: halo 2 md
    constexpr int TH2 = UF_TH + 2 * MD, TW2 = UF_TW + 2 * MD, P2 = TW2 | 1, PL2 = TH2 * P2;       // coefficients: halo md
    __shared__ float X[3 * PL4], Y[3 * PL4];
    __shared__ float CA[3 * PL2], CB[3 * PL2], CC[3 * PL2];
    int bid = (int)blockIdx.x;
    const int txi = bid % tiles_x;
    bid /= tiles_x;
    const int tyi = bid % tiles_y, b = bid / tiles_y;
    const UfImg g = uf_image(im, other, flow, flow_bs, occ0, b, h, w, H0, W0, sy, sx);
    const int ty0 = tyi * UF_TH, tx0 = txi * UF_TW;
    const bool ssim = k_ssim != 0.f, tern = k_tern != 0.f;

    if (ssim || tern) {
        for (int idx = (int)threadIdx.x; idx < TH4 * TW4; idx += 256) {
            const int ly = idx / TW4, lx = idx - ly * TW4;
            const int gy = ty0 - 2 * MD + ly, gx = tx0 - 2 * MD + lx;
            float xv[3] = {0.f, 0.f, 0.f}, yv[3] = {0.f, 0.f, 0.f};
            if (gy >= 0 && gy < h && gx >= 0 && gx < w) {
                Taps t;
                float v[3][4], rec[3], imv[3], o;
                uf_pixel(g, gy, gx, t, v, rec, imv, o);
#pragma unroll
                for (int c = 0; c < 3; ++c) {
                    xv[c] = rec[c] * o;
                    yv[c] = imv[c] * o;
                }
            }
#pragma unroll
            for (int c = 0; c < 3; ++c) {
                X[c * PL4 + ly * P4 + lx] = xv[c];
                Y[c * PL4 + ly * P4 + lx] = yv[c];
            }
        }
        __syncthreads();
    }
    if (ssim) {
        // window p: dist = clamp((1 - S) / 2, 0, 1), S = a1 a2 / (b1 b2);  d dist / d x_q = A + x_q B + y_q C for every q of the window
        constexpr float n = (float)(K * K);
        for (int idx = (int)threadIdx.x; idx < TH2 * TW2; idx += 256) {
            const int ly = idx / TW2, lx = idx - ly * TW2;
            const int gy = ty0 - MD + ly, gx = tx0 - MD + lx;
            const bool valid = gy >= MD && gy < h - MD && gx >= MD && gx < w - MD;
#pragma unroll
            for (int c = 0; c < 3; ++c) {
                float A = 0.f, Bc = 0.f, Cc = 0.f;
                if (valid) {
                    float mx, my, vx, vy, cxy;
                    uf_window<MD>(X + c * PL4 + ly * P4 + lx, Y + c * PL4 + ly * P4 + lx, P4, mx, my, vx, vy, cxy);
                    const float a1 = 2.f * mx * my + UF_C1, a2 = 2.f * cxy + UF_C2;
                    const float b1 = mx * mx + my * my + UF_C1, b2 = vx + vy + UF_C2;
                    const float b12 = b1 * b2;
                    const float S = a1 * a2 / b12;
                    const float dist = (1.f - S) * 0.5f;
                    if (dist > 0.f && dist < 1.f) {
                        const float wgt = -0.5f * k_ssim;
                        A = wgt * (2.f * my * (a2 - a1) / b12 - 2.f * mx * S * (1.f / b1 - 1.f / b2)) / n;
                        Bc = -2.f * wgt * S / (b2 * n);
                        Cc = 2.f * wgt * a1 / (b12 * n);
                    }
                }
                CA[c * PL2 + ly * P2 + lx] = A;
                CB[c * PL2 + ly * P2 + lx] = Bc;
                CC[c * PL2 + ly * P2 + lx] = Cc;
            }
        }
        __syncthreads();
    }
    const int tx = (int)threadIdx.x % UF_TW, ty = (int)threadIdx.x / UF_TW;
    const int gy = ty0 + ty, gx = tx0 + tx;
    if (gy >= h || gx >= w) return;
    Taps t;
    float v[3][4], rec[3], imv[3], o;
    uf_pixel(g, gy, gx, t, v, rec, imv, o);
    float drec[3] = {0.f, 0.f, 0.f};
    if (k_l1 != 0.f) {
#pragma unroll
        for (int c = 0; c < 3; ++c) {
            const float d = imv[c] - rec[c];
            drec[c] += (d > 0.f ? -1.f : (d < 0.f ? 1.f : 0.f)) * o * k_l1;
        }
    }
    if (ssim) {
        const int at4 = (ty + 2 * MD) * P4 + tx + 2 * MD;
#pragma unroll
        for (int c = 0; c < 3; ++c) {
            const float *a = CA + c * PL2 + ty * P2 + tx, *bb = CB + c * PL2 + ty * P2 + tx, *cc = CC + c * PL2 + ty * P2 + tx;
            float sa = 0.f, sb = 0.f, sc = 0.f;
#pragma unroll
            for (int i = 0; i < K; ++i)
#pragma unroll
                for (int j = 0; j < K; ++j) {
                    sa += a[i * P2 + j];
                    sb += bb[i * P2 + j];
                    sc += cc[i * P2 + j];
                }
            drec[c] += o * (sa + X[c * PL4 + at4] * sb + Y[c * PL4 + at4] * sc);
        }
    }
    if (tern) {
        // centre n pays psi(n -> q) to its neighbour q and -psi(n -> q') to itself; psi(q -> n) = -psi(n -> q), so q collects
        // ([n interior] + [q interior]) psi(n -> q) over its 8 neighbours
        const int at = (ty + 2 * MD) * P4 + tx + 2 * MD;
        const float i1 = uf_gray(X, PL4, at), i2 = uf_gray(Y, PL4, at);
        const bool vq = gy >= 1 && gy < h - 1 && gx >= 1 && gx < w - 1;
        float s = 0.f;
#pragma unroll
        for (int dy = -1; dy <= 1; ++dy)
#pragma unroll
            for (int dx = -1; dx <= 1; ++dx) {
                if (dy == 0 && dx == 0) continue;
                const int ny = gy + dy, nx = gx + dx;
                const bool vn = ny >= 1 && ny < h - 1 && nx >= 1 && nx < w - 1;
                const float cnt = (vn ? 1.f : 0.f) + (vq ? 1.f : 0.f);
                const float d1 = i1 - uf_gray(X, PL4, at + dy * P4 + dx), d2 = i2 - uf_gray(Y, PL4, at + dy * P4 + dx);
                const float r1 = 0.81f + d1 * d1, r2 = 0.81f + d2 * d2;
                const float u = d1 / sqrtf(r1) - d2 / sqrtf(r2);
                const float den = 0.1f + u * u;
                s += cnt * ((0.2f * u) / (den * den)) * (0.81f / (r1 * sqrtf(r1)));
            }
        const float gi = s * k_tern * 255.f * o;
        drec[0] += gi * UF_GR;
        drec[1] += gi * UF_GG;
        drec[2] += gi * UF_GB;
    }
    float gix = 0.f, giy = 0.f;
#pragma unroll
    for (int c = 0; c < 3; ++c) {
        float sx, sy;
        sample_dpos(v[c][0], v[c][1], v[c][2], v[c][3], t, sx, sy);
        gix += drec[c] * sx;
        giy += drec[c] * sy;
    }
    const float scale = dloss[0] / stats[4];
    const long hw = (long)h * w, p = (long)gy * w + gx;
    float *df = dflow + (long)b * 2 * hw;
    df[p] = t.gx_live ? scale * gix : 0.f;
    df[hw + p] = t.gy_live ? scale * giy : 0.f;
}

// ---------------------------------------------------------------------------------------------------------------- smoothness
// first order: loss_x = wx |dx f| / 2 over [B][2][h][w-1];  second: loss_x = wx[.., 1:] |dx dx f| over [B][2][h][w-2]; f = flow / s,
// wx = exp(-alpha mean_c |dx im|); the same along y.  out = mean(loss_x) / 2 + mean(loss_y) / 2.
__device__ __forceinline__ float uf_edge(const float *im, long hw, long a, long b, float alpha) {
    const float m = (fabsf(im[b] - im[a]) + fabsf(im[hw + b] - im[hw + a]) + fabsf(im[2 * hw + b] - im[2 * hw + a])) / 3.f;
    return expf(-m * alpha);
}
__device__ __forceinline__ float uf_sign(float v) { return v > 0.f ? 1.f : (v < 0.f ? -1.f : 0.f); }

// the difference along one axis at element j (stride st): first order f[j+1] - f[j], second (f[j+2] - f[j+1]) - (f[j+1] - f[j])
__device__ __forceinline__ float uf_diff(const float *f, long j, long st, float s, int second) {
    const float a = f[j] / s, b = f[j + st] / s;
    if (!second) return b - a;
    const float c = f[j + 2 * st] / s;
    return (c - b) - (b - a);
}

__global__ void __launch_bounds__(256) uf_smooth_fwd_kernel(const float *__restrict__ flow, long flow_bs, const float *__restrict__ im,
                                                            double *__restrict__ partials, int B, int h, int w, float alpha, float s,
                                                            int second) {
    __shared__ double red[8];
    const long hw = (long)h * w, total = (long)B * hw;
    const long step = (long)gridDim.x * 256;
    const int reach = second ? 2 : 1;
    double acc[2] = {0, 0};
    for (long i = (long)blockIdx.x * 256 + threadIdx.x; i < total; i += step) {
        const long b = i / hw, p = i - b * hw;
        const int y = (int)(p / w), x = (int)(p - (long)y * w);
        const float *f = flow + b * flow_bs, *img = im + b * 3 * hw;
        if (x + reach < w) {
            const float wg = uf_edge(img, hw, p + reach - 1, p + reach, alpha);
            const float t = fabsf(uf_diff(f, p, 1, s, second)) + fabsf(uf_diff(f + hw, p, 1, s, second));
            acc[0] += (double)(second ? wg * t : wg * t / 2.f);
        }
        if (y + reach < h) {
            const float wg = uf_edge(img, hw, p + (long)(reach - 1) * w, p + (long)reach * w, alpha);
            const float t = fabsf(uf_diff(f, p, w, s, second)) + fabsf(uf_diff(f + hw, p, w, s, second));
            acc[1] += (double)(second ? wg * t : wg * t / 2.f);
        }
    }
    block_sum_d<2>(acc, red);
    if (threadIdx.x < 2) partials[(long)blockIdx.x * 2 + threadIdx.x] = acc[threadIdx.x];
}

__global__ void __launch_bounds__(256) uf_smooth_finish_kernel(const double *__restrict__ partials, int n, float *__restrict__ out,
                                                               double n_x, double n_y) {
    __shared__ double red[8];
    double t[2];
    uf_sum_partials<2>(partials, n, t, red);
    if (threadIdx.x == 0) out[0] = (float)(t[0] / n_x / 2.0 + t[1] / n_y / 2.0);      // an empty axis: 0 / 0, the reference's NaN
}

// kx, ky: everything constant of a term's weight: 1 / (2 n_x s) (second order), 1 / (4 n_x s) (first order); 0 for an empty axis
__global__ void __launch_bounds__(256) uf_smooth_bwd_kernel(const float *__restrict__ flow, long flow_bs, const float *__restrict__ im,
                                                            const float *__restrict__ dloss, float *__restrict__ dflow, int B, int h,
                                                            int w, float alpha, float s, int second, float kx, float ky) {
    const long hw = (long)h * w, total = (long)B * hw;
    const long step = (long)gridDim.x * 256;
    const int reach = second ? 2 : 1;
    const float up = dloss[0];
    for (long i = (long)blockIdx.x * 256 + threadIdx.x; i < total; i += step) {
        const long b = i / hw, p = i - b * hw;
        const int y = (int)(p / w), x = (int)(p - (long)y * w);
        const float *f = flow + b * flow_bs, *img = im + b * 3 * hw;
        float g0x = 0.f, g1x = 0.f, g0y = 0.f, g1y = 0.f;
        // the difference that starts at j = x - k holds f[x] with coefficient: first order (k = 0: -1, k = 1: +1), second (+1, -2, +1)
#pragma unroll
        for (int k = 0; k <= 2; ++k) {
            if (k > reach) continue;
            const float coef = second ? (k == 1 ? -2.f : 1.f) : (k == 0 ? -1.f : 1.f);
            if (x - k >= 0 && x - k + reach < w) {
                const long j = p - k;
                const float wg = coef * uf_edge(img, hw, j + reach - 1, j + reach, alpha);
                g0x += wg * uf_sign(uf_diff(f, j, 1, s, second));
                g1x += wg * uf_sign(uf_diff(f + hw, j, 1, s, second));
            }
            if (y - k >= 0 && y - k + reach < h) {
                const long j = p - (long)k * w;
                const float wg = coef * uf_edge(img, hw, j + (long)(reach - 1) * w, j + (long)reach * w, alpha);
                g0y += wg * uf_sign(uf_diff(f, j, w, s, second));
                g1y += wg * uf_sign(uf_diff(f + hw, j, w, s, second));
            }
        }
        float *df = dflow + b * 2 * hw;
        df[p] = up * (g0x * kx + g0y * ky);
        df[hw + p] = up * (g1x * kx + g1y * ky);
    }
}

// -------------------------------------------------------------------------------------------------------------- area pyramid
// adaptive average of [B][3][H][W] (batch stride x_bs) -> [B][3][h][w]: window rows floor(i H / h) .. ceil((i + 1) H / h)
__global__ void __launch_bounds__(256) uf_area_kernel(const float *__restrict__ x, long x_bs, float *__restrict__ out, int B, int H,
                                                      int W, int h, int w) {
    const long total = (long)B * 3 * h * w;
    const long step = (long)gridDim.x * 256;
    for (long i = (long)blockIdx.x * 256 + threadIdx.x; i < total; i += step) {
        const int ox = (int)(i % w);
        long r = i / w;
        const int oy = (int)(r % h);
        r /= h;
        const int c = (int)(r % 3), b = (int)(r / 3);
        const int ys = (int)(((long)oy * H) / h), ye = (int)((((long)oy + 1) * H + h - 1) / h);
        const int xs = (int)(((long)ox * W) / w), xe = (int)((((long)ox + 1) * W + w - 1) / w);
        const float *pl = x + b * x_bs + (long)c * H * W;
        float sum = 0.f;
        for (int yy = ys; yy < ye; ++yy)
            for (int xx = xs; xx < xe; ++xx) sum += pl[(long)yy * W + xx];
        out[i] = sum / (float)((ye - ys) * (xe - xs));
    }
}

// ---------------------------------------------------------------------------------------------------------------- host side
inline bool uf_shape_ok(int B, int h, int w) {
    if (B <= 0 || h <= 0 || w <= 0) return false;
    if ((long)h * w >= (1L << 30)) return false;                   // a plane offset is held in an int
    return (long)B * h * w < (1L << 40);
}

inline bool uf_photo_ok(int B, int h, int w, int H0, int W0, int md) {
    if (!uf_shape_ok(B, h, w) || H0 <= 0 || W0 <= 0 || (long)H0 * W0 >= (1L << 30)) return false;
    if (md < 1 || md > UF_MAXMD) return false;
    if (h < 2 * md + 1 || w < 2 * md + 1) return false;
    return (long)B * rcf_cdiv(h, UF_TH) * rcf_cdiv(w, UF_TW) < (1L << 31);
}

inline int uf_stream_blocks(long total) {
    const long b = (total + 255) / 256;
    return (int)(b < 1 ? 1 : (b > 1024 ? 1024 : b));
}

}  // namespace

extern "C" int rcf_unflow_geometry(int which) {
    return which == 0 ? UF_TH : which == 1 ? UF_TW : which == 2 ? UF_MAXMD : 0;
}

extern "C" long rcf_unflow_photo_partials(int B, int h, int w) {
    if (!uf_shape_ok(B, h, w)) return 0;
    return 4L * B * rcf_cdiv(h, UF_TH) * rcf_cdiv(w, UF_TW);
}

extern "C" int rcf_unflow_photo_fwd_f32(const float *im, const float *other, const float *flow, long flow_bstride, const float *occ0,
                                        int H0, int W0, int md, float w_l1, float w_ssim, float w_ternary, float *out,
                                        double *partials, long partials_len, int B, int h, int w, void *stream) {
    if (!uf_photo_ok(B, h, w, H0, W0, md) || flow_bstride < 2L * h * w) return RCF_EINVAL;
    if (!im || !other || !flow || !occ0 || !out || !partials) return RCF_EINVAL;
    if (partials_len < rcf_unflow_photo_partials(B, h, w)) return RCF_EWORKSPACE;
    const int tx = rcf_cdiv(w, UF_TW), ty = rcf_cdiv(h, UF_TH);
    const long nb = (long)B * tx * ty;
    const float sy = (float)H0 / (float)h, sx = (float)W0 / (float)w;
    hipStream_t st = rcf_stream(stream);
    const int ds = w_ssim > 0.f, dt = w_ternary > 0.f;
#define UF_GO(m)                                                                                                                \
    hipLaunchKernelGGL((uf_photo_fwd_kernel<m>), dim3((unsigned)nb), dim3(256), 0, st, im, other, flow, flow_bstride, occ0, partials, \
                       h, w, H0, W0, sy, sx, tx, ty, ds, dt)
    switch (md) {
    case 1: UF_GO(1); break;
    case 2: UF_GO(2); break;
    default: UF_GO(3); break;
    }
#undef UF_GO
    RCF_LAUNCH_CHECK();
    const double npx = (double)B * h * w;
    hipLaunchKernelGGL(uf_photo_finish_kernel, dim3(1), dim3(256), 0, st, (const double *)partials, (int)nb, out, w_l1, w_ssim,
                       w_ternary, 3.0 * npx, 3.0 * B * (double)(h - 2 * md) * (double)(w - 2 * md), npx);
    RCF_LAUNCH_CHECK();
    return 0;
}

extern "C" int rcf_unflow_photo_bwd_f32(const float *im, const float *other, const float *flow, long flow_bstride, const float *occ0,
                                        int H0, int W0, int md, float w_l1, float w_ssim, float w_ternary, const float *dloss,
                                        const float *stats, float *dflow, int B, int h, int w, void *stream) {
    if (!uf_photo_ok(B, h, w, H0, W0, md) || flow_bstride < 2L * h * w) return RCF_EINVAL;
    if (!im || !other || !flow || !occ0 || !dloss || !stats || !dflow) return RCF_EINVAL;
    const int tx = rcf_cdiv(w, UF_TW), ty = rcf_cdiv(h, UF_TH);
    const long nb = (long)B * tx * ty;
    const float sy = (float)H0 / (float)h, sx = (float)W0 / (float)w;
    const double npx = (double)B * h * w;
    const float k1 = w_l1 > 0.f ? (float)((double)w_l1 / (3.0 * npx)) : 0.f;
    const float ks = w_ssim > 0.f ? (float)((double)w_ssim / (3.0 * B * (double)(h - 2 * md) * (double)(w - 2 * md))) : 0.f;
    const float kt = w_ternary > 0.f ? (float)((double)w_ternary / (9.0 * npx)) : 0.f;
    hipStream_t st = rcf_stream(stream);
#define UF_GO(m)                                                                                                                \
    hipLaunchKernelGGL((uf_photo_bwd_kernel<m>), dim3((unsigned)nb), dim3(256), 0, st, im, other, flow, flow_bstride, occ0, dloss,   \
                       stats, dflow, h, w, H0, W0, sy, sx, tx, ty, k1, ks, kt)
    switch (md) {
    case 1: UF_GO(1); break;
    case 2: UF_GO(2); break;
    default: UF_GO(3); break;
    }
#undef UF_GO
    RCF_LAUNCH_CHECK();
    return 0;
}

// partials: 2 * 1024 doubles
extern "C" int rcf_unflow_smooth_fwd_f32(const float *flow, long flow_bstride, const float *im, float alpha, float s, int second,
                                         float *out, double *partials, int B, int h, int w, void *stream) {
    if (!uf_shape_ok(B, h, w) || flow_bstride < 2L * h * w || (second != 0 && second != 1)) return RCF_EINVAL;
    if (!flow || !im || !out || !partials) return RCF_EINVAL;
    const int nb = uf_stream_blocks((long)B * h * w);
    hipStream_t st = rcf_stream(stream);
    hipLaunchKernelGGL(uf_smooth_fwd_kernel, dim3(nb), dim3(256), 0, st, flow, flow_bstride, im, partials, B, h, w, alpha, s, second);
    RCF_LAUNCH_CHECK();
    const int r = second ? 2 : 1;
    const double nx = 2.0 * B * h * (double)(w > r ? w - r : 0), ny = 2.0 * B * (double)(h > r ? h - r : 0) * w;
    hipLaunchKernelGGL(uf_smooth_finish_kernel, dim3(1), dim3(256), 0, st, (const double *)partials, nb, out, nx, ny);
    RCF_LAUNCH_CHECK();
    return 0;
}

extern "C" int rcf_unflow_smooth_bwd_f32(const float *flow, long flow_bstride, const float *im, float alpha, float s, int second,
                                         const float *dloss, float *dflow, int B, int h, int w, void *stream) {
    if (!uf_shape_ok(B, h, w) || flow_bstride < 2L * h * w || (second != 0 && second != 1)) return RCF_EINVAL;
    if (!flow || !im || !dloss || !dflow) return RCF_EINVAL;
    const int r = second ? 2 : 1;
    const double nx = 2.0 * B * h * (double)(w > r ? w - r : 0), ny = 2.0 * B * (double)(h > r ? h - r : 0) * w;
    const double c = (second ? 2.0 : 4.0) * (double)s;
    const float kx = nx > 0 ? (float)(1.0 / (c * nx)) : 0.f, ky = ny > 0 ? (float)(1.0 / (c * ny)) : 0.f;
    hipLaunchKernelGGL(uf_smooth_bwd_kernel, dim3(uf_stream_blocks((long)B * h * w)), dim3(256), 0, rcf_stream(stream), flow,
                       flow_bstride, im, dloss, dflow, B, h, w, alpha, s, second, kx, ky);
    RCF_LAUNCH_CHECK();
    return 0;
}

extern "C" int rcf_unflow_area_f32(const float *x, long x_bstride, float *out, int B, int H, int W, int h, int w, void *stream) {
    if (!uf_shape_ok(B, H, W) || !uf_shape_ok(B, h, w) || x_bstride < 3L * H * W) return RCF_EINVAL;
    if (!x || !out) return RCF_EINVAL;
    hipLaunchKernelGGL(uf_area_kernel, dim3(uf_stream_blocks(3L * B * h * w)), dim3(256), 0, rcf_stream(stream), x, x_bstride, out, B, H,
                       W, h, w);
    RCF_LAUNCH_CHECK();
    return 0;
}
