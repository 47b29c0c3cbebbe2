/* rcf_hip.h -- C ABI of librcf_hip.so: the MI355X (gfx950) kernels of RCF's training hot path.
 *
 * Conventions
 *   - plain C: device pointers + sizes, no torch types.  `stream` is a hipStream_t passed as void*.
 *   - every entry point returns 0 on success, a positive hipError_t on a HIP failure, or a
 *     negative RCF_E* code on a bad argument.  Nothing calls exit() (the reference's
 *     tools/torchCRF/src/permutohedral_gpu.cu:44-53 kills the process on a CUDA error).
 *   - activations are NHWC fp32 ("pixel-major": element (n,y,x,c) at ((n*H+y)*W+x)*pitch + c,
 *     pitch >= C so a tensor may be a channel slice of a wider buffer); conv weights are
 *     [Cout][R][S][Cin] (= a torch OIHW tensor in channels_last memory format).
 *   - nothing allocates: scratch is passed in, sized by the matching *_workspace_bytes().
 *
 * Each group cites the reference interface it stands in for (paths under the reference repo).
 */
#ifndef RCF_HIP_H
#define RCF_HIP_H
#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define RCF_EINVAL (-1)   /* bad shape / null pointer / unsupported size */
#define RCF_EWORKSPACE (-2) /* workspace too small */

/* storage type codes of the mixed-precision (`*_mp`, `*_bf16`) entry points: activations and activation gradients may
 * be held as bf16 between layers (BASELINE configs[2]: bf16 forward / fp32 gradients); every kernel computes in fp32.
 * Pitches are in ELEMENTS of the tensor's own type. */
#define RCF_F32 0
#define RCF_BF16 1

/* library identity: "rcf_hip <version> gfx950" */
const char *rcf_version(void);

/* ---- convolution as implicit GEMM on fp32 MFMA (v_mfma_f32_32x32x2_f32) ------------------------
 * Replaces torch.nn.Conv2d / cuDNN for every conv on the path: models/resnet.py:164-203,565-572,
 * models/res_layer.py:54-60, mmcv ConvModule in models/fcn_head.py:107-130, conv_seg :100-101,
 * flow_feat_before_agg models/flow_aggregation_head_with_residual.py:84-93.
 * Requirements: Cin % 4 == 0 (3-channel / 2-channel inputs are zero-padded to 4 by the caller),
 * pitches % 4 == 0, pointers 16-byte aligned.  Square kernels/strides/dilations/pads (all the
 * path uses).  act: 0 none, 1 LeakyReLU(slope).  bias may be NULL.  beta: 0 overwrite, 1 accumulate. */
typedef struct {
    int N, H, W, Cin;        /* input  [N,H,W,Cin], pixel pitch x_pitch */
    int Ho, Wo, Cout;        /* output [N,Ho,Wo,Cout], pixel pitch y_pitch */
    int R, S, stride, pad, dil;
    int x_pitch, y_pitch;
    /* Optional operand ranges: device scalars holding max |value| of x / w / dy as raw fp32 bits (rcf_absmax_f32);
     * NULL = unknown.  When the two a launch contracts are known (fwd: x, w; dgrad: dy, w; wgrad: x, dy) the
     * fp16-pair kernels run -- operands scaled by powers of two into fp16's range, split into 2 x fp16, 3 partial
     * products on the matrix cores (fp32-level error, see csrc/igemm_conv.hip) -- otherwise the bf16-triple kernels
     * (6 partial products).  A stale range that is too SMALL for its tensor overflows fp16: ranges must be fresh. */
    const unsigned *amax_x, *amax_w, *amax_dy;
    /* Optional, forward launches of the fp16-pair kernels: w already split by rcf_conv_weight_pairs_f32 with the
     * range amax_w points to (the kernel then reads the two fp16 planes instead of splitting w in every row tile) */
    const void *w_pairs;
    /* Optional, data-gradient launches: the transposed weight operand prepared ONCE per weight update instead of per
     * launch -- fp32 entry points: rcf_conv_weight_pairs_t_f32 (fp16 planes of the transposed weights, with amax_w);
     * bf16 entry points: rcf_conv_weight_bf16(..., transpose = 1).  The workspace of the launch may then be NULL. */
    const void *w_pairs_t;
    /* Optional, preferred over w_pairs / w_pairs_t: rcf_conv_weight_pairs2_f32 buffers (transpose 0 / 1) holding the split
     * weights in BOTH reading orders; the wide, deep convs then run on the persistent LDS-DMA kernel (conv_h2p_kernel,
     * csrc/igemm_h2p.inc), the others on the kernels that read w_pairs / w_pairs_t.  Results are identical. */
    const void *w_pairs2, *w_pairs2_t;
    /* Optional: a zeroed device scalar that receives (atomicMax) the raw bits of max |value| of the tensor the launch WRITES
     * (forward: y; data gradient: dx, after the accumulation when beta = 1) -- the next consumer's operand range without a pass
     * over the tensor.  Exact only for a launch that writes the whole tensor (no region). */
    unsigned *amax_y;
    /* RCF_CONV_* bits below; 0 = the library's own choices.  Per call, not process state: two host threads may launch with
     * different flags at the same time. */
    unsigned flags;
    /* sizeof(rcf_conv_shape) as the CALLER compiled it.  Every entry point that takes the struct refuses (RCF_EINVAL) a size
     * other than its own: a caller built against an older, shorter header cannot make the library read past its struct. */
    unsigned struct_bytes;
} rcf_conv_shape;

/* weight gradient on 128 x 256 tiles (two workgroups per CU) even where the 256 x 256 tile (one workgroup per CU, 1.02 - 1.08 x
 * alone on the chip) applies: for a launch that shares the chip with an HBM-bound kernel on another stream, whose workgroups
 * need slots on the CUs (the late weight-gradient schedule of the training step) */
#define RCF_CONV_WGRAD_TILE_128 0x1u
/* Pre-split activation operands ("pair planes").  A tensor [N,H,W,C] (C % 16 == 0, contiguous) is stored as
 * [pixel][h: C fp16 | m: C fp16] -- x * 2^k = h + m, the byte size and pixel pitch of the fp32 tensor it replaces -- with
 * k = 14 - floor(log2(bound)) from the range scalar of the operand (amax_x / amax_dy), which for such a tensor is an UPPER BOUND
 * its producer knew before writing it (rcf_bn_apply_mp / rcf_bn_bwd_apply_mp with RCF_BN_*_PLANES emit them).  The conv kernels
 * then take both operands by LDS-DMA with no split of their own (csrc/igemm_h2d.inc; weights: rcf_conv_weight_pairs2_f32).
 *   X_PLANES:  `x` of a forward / weight-gradient launch is in that format;   DY_PLANES: `dy` of a data- / weight-gradient launch.
 * Needs the matching operand ranges and w_pairs2 / w_pairs2_t; RCF_EINVAL for shapes the plane kernels do not take. */
#define RCF_CONV_X_PLANES 0x2u
#define RCF_CONV_DY_PLANES 0x4u
/* A/B and test switches (results are bit-identical, or identical up to the re-association of fp32 sums, in every setting):
 *   H2P_NEVER / H2P_ALWAYS   the persistent LDS-DMA kernel (conv_h2p_kernel) never / whenever the shape is eligible (built-in
 *                            rule: the deep 3x3 layers: K >= 2304, >= 32768 rows, <= 2 column tiles per 2304 of K)
 *   NO_WGRAD_XCD             weight-gradient workgroups in plain grid order instead of XCD-aware (an XCD's workgroups share
 *                            their pixel range)
 *   NO_COLMAP                forward / data-gradient grids always as row bands per XCD (default: convs whose weight operand
 *                            exceeds the XCDs' L2 many times over give every XCD its own column tiles)
 *   KORDER_NATURAL           K runs tap-outer (the weight's memory order) instead of (channel chunk, tap, channel in chunk) on
 *                            the 3x3 layers with >= 256 channels per tap.  The derived weight operands are written in the
 *                            order the kernels walk: pass the same flag to the rcf_conv_weight_* / rcf_conv_weights_prepare_*
 *                            call that builds them.
 *   FP32_MFMA(v)             the exact fp32 matrix-core kernels (v_mfma_f32_32x32x2_f32) with tuning variant v = 0..3 (bit 0:
 *                            K-step 32, bit 1: row-major LDS tiles) instead of the fp16-pair / bf16-triple kernels; no regions,
 *                            no fused statistics on this path */
#define RCF_CONV_H2P_NEVER 0x8u
#define RCF_CONV_H2P_ALWAYS 0x10u
#define RCF_CONV_NO_WGRAD_XCD 0x20u
#define RCF_CONV_NO_COLMAP 0x40u
#define RCF_CONV_KORDER_NATURAL 0x80u
/*   NO_TAP_SKIP              the forward / data-gradient tile kernel walks every K-step and a frame region's pixels row-major
 *                            strip by strip (default, on frame regions and with a source frame: a tile drops the K-steps of
 *                            taps that none of its rows can read -- outside the image, or off a data gradient's source frame --
 *                            and the frame is walked by depth so that whole tiles share such taps; csrc/region_order.h).  The
 *                            dropped terms are exact zeros: bit-identical. */
#define RCF_CONV_NO_TAP_SKIP 0x400u
/* 1x1 convs with 4 / 8 / 16 output channels on 64 .. 512 input channels (the decode heads' classifiers) run as streaming fp32
 * passes (csrc/thin.hip) instead of GEMM tiles with a handful of live columns; this bit keeps them on the GEMM kernels (A/B, tests) */
#define RCF_CONV_NO_THIN 0x100u
/* the forward / data-gradient tile kernels write their output with non-temporal (streaming) stores: the tile's 64 KB of output
 * does not stay in the XCD's 4 MB L2, where -- with 64 tiles in flight per XCD -- it evicts the weights and the activation rows
 * the neighbouring column tiles are still reading (tools/lab/gemm_lab, profiles/r06_gemm_lab_nt_stores.txt).  Results are
 * bit-identical; a per-call choice (rcf_amd.layers decides per layer: SCHED.nt_stores). */
#define RCF_CONV_NT_STORES 0x200u
#define RCF_CONV_FP32_MFMA(v) ((((unsigned)(v) & 3u) + 1u) << 12)

/* planes (rcf_conv_weight_pairs_bytes): fp16 h and m of w * 2^k, k from *amax_w, in the kernel's reading order
 * [K/16][Cout][4][h0 h1 h2 h3 m0 m1 m2 m3] with K = R*S*Cin padded to a multiple of 16 */
size_t rcf_conv_weight_pairs_bytes(int Cout, int Cin, int R, int S);
int rcf_conv_weight_pairs_f32(const float *w, int Cout, int Cin, int R, int S, const unsigned *amax_w, void *planes,
                              unsigned flags, void *stream);

size_t rcf_conv_weight_pairs2_bytes(int Cout, int Cin, int R, int S, int transpose);
int rcf_conv_weight_pairs2_f32(const float *w, int Cout, int Cin, int R, int S, int transpose, const unsigned *amax_w,
                               void *planes, unsigned flags, void *stream);
/* Batched weight preparation: the derived operands of EVERY conv weight of a model in three (fp16 pairs: ranges, forward
 * buffers, transposed buffers) or two (bf16: forward, transposed) launches instead of one per weight and layout -- they are
 * rebuilt after every optimizer step.  tab_*: device arrays of n entries {const float *w; void *out; unsigned *amax; int Cout,
 * Cin, RS, first_block, nblocks, flags; int pad[2]} (56 bytes; csrc/rcf_common.h rcf_wprep_entry) -- block b of a launch
 * serves the entry with first_block <= b < first_block + nblocks; flags bit 0 = also write the plane-separated half
 * (rcf_conv_pairs2_useful).  Outputs are byte-identical to rcf_absmax_f32 / rcf_conv_weight_pairs2_f32 / rcf_conv_weight_bf16. */
int rcf_conv_pairs2_useful(int Cout, int Cin, int R, int S, int transpose);
int rcf_conv_weights_prepare_f32(const void *tab_absmax, int blocks_absmax, const void *tab_pairs, int blocks_pairs,
                                 const void *tab_pairs_t, int blocks_pairs_t, int n, unsigned *amax_base, unsigned flags,
                                 void *stream);
int rcf_conv_weights_prepare_bf16(const void *tab_fwd, int blocks_fwd, const void *tab_t, int blocks_t, int n, unsigned flags,
                                  void *stream);

/* amax[0] = max(amax[0], bits(max |x|)) over [rows][C] (row pitch `pitch`); the caller zeroes amax[0] first */
int rcf_absmax_f32(const float *x, long rows, int C, int pitch, unsigned *amax, void *stream);

int rcf_conv2d_fwd_f32(const float *x, const float *w, const float *bias, float *y, const rcf_conv_shape *s,
                       int act, float slope, int beta, void *stream);
/* The same operators restricted to a rectangle of pixels (all channels): `region` is in OUTPUT coordinates for
 * fwd (only those pixels of y are written) and wgrad (only those pixels of dy/x-patches contribute), in INPUT
 * coordinates for dgrad (only those pixels of dx are written).  NULL = the whole tensor.  Used to evaluate
 * conv(bilinear_2x(x)) as bilinear_2x(conv_half_dilation(x)) in the interior and directly on the border band
 * (models/fcn_head.py:211-218 with input_transform='resize_concat'). */
typedef struct {
    int y0, x0, h, w;     /* rectangle */
    int band;             /* 0: the whole rectangle; t > 0: only its border frame of thickness t (2t < h, w) */
} rcf_conv_region;
/* What a conv launch with this shape, these operand pointers (which of them are NULL: none is read) and these flags will run: the
 * library's own launch plan, the one value its entry points consume.  direction: 0 forward, 1 data gradient, 2 weight gradient;
 * storage: RCF_F32 (rcf_conv2d_*_f32) or RCF_BF16 (rcf_conv2d_*_bf16).  Returns 0, or the status with which the launch itself is
 * refused.  A pure function of its arguments: nothing is launched, no state is read.  It answers for the GEMM kernels; the thin
 * 1x1 convs (<= 16 output channels) that the fp32 entry points hand to their streaming passes are not marked.
 *   kernel (forward / data gradient)          kernel (weight gradient)
 *   0 RCF_KERNEL_MFMA  igemm_conv_kernel        16 RCF_KERNEL_WGRAD_MFMA      igemm_wgrad_kernel (fp32 MFMA)
 *   1 RCF_KERNEL_TILE  igemm_conv_x3_kernel     17 RCF_KERNEL_WGRAD_X3        igemm_wgrad_x3_kernel
 *   2 RCF_KERNEL_H2P   conv_h2p_kernel          18 RCF_KERNEL_WGRAD_X3_WIDE   igemm_wgrad_x3_wide_kernel
 *   3 RCF_KERNEL_H2D   conv_h2d_kernel          19 RCF_KERNEL_WGRAD_H2T       igemm_wgrad_h2t_kernel
 *   4 RCF_KERNEL_BF16  conv_bf16_kernel         20 RCF_KERNEL_WGRAD_H2D       igemm_wgrad_h2d_kernel (x and dy as pair planes)
 *                                               21 RCF_KERNEL_WGRAD_BF16      wgrad_bf16_kernel
 *                                               22 RCF_KERNEL_WGRAD_BF16_DMA  wgrad_bf16_dma_kernel
 * tile_rows x tile_cols: the output tile of one workgroup (conv_h2p_kernel: the 32-row blocks it walks); splitk: workgroups that
 * share one tile of a weight gradient (1 otherwise). */
#define RCF_KERNEL_MFMA 0
#define RCF_KERNEL_TILE 1
#define RCF_KERNEL_H2P 2
#define RCF_KERNEL_H2D 3
#define RCF_KERNEL_BF16 4
#define RCF_KERNEL_WGRAD_MFMA 16
#define RCF_KERNEL_WGRAD_X3 17
#define RCF_KERNEL_WGRAD_X3_WIDE 18
#define RCF_KERNEL_WGRAD_H2T 19
#define RCF_KERNEL_WGRAD_H2D 20
#define RCF_KERNEL_WGRAD_BF16 21
#define RCF_KERNEL_WGRAD_BF16_DMA 22
typedef struct { int kernel, tile_rows, tile_cols, splitk; } rcf_conv_plan;
int rcf_conv_plan_of(const rcf_conv_shape *s, const rcf_conv_region *region, int direction /* 0 fwd, 1 dgrad, 2 wgrad */,
                     int storage /* RCF_F32, RCF_BF16 */, rcf_conv_plan *out);
/* rcf_conv_plan_of(s, region, dgrad ? 1 : 0, RCF_F32).kernel, or its status where that launch is refused; RCF_EWORKSPACE for a data
 * gradient whose weights are not prepared (it needs a workspace, and this query has none to offer) */
int rcf_conv_kernel_of(const rcf_conv_shape *s, const rcf_conv_region *region, int dgrad);
int rcf_conv2d_fwd_region_f32(const float *x, const float *w, const float *bias, float *y, const rcf_conv_shape *s,
                              const rcf_conv_region *region, int act, float slope, int beta, void *stream);
/* y = conv(x, w) (no bias, whole tensor) and, from the same kernel's epilogue, the batch-norm statistics of y:
 * sums[2*Cout] (doubles, [sum | sumsq], the layout of rcf_bn_stats_f32; a lane's <= 64 values of a column are added
 * in fp32, everything above that in fp64) -- the conv -> (Sync)BatchNorm pairs of
 * models/resnet.py:268-300 and mmcv ConvModule without the statistics pass re-reading y.  Split-bf16 kernels only
 * (RCF_EINVAL otherwise: the caller then runs rcf_bn_stats_f32). */
size_t rcf_conv2d_fwd_stats_workspace_bytes(const rcf_conv_shape *s);
/* the transposed ([Cin][R][S][Cout], K padded to whole K-steps) fp16-pair planes the data gradient contracts against;
 * rcf_conv2d_dgrad_workspace_bytes(s) bytes */
int rcf_conv_weight_pairs_t_f32(const float *w, int Cout, int Cin, int R, int S, const unsigned *amax_w, void *planes,
                                unsigned flags, void *stream);
int rcf_conv2d_fwd_stats_f32(const float *x, const float *w, float *y, const rcf_conv_shape *s, double *sums,
                             void *workspace, size_t workspace_bytes, void *stream);
/* What a training-mode batch norm derives from its statistics (the per-channel constants of the normalisation, the
 * running statistics with momentum, torch's num_batches_tracked): handed to a statistics-producing entry point, the
 * final reduction kernel writes these too and no separate finalize launch is needed.  All pointers are device memory;
 * running_mean / running_var / num_batches_tracked may be NULL. */
typedef struct rcf_bn_finalize {
    double count;                 /* rows the statistics cover (N*H*W) */
    float eps, momentum;
    float *mean, *invstd;         /* out [C] */
    float *running_mean, *running_var;
    long long *num_batches_tracked;
} rcf_bn_finalize;
/* rcf_conv2d_fwd_stats_f32 / the statistics form of rcf_conv2d_fwd_bf16 with the batch norm finalized by the same
 * reduction launch (fin != NULL; sums may then be NULL).  fin == NULL: as the plain entry points. */
int rcf_conv2d_fwd_bnstats_f32(const float *x, const float *w, float *y, const rcf_conv_shape *s, double *sums,
                               const rcf_bn_finalize *fin, void *workspace, size_t workspace_bytes, void *stream);
int rcf_conv2d_fwd_bnstats_bf16(const void *x, const void *w_bf16, void *y, int ydt, const rcf_conv_shape *s, double *sums,
                                const rcf_bn_finalize *fin, void *workspace, size_t workspace_bytes, void *stream);
/* out[i] = sum_k partial[k][i], k < chunks, i < n, in a fixed order; scratch (64 * n doubles, may be NULL) lets a
 * long list of partial rows be summed in two levels */
int rcf_sum_partials_f64(const double *partial, int chunks, int n, double *out, double *scratch, void *stream);
/* dx[N,H,W,Cin] (pitch x_pitch) (+)= conv_transpose(dy[N,Ho,Wo,Cout] (pitch y_pitch), w).
 * `workspace` (rcf_conv2d_dgrad_workspace_bytes) holds the transposed weights [Cin][R][S][Cout] the
 * split-bf16 kernels contract against. */
size_t rcf_conv2d_dgrad_workspace_bytes(const rcf_conv_shape *s);
int rcf_conv2d_dgrad_f32(const float *dy, const float *w, float *dx, const rcf_conv_shape *s, int beta,
                         void *workspace, size_t workspace_bytes, void *stream);
int rcf_conv2d_dgrad_region_f32(const float *dy, const float *w, float *dx, const rcf_conv_shape *s,
                                const rcf_conv_region *region, int beta, void *workspace, size_t workspace_bytes,
                                void *stream);
/* The same with a source frame: dy_band > 0 takes dy as ZERO off the border frame of that thickness of its [Ho, Wo] grid and does
 * not read it there (the contract of the resize kernels' `frame`): the caller passes the whole gradient instead of a copy with a
 * zeroed interior, and tiles whose taps all fall off the frame skip them.  Stride 1, at most 32 taps, no DY_PLANES. */
int rcf_conv2d_dgrad_region_band_f32(const float *dy, const float *w, float *dx, const rcf_conv_shape *s,
                                     const rcf_conv_region *region, int dy_band, int beta, void *workspace,
                                     size_t workspace_bytes, void *stream);
/* The data gradient of a conv whose INPUT is the output of a training-mode batch norm + ReLU (the bottlenecks' bn1 -> conv2,
 * bn2 -> conv3, bn3 + identity -> the next block's conv1; models/resnet.py:268-302), and, from the same kernel's epilogue, the
 * two sums that norm's backward needs: sums2[2*Cin] = [sum g | sum g * xhat] with g = dx masked by the norm's ReLU sign bits
 * (dx after the accumulation when beta = 1: the call must be the LAST writer of dx) and xhat = (x - mean) * invstd of the norm's
 * input x -- what rcf_bn_bwd_reduce_mp would read dx and x back for.  A lane's <= 64 values of a column are added in fp32,
 * everything above in fp64, in a fixed order.  rcf_conv2d_dgrad_bnsums_ok(s): 1 when the launch this shape takes has that epilogue
 * (fp16-pair kernels with prepared weights -- w_pairs_t / w_pairs2_t and both ranges --, Cin = 64, 128 or a multiple of 256);
 * otherwise the entry point returns RCF_EINVAL before launching anything and the caller runs the two passes. */
typedef struct rcf_bn_bwd_in {
    const float *x;                 /* the norm's input [N*H*W][x_pitch] */
    int x_pitch;
    const unsigned char *relu_mask; /* [N*H*W][Cin/4] as rcf_bn_apply_mp writes it */
    const float *mean, *invstd;     /* [Cin] */
} rcf_bn_bwd_in;
int rcf_conv2d_dgrad_bnsums_ok(const rcf_conv_shape *s);
size_t rcf_conv2d_dgrad_bnsums_workspace_bytes(const rcf_conv_shape *s);
int rcf_conv2d_dgrad_bnsums_f32(const float *dy, const float *w, float *dx, const rcf_conv_shape *s, int beta,
                                const rcf_bn_bwd_in *bn, double *sums2, void *workspace, size_t workspace_bytes, void *stream);
/* The same launch with a masked addend: dx = conv_transpose(dy, w) + (add_mask ? add : 0), add [N*H*W][add_pitch], add_mask
 * [N*H*W][Cin/4] (rcf_bn_apply_mp's sign bits) -- the conv1 of a bottleneck whose input also feeds the block's identity branch
 * (models/resnet.py:268-302): the identity's gradient IS the join's output gradient under the join's ReLU mask, so the batch norm's
 * backward need not write it (rcf_bn_bwd_apply_mp with dres = NULL: one tensor write less per identity block) and this launch need
 * not read it back -- it reads the join's output gradient instead.  Bit-identical to dres + accumulate.  beta must be 0 with an
 * addend; bn / sums2 / workspace as in rcf_conv2d_dgrad_bnsums_f32 or all NULL; same shapes (rcf_conv2d_dgrad_bnsums_ok). */
int rcf_conv2d_dgrad_add_f32(const float *dy, const float *w, float *dx, const rcf_conv_shape *s, int beta, const float *add,
                             int add_pitch, const unsigned char *add_mask, const rcf_bn_bwd_in *bn, double *sums2,
                             void *workspace, size_t workspace_bytes, void *stream);
/* dw[Cout][R][S][Cin] (+)= sum_pixels dy * x.  Split over pixels into `workspace`, then reduced
 * deterministically (no float atomics). */
size_t rcf_conv2d_wgrad_workspace_bytes(const rcf_conv_shape *s);
int rcf_conv2d_wgrad_f32(const float *x, const float *dy, float *dw, const rcf_conv_shape *s, int beta,
                         void *workspace, size_t workspace_bytes, void *stream);
size_t rcf_conv2d_wgrad_region_workspace_bytes(const rcf_conv_shape *s, const rcf_conv_region *region);
int rcf_conv2d_wgrad_region_f32(const float *x, const float *dy, float *dw, const rcf_conv_shape *s,
                                const rcf_conv_region *region, int beta, void *workspace, size_t workspace_bytes,
                                void *stream);

/* ---- the same three operators with bf16 OPERANDS and fp32 accumulation (csrc/igemm_bf16.hip) -----------------------
 * The mixed-precision training step (BASELINE configs[2]; the reference's AMP configs configs/rcf_stv2/rcf_stage1.yaml:57-60):
 * x, dy, dx are NHWC bf16 (channel counts and pitches multiples of 8, pitches in bf16 elements), weights stay fp32
 * master copies ([Cout][R][S][Cin]) and are cast per launch, dw is fp32.  One MFMA pass (v_mfma_f32_32x32x16_bf16).
 * rcf_conv_shape's amax / w_pairs members are ignored.
 * rcf_conv_weight_bf16: the kernels' weight operand, K-step major [K/32][rows][32] bf16 (K zero-padded to a multiple of
 * 32); transpose = 0: rows = Cout, k = (r, s, cin) -- forward; transpose = 1: rows = Cin, k = (r, s, cout) -- data gradient. */
size_t rcf_conv_weight_bf16_bytes(int Cout, int Cin, int R, int S, int transpose);
int rcf_conv_weight_bf16(const float *w, int Cout, int Cin, int R, int S, int transpose, void *out, unsigned flags,
                         void *stream);
/* y (ydt: RCF_BF16 or RCF_F32, pitch s->y_pitch in its own elements) (+)= conv(x, w) + bias, act 0 none / 1 LeakyReLU.
 * w_bf16 = rcf_conv_weight_bf16(w, ..., transpose 0).  region: as rcf_conv2d_fwd_region_f32 (NULL = whole tensor).
 * sums != NULL (needs region == NULL, bias == NULL, act == beta == 0 and the workspace): the batch-norm statistics of the
 * fp32 accumulators [sum | sumsq] per output channel from the epilogue, like rcf_conv2d_fwd_stats_f32. */
size_t rcf_conv2d_fwd_stats_bf16_workspace_bytes(const rcf_conv_shape *s);
int rcf_conv2d_fwd_bf16(const void *x, const void *w_bf16, const float *bias, void *y, int ydt, const rcf_conv_shape *s,
                        const rcf_conv_region *region, int act, float slope, int beta, double *sums, void *workspace,
                        size_t workspace_bytes, void *stream);
/* dx (bf16) (+)= conv_transpose(dy (bf16), w (fp32 master)); the workspace receives the transposed bf16 weights */
size_t rcf_conv2d_dgrad_bf16_workspace_bytes(const rcf_conv_shape *s);
int rcf_conv2d_dgrad_bf16(const void *dy, const float *w, void *dx, const rcf_conv_shape *s, const rcf_conv_region *region,
                          int beta, void *workspace, size_t workspace_bytes, void *stream);
/* ---- 1x1 conv -> training-mode batch norm -> (+ residual) -> ReLU as ONE tile (csrc/foldbn.hip, csrc/igemm_bf16.hip) ----------
 * Replaces, in the bf16 step, the bottleneck tail `out = conv3(out); out = norm3(out); out += identity; out = relu(out)`
 * (models/resnet.py:281-296) and the 1x1 downsample conv -> norm (models/res_layer.py:53-63) WITHOUT the conv output or its
 * gradient ever existing in memory.  A 1x1 conv is linear in its input, so the norm's statistics and both of its backward sums
 * are functions of two small moments of the conv's INPUT x [rows][K]: the column sums A1 [K] (rcf_colsum_mp) and the Gram
 * matrix S = x^T x [K][K] (rcf_conv2d_wgrad_bf16 with dy = x).  W [N][K] is the fp32 master weight; every routine rounds it to
 * bf16 as the conv kernels do.
 *   forward   rcf_fold_fwd_f32:       P = W (S - A1 A1^T / rows_local) [N][K] + the N local means of z behind it (N K + N floats, kept
 *                                     for the backward pass; the Gram matrix is centred in fp64 BEFORE the fp32 contraction, so the
 *                                     variance w . P / n carries no mean^2 to cancel), sums = [sum z | sum z^2] (fp64 [2N]; SyncBN
 *                                     all-reduces them like any other statistics) and / or the finalized norm
 *             rcf_fold_finalize_f32:  mean, invstd, running statistics, num_batches_tracked as rcf_bn_finalize_f32, plus the
 *                                     folded constants scale = gamma invstd, shift = beta - mean scale (after the all-reduce)
 *             rcf_conv2d_fwd_affine_bf16:  y = [relu](conv(x, w) * scale[c] + shift[c] [+ residual]) (bf16; whole column tiles:
 *                                     Cout % 64 == 0 and Cout in {64, 128} or Cout % 256 == 0; stride 1)
 *   backward  g = dy under the ReLU mask + its column sums: rcf_relu_mask_colsum_bf16 (one pass, in place allowed), or
 *             rcf_conv2d_dgrad_masked_bf16 when a data gradient is the LAST writer of dy: dx = mask_src > 0 ? dgrad (+ dx) : 0
 *             with colsums [2 Cin] (sum | sum of squares) from its epilogue
 *             G = g^T x [N][K]: rcf_conv2d_wgrad_bf16(x, g)
 *             rcf_fold_bwd_sums_f32:     sums2 = [sum g | sum g zhat] (fp64 [2N]) from G, W, the column sums of g
 *             rcf_fold_wg_bf16:          wg_t = the data gradient's weight operand (bf16, rcf_conv_weight_bf16 layout, transpose = 1) of
 *                                     scale[c] W[c][k] -- forward constants only, so g Wg^T may run beside the G product
 *             rcf_fold_bwd_prepare_f32:  dW += ..., dgamma += sums2_local[N + c], dbeta += sums2_local[c] (sums2_local NULL = sums2),
 *                                     negT (bf16, transpose = 0 layout of the K -> K weight -T), c0 [K]
 *             dx = rcf_conv2d_dgrad_bf16(g, w_pairs_t = wg_t) then rcf_conv2d_fwd_bf16(x, negT, bias = c0, beta = 1)
 * N % 64 == 0 and K % 64 == 0. */
typedef struct rcf_fold_finalize {
    double count;                 /* rows the statistics cover */
    float eps, momentum;
    const float *gamma, *beta;    /* the norm's affine parameters [C] */
    float *mean, *invstd;         /* out [C] */
    float *scale, *shift;         /* out [C]: gamma invstd, beta - mean gamma invstd */
    float *running_mean, *running_var;   /* may be NULL */
    long long *num_batches_tracked;      /* may be NULL */
} rcf_fold_finalize;
size_t rcf_fold_fwd_scratch_bytes(int N, int K);
/* A1: fp64 [K] (the first half of rcf_bn_stats_mp's sums of x); rows_local: the rows S and A1 were summed over (this rank's).
 * P: N K + N floats.  fin != NULL: the statistics are local (fin->count == rows_local), the norm is finalized by the same launch
 * (sums may be NULL); fin == NULL: sums only.  N % 64 == 0, K % 64 == 0. */
int rcf_fold_fwd_f32(const float *S, const double *A1, const float *W, float *P, double *sums, const rcf_fold_finalize *fin,
                     void *scratch, size_t scratch_bytes, double rows_local, int N, int K, void *stream);
int rcf_fold_finalize_f32(const double *sums, int C, const rcf_fold_finalize *fin, void *stream);
/* relu_bits (optional, with relu): receives the sign bits of y, one 64-bit wavefront ballot per (tile, wave, 32 x 32 sub-tile,
 * accumulator register) -- rcf_conv_relu_bits_bytes(rows, Cout) bytes, 1/16 of y; only a launch over the SAME [rows][Cout]
 * tensor can read them back (rcf_conv2d_dgrad_masked_bf16's mask_bits). */
size_t rcf_conv_relu_bits_bytes(long rows, int C);
int rcf_conv2d_fwd_affine_bf16(const void *x, const void *w_bf16, const float *scale, const float *shift, const void *residual,
                               int res_pitch, int relu, void *y, void *relu_bits, const rcf_conv_shape *s, void *stream);
size_t rcf_relu_mask_colsum_bf16_workspace_bytes(long rows, int C);
int rcf_relu_mask_colsum_bf16(const void *dy, int dy_pitch, const void *y, int y_pitch, void *g, int g_pitch, long rows, int C,
                              double *colsums, void *workspace, size_t workspace_bytes, void *stream);
size_t rcf_conv2d_dgrad_masked_bf16_workspace_bytes(const rcf_conv_shape *s);
/* the mask: mask_src (the bf16 ReLU output itself, [rows][Cin] with mask_pitch) or mask_bits (its sign bits as
 * rcf_conv2d_fwd_affine_bf16 wrote them: 1/16 of the bytes; mask_src may then be NULL) */
int rcf_conv2d_dgrad_masked_bf16(const void *dy, const void *w_t_bf16, void *dx, const rcf_conv_shape *s, int beta,
                                 const void *mask_src, int mask_pitch, const void *mask_bits, double *colsums, void *workspace,
                                 size_t workspace_bytes, void *stream);
int rcf_fold_bwd_sums_f32(const float *G, const float *W, const double *colsums, const float *mean, const float *invstd,
                          double *sums2, int N, int K, void *stream);
size_t rcf_fold_bwd_scratch_bytes(int N, int K);
int rcf_fold_wg_bf16(const float *W, const float *scale, void *wg_t_bf16, int N, int K, void *stream);
/* P: rcf_fold_fwd_f32's (N K + N floats) */
int rcf_fold_bwd_prepare_f32(const float *G, const float *P, const double *A1, const float *W, const double *sums2,
                             const double *sums2_local, double count, const float *mean, const float *invstd, const float *gamma,
                             float *dW, float *dgamma, float *dbeta, void *negT_bf16, float *c0, void *scratch,
                             size_t scratch_bytes, int N, int K, void *stream);

/* dw (fp32, [Cout][R][S][Cin]) (+)= sum over pixels of dy (bf16) * x (bf16); deterministic split-K through the workspace */
size_t rcf_conv2d_wgrad_bf16_workspace_bytes(const rcf_conv_shape *s, const rcf_conv_region *region);
int rcf_conv2d_wgrad_bf16(const void *x, const void *dy, float *dw, const rcf_conv_shape *s, const rcf_conv_region *region,
                          int beta, void *workspace, size_t workspace_bytes, void *stream);
/* ---- batch norm (training), fused ReLU / residual add / Dropout2d channel scale -----------------
 * Replaces (Sync)BatchNorm in models/resnet.py:159-162 and mmcv ConvModule's norm, the ReLU and
 * `out += identity` of models/resnet.py:268-300, and nn.Dropout2d of models/decode_head.py:84-85.
 * x is [rows][C] with pixel pitch `pitch` (rows = N*H*W).
 * stats: per-channel sum and sum of squares accumulated in fp64 -> sums[2*C] (doubles, [sum | sumsq]).
 * A data-parallel run all-reduces `sums` (and the row count) between stats and finalize: that IS SyncBN. */
size_t rcf_bn_stats_workspace_bytes(long rows, int C);
int rcf_bn_stats_f32(const float *x, long rows, int C, int pitch, double *sums, void *workspace,
                     size_t workspace_bytes, void *stream);
/* mean/invstd (biased var, eps) from sums over `count` rows; running stats updated with `momentum`
 * and the unbiased variance; running_* may be NULL. */
int rcf_bn_finalize_f32(const double *sums, double count, int C, float eps, float momentum, float *mean,
                        float *invstd, float *running_mean, float *running_var, void *stream);
/* y = [relu]( (x-mean)*invstd*gamma + beta [+ residual] ) [* chan_scale[n][c]]
 * rows_per_image only matters with chan_scale (Dropout2d keep-mask / keep-prob, NULL = off). */
int rcf_bn_apply_f32(const float *x, int x_pitch, const float *residual, int r_pitch, float *y, int y_pitch,
                     long rows, int C, const float *mean, const float *invstd, const float *gamma,
                     const float *beta, int relu, const float *chan_scale, long rows_per_image,
                     unsigned char *relu_mask, unsigned *amax_out, void *stream);
/* amax_out (may be NULL; here and in rcf_bn_bwd_apply_f32): amax_out[0] = max(amax_out[0], bits(max |output|)), the
 * operand range of the convs that read the output next (rcf_conv_shape), without another pass over it.
 * relu_mask (may be NULL): with relu, one byte per 4 channels [rows][C/4], bit e = output channel 4j+e was positive
 * before the clamp.  The backward kernels take it in place of y (1/16 of the bytes of re-reading y). */
/* eval-mode BN: same kernel with mean=running_mean, invstd from running_var */
int rcf_bn_invstd_from_var_f32(const float *var, int C, float eps, float *invstd, void *stream);
/* backward.  g = dy [* chan_scale] [* (y>0)];  sums2 = [sum g | sum g*xhat] (fp64).
 * After a data-parallel all-reduce of sums2:  dx = gamma*invstd*(g - sum_g/count - xhat*sum_gx/count) with the
 * GLOBAL sums and count; dgamma += sum_gx, dbeta += sum_g from sums2_local (this rank's sums before the
 * all-reduce; NULL = sums2) because the gradient all-reduce adds the ranks later; and (if dres != NULL)
 * dres (+)= g  (res_beta 0/1). */
int rcf_bn_bwd_reduce_f32(const float *dy, int dy_pitch, const float *x, int x_pitch, const float *y,
                          int y_pitch, long rows, int C, const float *mean, const float *invstd, int relu,
                          const unsigned char *relu_mask, const float *chan_scale, long rows_per_image,
                          double *sums2, void *workspace, size_t workspace_bytes, void *stream);
int rcf_bn_bwd_apply_f32(const float *dy, int dy_pitch, const float *x, int x_pitch, const float *y, int y_pitch,
                         float *dx, int dx_pitch, float *dres, int dres_pitch, int res_beta, long rows, int C,
                         const float *mean, const float *invstd, const float *gamma, int relu,
                         const unsigned char *relu_mask, const float *chan_scale, long rows_per_image,
                         const double *sums2,
                         const double *sums2_local, double count, float *dgamma, float *dbeta,
                         unsigned *amax_out, void *stream);

/* Mixed-precision forms of the batch-norm family (the `_f32` entry points above are these with every code RCF_F32).
 * xdt: storage type of the conv-output side (x, dx); ydt: of the activation side (y, residual, dy, dres).
 * Supported (xdt, ydt): (F32, F32), (BF16, BF16), (F32, BF16) -- an fp32 conv output (the stem) normalised into bf16
 * activations.  The reference runs these layers under torch autocast (configs/rcf_stv2/rcf_stage1.yaml:57-60). */
int rcf_bn_stats_mp(const void *x, int xdt, long rows, int C, int pitch, double *sums, void *workspace,
                    size_t workspace_bytes, void *stream);
/* out (+)= relu_mask ? dy : 0 (bit e of byte [row][c/4] = channel 4 (c/4) + e was positive, as rcf_bn_apply_mp writes it): the
 * gradient a join relu(bn3(x) + identity) passes to its identity branch (models/resnet.py:296-300), for callers that did not
 * let rcf_bn_bwd_apply_mp write it (dres = NULL) and cannot take it as the addend of rcf_conv2d_dgrad_add_f32. */
int rcf_relu_mask_copy_mp(const void *dy, int dt, int dy_pitch, const unsigned char *relu_mask, void *out, int out_pitch,
                          long rows, int C, int beta, void *stream);
/* `flags` of the three streaming passes (per call; 0 = the library's own choices):
 *   RCF_BN_SWEEP_OFF / RCF_BN_SWEEP_ALWAYS   row order (csrc/bn.hip struct Sweep): by default tensors of 192 MB and more are walked
 *       in eight bands (the conv kernels' XCD bands), the forward apply and the backward reduction downwards, the backward apply
 *       upwards -- a kernel starts in what its producer touched last, which the 256 MB Infinity Cache still holds; OFF: front to
 *       back; ALWAYS: banded on every tensor of 8192 rows and more (tests).  Element-wise outputs are bit-identical.
 *   RCF_BN_Y_PLANES_ONLY (apply, with planes_out)   y itself is not written (its only consumers are convs); y may be NULL.
 *   RCF_BN_DX_PLANES (bwd_apply)   dx is written as fp16 pair planes instead of fp32 (dx_pitch == C).
 * Pair planes (RCF_CONV_X_PLANES / RCF_CONV_DY_PLANES above): fp32 tensors only, C % 8 == 0, no chan_scale.  planes_out (apply):
 * [rows][h: C fp16 | m: C fp16] of y * 2^k; the scale comes from an upper bound of |y| (resp. |dx|) that every workgroup derives
 * from the per-channel constants, amax_x = the range of x (the conv epilogue's by-product) and amax_res / amax_dy = the ranges
 * of the residual / of dy BEFORE reading an element; the bound's raw bits are left in *amax_out, which is what the consuming
 * convs take as amax_x / amax_dy. */
#define RCF_BN_SWEEP_OFF 0x1u
#define RCF_BN_SWEEP_ALWAYS 0x2u
#define RCF_BN_Y_PLANES_ONLY 0x4u
#define RCF_BN_DX_PLANES 0x8u
int rcf_bn_apply_mp(const void *x, int xdt, int x_pitch, const void *residual, int r_pitch, void *y, int ydt, int y_pitch,
                    long rows, int C, const float *mean, const float *invstd, const float *gamma, const float *beta,
                    int relu, const float *chan_scale, long rows_per_image, unsigned char *relu_mask,
                    unsigned *amax_out, void *planes_out, const unsigned *amax_x, const unsigned *amax_res, unsigned flags,
                    void *stream);
/* rcf_bn_apply_mp whose residual is itself a conv output in front of a finalized train-mode batch norm WITHOUT ReLU (a stage's
 * downsample branch: models/resnet.py:293-294 `identity = self.downsample(x)`, `out += identity`): res_norm's four [C] vectors
 * normalise the residual on the fly -- (r - mean) * invstd * gamma + beta, the apply pass's own operations and order, rounded to
 * the storage type as the stored tensor would have been -- so that norm's apply pass never runs.  amax_res is then the range of
 * the RAW residual.  res_norm == NULL: rcf_bn_apply_mp. */
typedef struct rcf_bn_res_norm {
    const float *mean, *invstd, *gamma, *beta;
} rcf_bn_res_norm;
int rcf_bn_apply_res_mp(const void *x, int xdt, int x_pitch, const void *residual, int r_pitch, const rcf_bn_res_norm *res_norm,
                        void *y, int ydt, int y_pitch, long rows, int C, const float *mean, const float *invstd,
                        const float *gamma, const float *beta, int relu, const float *chan_scale, long rows_per_image,
                        unsigned char *relu_mask, unsigned *amax_out, void *planes_out, const unsigned *amax_x,
                        const unsigned *amax_res, unsigned flags, void *stream);
/* The join of a stage's first block together with its downsample norm in the backward pass (models/resnet.py:293-296): both
 * norms' backward is taken of g = dy under the JOIN's sign bits, against conv3's output x and the downsample conv's output x2.
 * rcf_bn_bwd_reduce2_mp: ONE reduction -> sums4 [4C] = [sum g | sum g xhat | sum g | sum g xhat2] (each norm's [2C] pair is
 * contiguous: what rcf_bn_bwd_reduce_mp would give it, bit for bit); workspace: 2 x rcf_bn_stats_workspace_bytes(rows, C).
 * rcf_bn_bwd_apply2_mp: ONE apply pass -> dx and second->dx (both fp32 / bf16, or with RCF_BN_DX_PLANES both as fp16 pair
 * planes, each with its own bound in its own amax_out), the parameter gradients of both norms; dy and the sign bits are read
 * once.  Same element operations in the same order as two rcf_bn_bwd_apply_mp calls with relu = 1 and this mask. */
typedef struct rcf_bn_bwd_second {
    const void *x;                 /* the second norm's input [rows][C], storage type of x */
    int x_pitch;
    void *dx;                      /* its input gradient */
    int dx_pitch;
    const float *mean, *invstd, *gamma;
    const double *sums2;           /* [2C] (global under SyncBN) */
    const double *sums2_local;     /* [2C] this rank's (parameter gradients); NULL = sums2 */
    float *dgamma, *dbeta;         /* accumulated into; may be NULL */
    unsigned *amax_out;            /* range of dx (fp32 / bf16: may be NULL) or, with planes, the bound they are scaled by */
    const unsigned *amax_x;        /* planes: range of x */
} rcf_bn_bwd_second;
int rcf_bn_bwd_reduce2_mp(const void *dy, int ydt, int dy_pitch, const void *x, int xdt, int x_pitch, const void *x2, int x2_pitch,
                          long rows, int C, const float *mean, const float *invstd, const float *mean2, const float *invstd2,
                          const unsigned char *relu_mask, double *sums4, void *workspace, size_t workspace_bytes, unsigned flags,
                          void *stream);
int rcf_bn_bwd_apply2_mp(const void *dy, int ydt, int dy_pitch, const void *x, int xdt, int x_pitch, void *dx, int dx_pitch,
                         long rows, int C, const float *mean, const float *invstd, const float *gamma,
                         const unsigned char *relu_mask, const double *sums2, const double *sums2_local, double count,
                         float *dgamma, float *dbeta, unsigned *amax_out, const unsigned *amax_x, const unsigned *amax_dy,
                         const rcf_bn_bwd_second *second, unsigned flags, void *stream);
int rcf_bn_bwd_reduce_mp(const void *dy, int ydt, int dy_pitch, const void *x, int xdt, int x_pitch, const void *y,
                         int y_pitch, long rows, int C, const float *mean, const float *invstd, int relu,
                         const unsigned char *relu_mask, const float *chan_scale, long rows_per_image, double *sums2,
                         void *workspace, size_t workspace_bytes, unsigned flags, void *stream);
int rcf_bn_bwd_apply_mp(const void *dy, int ydt, int dy_pitch, const void *x, int xdt, int x_pitch, const void *y,
                        int y_pitch, void *dx, int dx_pitch, void *dres, int dres_pitch, int res_beta, long rows, int C,
                        const float *mean, const float *invstd, const float *gamma, int relu,
                        const unsigned char *relu_mask, const float *chan_scale, long rows_per_image,
                        const double *sums2, const double *sums2_local, double count, float *dgamma, float *dbeta,
                        unsigned *amax_out, const unsigned *amax_x, const unsigned *amax_dy, unsigned flags, void *stream);
int rcf_colsum_mp(const void *x, int xdt, long rows, int C, int pitch, float *out, int beta, void *workspace,
                  size_t workspace_bytes, void *stream);

/* ---- pooling / resize / layout ------------------------------------------------------------------
 * MaxPool2d(3,2,1): models/resnet.py:577.  argmax: uint8 window position (r*3+s), first max wins.  Both directions answer
 * RCF_EINVAL unless Ho = (H - 1) / 2 + 1 and Wo = (W - 1) / 2 + 1 (y, dy and argmax are indexed by them) and every size is positive. */
int rcf_maxpool3x3s2_fwd_f32(const float *x, float *y, uint8_t *argmax, int N, int H, int W, int C, int Ho,
                             int Wo, void *stream);
int rcf_maxpool3x3s2_bwd_f32(const float *dy, const uint8_t *argmax, float *dx, int N, int H, int W, int C,
                             int Ho, int Wo, void *stream);
/* bilinear resize, NHWC, align_corners 0/1 (mmseg `resize`: models/decode_head.py:157-163,
 * models/rcf_model.py:213-220).  bwd is a gather over the contributing outputs (no atomics). */
int rcf_resize_bilinear_nhwc_fwd_f32(const float *x, int x_pitch, float *y, int y_pitch, int N, int Hi, int Wi,
                                     int Ho, int Wo, int C, int align_corners, void *stream);
int rcf_resize_bilinear_nhwc_bwd_f32(const float *dy, int dy_pitch, float *dx, int dx_pitch, int beta, int N,
                                     int Hi, int Wi, int Ho, int Wo, int C, int align_corners, void *stream);
/* planar NCHW bilinear resize (ground-truth flows 480x854 -> mask size, models/rcf_model.py:438-442) */
/* the same restricted to the border frame of thickness `frame` (fine-resolution pixels): fwd writes only the frame's
 * output pixels, bwd takes dy as zero off the frame (and does not read it there).  See rcf_conv_region. */
int rcf_resize_bilinear_nhwc_fwd_frame_f32(const float *x, int x_pitch, float *y, int y_pitch, int N, int Hi, int Wi,
                                           int Ho, int Wo, int C, int align_corners, int frame, void *stream);
int rcf_resize_bilinear_nhwc_bwd_frame_f32(const float *dy, int dy_pitch, float *dx, int dx_pitch, int beta, int N,
                                           int Hi, int Wi, int Ho, int Wo, int C, int align_corners, int frame,
                                           void *stream);
int rcf_resize_bilinear_nchw_f32(const float *x, float *y, int planes, int Hi, int Wi, int Ho, int Wo,
                                 int align_corners, void *stream);
/* NCHW [N,C,H,W] -> NHWC [N,H,W,Cpad] (channels >= C zero-filled) and back (drops the padding) */
int rcf_nchw_to_nhwc_f32(const float *x, float *y, int N, int C, int H, int W, int Cpad, void *stream);
int rcf_nhwc_to_nchw_f32(const float *x, int x_pitch, float *y, int N, int C, int H, int W, void *stream);
/* strided 2-D copy: dst[r*dpitch + c] (+)= src[r*spitch + c], c < C (concat / pair-concat / slices) */
int rcf_copy2d_f32(const float *src, long spitch, float *dst, long dpitch, long rows, int C, int beta,
                   void *stream);
/* n0 x n1 such copies in one launch: copy (i0, i1) reads src + i0*sb0 + i1*sb1 and writes dst + i0*db0 + i1*db1
 * (element offsets, multiples of 4, may be negative) -- the frames-of-a-pair channel concat of models/rcf_model.py:325 */
int rcf_copy2d_batched_f32(const float *src, long spitch, long sb0, long sb1, float *dst, long dpitch, long db0, long db1,
                           long rows, int C, int beta, int n0, int n1, void *stream);
/* dense NHWC [N,H,W,C]: inside = src on the rectangle (0 elsewhere), outside = src off the rectangle (0 on it);
 * either output may be NULL.  Splits a gradient into its interior / border-band parts (see rcf_conv_region). */
int rcf_split_rect_f32(const float *src, float *inside, float *outside, int N, int H, int W, int C, int y0, int x0,
                       int h, int w, void *stream);
/* Mixed-precision forms (dt = RCF_F32 / RCF_BF16 storage of every tensor argument; `frame` 0 = the whole tensor; -1 = the whole
 * tensor on the general kernels even where the exact-2x forms apply -- a thread there makes the 2 x 2 outputs of one source pixel
 * from 9 loads instead of 16, bit-identical -- for tests) */
int rcf_maxpool3x3s2_fwd_mp(const void *x, void *y, int dt, uint8_t *argmax, int N, int H, int W, int C, int Ho, int Wo,
                            void *stream);
int rcf_maxpool3x3s2_bwd_mp(const void *dy, const uint8_t *argmax, void *dx, int dt, int N, int H, int W, int C, int Ho,
                            int Wo, void *stream);
int rcf_resize_bilinear_nhwc_fwd_mp(const void *x, int x_pitch, void *y, int y_pitch, int dt, int N, int Hi, int Wi, int Ho,
                                    int Wo, int C, int align_corners, int frame, void *stream);
int rcf_resize_bilinear_nhwc_bwd_mp(const void *dy, int dy_pitch, void *dx, int dx_pitch, int dt, int beta, int N, int Hi,
                                    int Wi, int Ho, int Wo, int C, int align_corners, int frame, void *stream);
int rcf_copy2d_batched_mp(const void *src, long spitch, long sb0, long sb1, void *dst, long dpitch, long db0, long db1, int dt,
                          long rows, int C, int beta, int n0, int n1, void *stream);
/* source and destination in their own storage types: strided copy, or the fp32 <-> bf16 cast */
int rcf_copy2d_mp(const void *src, int sdt, long spitch, void *dst, int ddt, long dpitch, long rows, int C, int beta,
                  void *stream);
int rcf_split_rect_mp(const void *src, void *inside, void *outside, int dt, int N, int H, int W, int C, int y0, int x0, int h,
                      int w, void *stream);
/* column sums of [rows][C] (pitch) in fp64 -> out[C] (+)= (bias gradients of conv_seg) */
int rcf_colsum_f32(const float *x, long rows, int C, int pitch, float *out, int beta, void *workspace,
                   size_t workspace_bytes, void *stream);

/* ---- backward warp / occlusion / photometric residual -------------------------------------------
 * utils/warp_utils.py:84-94 (flow_warp; pad 0 = 'border', 1 = 'zeros'), :107-113 + :27-81
 * (get_occu_mask_backward), :97-104 (get_occu_mask_bidirection), models/amd/flow_loss.py:15-29 with
 * models/amd/loss_blocks.py:46-65 (L1 + SSIM photometric loss).  Planar NCHW fp32 as the reference. */
/* pad_mode: 0 border, 1 zeros.  RGB / border-mode calls take the tile kernels (lane = x, dword taps); pad_mode | RCF_WARP_PER_PIXEL
 * keeps such a call on the per-pixel kernels every other call takes (bit-identical results; a per-call choice for tests) */
#define RCF_WARP_PER_PIXEL 0x100
int rcf_flow_warp_f32(const float *x, const float *flow, float *out, int B, int C, int H, int W, int pad_mode,
                      void *stream);
/* grads of flow_warp w.r.t. x (atomic scatter; dx must be zero-filled or hold a running sum) and flow */
int rcf_flow_warp_bwd_f32(const float *x, const float *flow, const float *dout, float *dx, float *dflow, int B,
                          int C, int H, int W, int pad_mode, void *stream);
/* occ[B,1,H,W] = (clamp(splat(flow21),0,1) < th); scratch: B*H*W floats */
int rcf_occu_mask_backward_f32(const float *flow21, float *occ, float th, float *scratch, int B, int H, int W,
                               void *stream);
int rcf_occu_mask_bidirection_f32(const float *flow12, const float *flow21, float *occ, float scale, float bias,
                                  int B, int H, int W, void *stream);
/* fused warp + occlusion-masked L1: out[0] = sum |im1 - warp(im2,flow)| * occ, out[1] = sum occ (fp64) */
int rcf_warp_l1_residual_f32(const float *im1, const float *im2, const float *flow, const float *occ, double *out,
                             int B, int C, int H, int W, int pad_mode, void *stream);
/* loss_photomatric: (w_l1*mean(|a-b|*occ) + w_ssim*mean(SSIM(b*occ,a*occ))) / mean(occ) -> out[0] (fp32).
 * scratch: 4 doubles. */
int rcf_photometric_loss_f32(const float *im, const float *recon, const float *occ, float w_l1, float w_ssim,
                             float *out, double *scratch, int B, int C, int H, int W, void *stream);

/* ---- PWC-Lite cost volume (models/amd/correlation_native.py:6-23; csrc/correlation.hip) ----------------------------------
 * d = max_disp (1..4; PWC-Lite: 4), D = 2 d + 1, x1 / x2 f32 [B][C][H][W], out / dout f32 [B][D D][H][W]:
 *   corr[b, i D + j, y, x] = (1/C) sum_c x1[b,c,y,x] x2z[b,c, y+i-d, x+j-d]     i, j in 0..D-1, the row displacement i outermost
 *   out = corr where slope == 1, else corr > 0 ? corr : slope corr              (the LeakyReLU(0.1) of pwc_lite.py:202-203, fused)
 * x2z is x2 with real zeros outside the image, as F.pad makes them: the zeros are multiplied, not skipped (an infinite x1 against
 * a tap outside the image gives NaN; a NaN in x2 reaches exactly the (i, j, y, x) whose tap is that pixel).
 * Backward, with g = dout where slope == 1, else dout (out > 0 ? 1 : slope) for the caller's `out` (may be NULL iff slope == 1):
 *   dx1[b,c,y,x] = (1/C) sum_ij g[b, i D + j, y, x]         x2z[b,c, y+i-d, x+j-d]
 *   dx2[b,c,y,x] = (1/C) sum_ij g[b, i D + j, y-i+d, x-j+d] x1[b,c, y-i+d, x-j+d]   (terms whose source pixel is outside the image drop)
 * dx1 / dx2 (either may be NULL, not both) are OVERWRITTEN.  Every sum runs in one thread in a fixed order: no atomics, results
 * are bit-reproducible.  RCF_EINVAL before any launch -- sizes and ranges first, then pointers: a size <= 0, max_disp outside
 * 1..4, a tensor of 2^31 elements or more; a NULL operand, both gradients NULL, slope != 1 without out.
 * rcf_correlation_geometry: 0 -> rows, 1 -> columns of a workgroup's pixel tile, 2 -> channels staged per trip; 0 otherwise. */
int rcf_correlation_geometry(int which);
int rcf_correlation_fwd_f32(const float *x1, const float *x2, float *out, int B, int C, int H, int W, int max_disp, float slope,
                            void *stream);
int rcf_correlation_bwd_f32(const float *x1, const float *x2, const float *dout, const float *out, float *dx1, float *dx2, int B,
                            int C, int H, int W, int max_disp, float slope, void *stream);

/* ---- unFlowLoss (models/amd/flow_loss.py, models/amd/loss_blocks.py; csrc/unflow.hip) --------------------------------------
 * One direction of one pyramid level.  im, other f32 [B][3][h][w] (the area-resized frames), flow f32 [B][2][h][w] with batch
 * stride flow_bstride floats (a channel slice of the [B][4][h][w] pyramid flow is read in place), occ0 f32 [B][1][H0][W0] the
 * level-0 mask, read at (min(floor(y * float(H0) / h), H0 - 1), the same in x): torch's `nearest`.  With
 * rec = flow_warp(other, flow, 'border'), x = rec occ, y = im occ, md = ssim_sz in 1..3, n = (2 md + 1)^2:
 *   loss = ( w_l1 mean_{B,3,h,w} |im - rec| occ + w_ssim mean_{B,3,h-2md,w-2md} clamp((1 - S) / 2, 0, 1)
 *            + w_ternary mean_{B,1,h,w} T ) / mean_{B,1,h,w} occ                        (a weight <= 0 drops its term)
 *   S = a1 a2 / (b1 b2),  a1 = 2 mx my + C1, a2 = 2 cxy + C2, b1 = mx^2 + my^2 + C1, b2 = vx + vy + C2 over the window's means and
 *   biased (co)variances, C1 = 1e-4, C2 = 9e-4;  T at an interior pixel p (the 1-pixel border is 0) = (1/9) sum_k u_k^2 / (0.1 + u_k^2),
 *   u_k = t(Ix(p+k) - Ix(p)) - t(Iy(p+k) - Iy(p)), t(d) = d / sqrt(0.81 + d^2), I = 255 (0.2989 R + 0.5870 G + 0.1140 B).
 * fwd: out f32 [5] = loss, the three means (L1, SSIM, ternary), the mask mean (0 -> loss NaN, as the reference's 0 / 0).
 *   partials: rcf_unflow_photo_partials(B, h, w) doubles (RCF_EWORKSPACE when partials_len is less).
 * bwd: dflow f32 [B][2][h][w] OVERWRITTEN with (dloss[0] / stats[4]) sum_c d rec_c d sample / d position (the tap differences of
 *   rcf_flow_warp_bwd_f32; 0 on a clipped coordinate), stats = the forward's out, dloss a device scalar, and
 *   d rec_q = occ_q ( -w_l1 sign(im - rec) / count_l1  +  sum_{p contains q} A_p + x_q sum B_p + y_q sum C_p  +  ternary ) with, for window p,
 *   live = 0 < (1 - S) / 2 < 1, wgt = -(1/2) live w_ssim / count_ssim,
 *   A = wgt (2 my (a2 - a1) / (b1 b2) - 2 mx S (1 / b1 - 1 / b2)) / n,  B = -2 wgt S / (b2 n),  C = 2 wgt a1 / (b1 b2 n);
 *   the ternary part: 255 (0.2989, 0.5870, 0.1140)_c (w_ternary / (9 B h w)) sum over the 8 neighbours m of q of
 *   ([m interior] + [q interior]) g'(u) t'(d1), d = I(q) - I(m), g'(u) = 0.2 u / (0.1 + u^2)^2, t'(d) = 0.81 / (0.81 + d^2)^1.5.
 * Every sum is a gather in a fixed order, no atomics: the same bits on every call.  Nothing synchronises with the host.
 * smooth: flow / s through smooth_grad_1st (second = 0) or smooth_grad_2nd (1) with im [B][3][h][w]; out f32 [1]; an axis with no
 *   difference gives the reference's NaN.  partials: 2048 doubles.  bwd: dflow OVERWRITTEN with dloss[0] d out / d flow, sign(0) = 0.
 * area: adaptive average [B][3][H][W] (batch stride x_bstride floats) -> [B][3][h][w], rows floor(i H / h) .. ceil((i + 1) H / h):
 *   F.interpolate(mode='area').
 * RCF_EINVAL before any launch -- sizes first, then pointers: B, h, w, H0 or W0 <= 0, md outside 1..3, h or w under 2 md + 1,
 * h w or H0 W0 >= 2^30, a batch stride under the tensor's own, second outside {0, 1}; a NULL pointer.
 * rcf_unflow_geometry: 0 -> rows, 1 -> columns of a workgroup's tile, 2 -> the largest md; 0 otherwise. */
int rcf_unflow_geometry(int which);
long rcf_unflow_photo_partials(int B, int h, int w);
int rcf_unflow_photo_fwd_f32(const float *im, const float *other, const float *flow, long flow_bstride, const float *occ0, int H0,
                             int W0, int md, float w_l1, float w_ssim, float w_ternary, float *out, double *partials,
                             long partials_len, int B, int h, int w, void *stream);
int rcf_unflow_photo_bwd_f32(const float *im, const float *other, const float *flow, long flow_bstride, const float *occ0, int H0,
                             int W0, int md, float w_l1, float w_ssim, float w_ternary, const float *dloss, const float *stats,
                             float *dflow, int B, int h, int w, void *stream);
int rcf_unflow_smooth_fwd_f32(const float *flow, long flow_bstride, const float *im, float alpha, float s, int second, float *out,
                              double *partials, int B, int h, int w, void *stream);
int rcf_unflow_smooth_bwd_f32(const float *flow, long flow_bstride, const float *im, float alpha, float s, int second,
                              const float *dloss, float *dflow, int B, int h, int w, void *stream);
int rcf_unflow_area_f32(const float *x, long x_bstride, float *out, int B, int H, int W, int h, int w, void *stream);

/* ---- dense CRF (permutohedral mean-field) -------------------------------------------------------
 * Replaces torchcrf_cpp.crf_soft / crf_hard (tools/torchCRF/src/torchcrf.cu:106-149), batched over
 * frames, persistent caller-owned workspace instead of 12 cudaMalloc/cudaFree per frame.
 *   rgb   : u8 [batch,H,W,3]         unary : f32 [batch,H*W,2] energies (label minor)
 *   out   : i16 [batch,H,W] MAP      q_out : optional f32 [batch,H*W,2] final marginals (NULL = skip)
 *   nvert : optional int32 [batch,2] lattice vertex counts (smoothness, appearance)
 * A potential is active when its weight and sigma are > 0 (torchcrf.cu:28,41). */
size_t rcf_crf_workspace_bytes(int W, int H, int batch);
int rcf_crf_soft(const uint8_t *rgb, const float *unary, int W, int H, int batch, float scomp_smooth,
                 float sxy_smooth, float scomp_app, float sxy_app, float srgb_app, int iters, int16_t *out_map,
                 float *q_out, int32_t *nvert, void *workspace, size_t workspace_bytes, void *stream);
/* normalization 0 = rcf_crf_soft; 1 = the symmetric kernel normalisation N^1/2 K N^1/2, N = diag(1 / (K 1 + 1e-20)), of
 * pydensecrf's DenseCRF2D (NORMALIZE_SYMMETRIC, the default of addPairwiseBilateral): the CPU post-processor
 * tools/pydenseCRF/crf.py:58-89 and models/crf_head.py:62-91.  Exactly one potential may be active with 1. */
int rcf_crf_soft_ex(const uint8_t *rgb, const float *unary, int W, int H, int batch, float scomp_smooth, float sxy_smooth,
                    float scomp_app, float sxy_app, float srgb_app, int iters, int normalization, int16_t *out_map,
                    float *q_out, int32_t *nvert, void *workspace, size_t workspace_bytes, void *stream);
/* rcf_crf_soft_ex on FLOAT colour features f32 [batch,H,W,3]: torchcrf_cpp.crf_soft accepts rgbFeat of any dtype and converts
 * it to float unrounded (tools/torchCRF/src/torchcrf.cu:84-85); RCF itself passes uint8 (models/crf_head.py:43-55).  Always
 * the array-of-keys lattice build (the RCF_CRF_BUILD_* bits are ignored). */
int rcf_crf_soft_f32(const float *rgbf, const float *unary, int W, int H, int batch, float scomp_smooth, float sxy_smooth,
                     float scomp_app, float sxy_app, float srgb_app, int iters, int normalization, int16_t *out_map,
                     float *q_out, int32_t *nvert, void *workspace, size_t workspace_bytes, void *stream);
int rcf_crf_hard(const uint8_t *rgb, const int16_t *label, int W, int H, int batch, float scomp_smooth,
                 float sxy_smooth, float scomp_app, float sxy_app, float srgb_app, float confidence, int iters,
                 int16_t *out_map, float *q_out, int32_t *nvert, void *workspace, size_t workspace_bytes,
                 void *stream);
/* lattice build, OR-ed into rcf_crf_soft_ex's `normalization` (a per-call choice; results are identical): default = packed
 * 64-bit keys + block-local de-duplication when the key coordinates fit 12 bits; ARRAY = always the array-of-keys build;
 * SMALL_TABLE = packed build whose first-attempt table is tiny, so every frame takes the overflow path (tests) */
#define RCF_CRF_BUILD_ARRAY 0x100
#define RCF_CRF_BUILD_SMALL_TABLE 0x200
/* SORT = the appearance lattice by ONE device-wide radix sort of all frames' (packed key, entry) pairs + run heads + scan
 * instead of the hash table (the sort / unique / scan form of SURVEY section 7 step 6): vertices numbered in key order, neighbour
 * search as a merge.  Slower than the packed build on natural frames (a few 10^4 vertices per frame), faster on noise-like
 * ones (10^6 vertices): what the caller picks when the previous call's vertex counts were high (rcf_amd.crf.CRFHead).
 * Needs keys that fit 12 bits per coordinate and batch <= 16; otherwise the default build runs. */
#define RCF_CRF_BUILD_SORT 0x300
/* the six blur passes of a filter as six launches (one per lattice axis) instead of three (two axes per launch, the first
 * axis's values recomputed on the fly for the three vertices the second reads: same operations, same bits) -- tests and A/B */
#define RCF_CRF_BLUR_SEQUENTIAL 0x400
/* The splat of a filter pass.  Default: frames built by the packed build whose 16 x 16 pixel tiles share most of their vertices
 * (natural images) take the TILE splat -- a scatter into the tile's short vertex list in LDS, one 64-bit atomic per distinct
 * vertex of the tile and channel, no CSR list built -- the others the gather over the CSR lists.  Sums are in 2^-40 fixed point
 * either way: identical bits.  SPLAT_GATHER: always the gather (A/B, tests); SPLAT_TILES: the tile splat for every frame the
 * packed build made, whatever its content (tests). */
#define RCF_CRF_SPLAT_GATHER 0x4000
#define RCF_CRF_SPLAT_TILES 0x8000
/* With ONE potential active, the slice of a filter pass hands a tile-mode frame's new marginals straight to the next pass's
 * per-tile sums (one kernel reads the entries' weights and list positions once; the intermediate marginals are never written).
 * SLICE_SPLAT_SEPARATE: slice and per-tile sums as two kernels, as with two potentials (tests, A/B; identical bits). */
#define RCF_CRF_SLICE_SPLAT_SEPARATE 0x10000
/* CRFHead pre-processing (models/crf_head.py:33-37,43-55,95-98): normalised NCHW image -> u8 HWC;
 * soft mask -> u8 quantisation -> unary energies.  scratch: batch uint32 (per-frame max). */
int rcf_crf_prepare(const float *img_nchw, const float *mask, const float *mean3, const float *std3,
                    int unstandardize, float crf_scale, uint8_t *rgb_out, float *unary_out, uint32_t *scratch,
                    int batch, int H, int W, void *stream);
/* Unary energies of the pydenseCRF post-processor (tools/pydenseCRF/crf.py:60-68) from u8 masks [frames][npix], by table:
 * unary[f][p][:] = table[max_f][mask[f][p]][:], max_f the largest byte of frame f.  table: [256][256][2] fp32 on the device, indexed
 * (frame maximum, pixel value) -- the caller tabulates the host's float64 steps (divide by the maximum + 1e-8, clip, -log(1 - U),
 * -log(U); any monotone pre-scaling of the bytes composed in), so the device copies the host's bits and evaluates no function.
 * unary: [frames][npix][2] fp32, the layout rcf_crf_soft takes.  scratch: frames uint32 (per-frame maximum; zeroed by the call).
 * npix needs no alignment (the mask is read in aligned 16-byte pieces wherever a frame starts); table and unary 8-byte aligned. */
int rcf_crf_unary_lut_u8(const uint8_t *mask, int frames, long npix, const float *table, float *unary, uint32_t *scratch,
                         void *stream);

/* ---- flow-aggregation head (relaxed common fate) + loss tail ------------------------------------
 * models/flow_aggregation_head_with_residual.py:235-310 (aggregate), :164-233 (per-segment affine
 * least squares), :312-399 (forward, L1 / robust loss); softmax + double-softmax entropy of
 * models/rcf_model.py:433-434,376-378; asymmetric clamped MSE against pl / crf targets :380-408.
 * "Direction image" n = 2*b + d: d = 0 forward (frame-0 masks, fw flow, residual channels [0,2C)),
 * d = 1 backward (frame-1 masks, bw flow, residual channels [2C,4C)); P = h*w.
 *   logits   NHWC [2B][P][logits_pitch]         (conv_seg output of decode_head2)
 *   feat     NHWC [2B][P][64]                   (flow_feat_before_agg output, LeakyReLU applied)
 *   residual NHWC [B][P][4C]                    (decode_head3 output resized to the mask size)
 *   W1 [64][64], b1 [64], W2 [2][64], b2 [2]    (flow_feat_after_agg Conv1d weights)
 *   targets  [2B][P] planar or NULL             (pl / crf masks at mask size)
 * The same workspace must be passed to prepare -> fwd -> bwd of one step. */
typedef struct {
    int B, C, h, w;          /* pairs, segments (mask_layer), mask size */
    int logits_pitch;
    int nf;                  /* must be 64 */
    int D;                   /* 0 free_residual, 2 free_residual_with_affine, 5 + quadratic */
    int robust;              /* outlier_robust_loss */
    int tanh_residual;       /* 1: scale*tanh(r/div) ; 0: plain r (residual_adjustment_scale == -1) */
    float eps, q;
    float clamp_t;           /* < 0: no clamp */
    float res_scale, div_coeff;
    float w_seg, w_entropy;
    int n_targets, target_channel;
    float t_wpos[2], t_wneg[2], t_weight[2], t_thresh[2];   /* t_thresh -1: soft target */
    /* models/compactness_head.py:14-57 (GWM compactness of one channel); weight 0 = off */
    float w_compact;
    int compact_channel;
    /* models/rcf_model.py:350-374 sharpen loss: mode 0 off, 1 KL to the sharpened (p^(1/T)) masks,
     * 2 object-aware hinge on |p_obj - max other| (object channel = target_channel) */
    float w_sharpen, t_sharpen;
    int sharpen_mode;
} rcf_flowhead_cfg;
size_t rcf_flowhead_workspace_bytes(const rcf_flowhead_cfg *c);
/* gt_fw / gt_bw [B][2][P] -> clamped flows (kept in the workspace) and flow4 NHWC [2B][P][4], the
 * zero-padded input of flow_feat_before_agg.0 */
int rcf_flowhead_prepare_f32(const rcf_flowhead_cfg *c, const float *gt_fw, const float *gt_bw, float *flow4,
                             void *workspace, size_t workspace_bytes, void *stream);
/* losses_out[8] = seg_fw, seg_bw, entropy, target0, target1, compactness, sharpen, 0 (unweighted means).  masks_out [2B][C][P] and
 * the four flow planes [2B][2][P] (overall, aggregated, residual adjustment, affine) are optional. */
int rcf_flowhead_fwd_f32(const rcf_flowhead_cfg *c, const float *logits, const float *feat, const float *residual,
                         const float *W1, const float *b1, const float *W2, const float *b2, const float *target0,
                         const float *target1, float *losses_out, float *masks_out, float *flow_pred,
                         float *flow_agg, float *flow_adj, float *flow_aff, void *workspace, size_t workspace_bytes,
                         void *stream);
/* gradients of grad_scale * (w_seg*seg + w_entropy*entropy + sum t_weight*target + w_compact*compactness +
 * w_sharpen*sharpen): dlogits (same layout as
 * logits, written), dresidual [B][P][4C] (written), dfeat [2B][P][64] = gradient w.r.t. the PRE-activation of
 * the second flow conv (written); dW1/db1/dW2/db2 accumulate. */
int rcf_flowhead_bwd_f32(const rcf_flowhead_cfg *c, const float *feat, const float *residual, const float *W1,
                         const float *W2, const float *target0, const float *target1, float grad_scale,
                         float *dlogits, float *dresidual, float *dfeat, float *dW1, float *db1, float *dW2,
                         float *db2, void *workspace, size_t workspace_bytes, void *stream);
/* dx = dy * (y > 0 ? 1 : slope), y = LeakyReLU output (n % 4 == 0) */
int rcf_lrelu_bwd_f32(const float *dy, const float *y, float *dx, long n, float slope, void *stream);

/* ---- optimiser / EMA ----------------------------------------------------------------------------
 * torch.optim.Adam with coupled weight decay (main.py:299-307) over one flat fp32 buffer;
 * EMA lerp of utils/model_utils.py:33-38 over flat buffers. */
int rcf_adam_step_f32(float *param, const float *grad, float *exp_avg, float *exp_avg_sq, long n, float lr,
                      float beta1, float beta2, float eps, float weight_decay, int step, float grad_scale,
                      void *stream);
int rcf_ema_update_f32(float *dest, const float *src, long n, float m, void *stream);
/* ... over ALL entries of a state dict in one launch (utils/model_utils.py:33-38 loops over them: ~500 launches of a few
 * microseconds per step for the EMA teacher, which the host cannot enqueue as fast as the GPU runs them -- 5.7 ms of idle GPU per
 * bf16 stage-2.1 step).  `chunks_dev`: device array of `count` chunks, one workgroup each; kind 0: fp32 dest = dest m + src (1 - m),
 * kind 1: int64 counters (num_batches_tracked), dest = trunc(float(dest) m + float(src) one_minus_m_counter) -- what torch's
 * int64 * python-float arithmetic gives the reference. */
typedef struct rcf_ema_chunk {
    void *dst;
    const void *src;
    long n;
    long kind;
} rcf_ema_chunk;
int rcf_ema_update_multi(const rcf_ema_chunk *chunks_dev, int count, float m, float one_minus_m_counter, void *stream);
int rcf_fill_f32(float *p, long n, float v, void *stream);
/* nn.Dropout2d's draw as a per-(sample, channel) scale (models/decode_head.py:84-87, models/fcn_head.py:142-147): out[i] = 0 with
 * probability p, 1 / (1 - p) otherwise, i < n = samples * channels; Philox4x32-10 keyed by `seed`, counter = i (reproducible
 * whatever the launch geometry).  The batch-norm apply pass of the head's last conv module multiplies it in (chan_scale). */
int rcf_dropout2d_scale_f32(float *out, long n, float p, unsigned long long seed, void *stream);

/* ---- evaluation metric ---------------------------------------------------------------
 * main.py:200-235 + utils/eval_utils.py:5-52,120-123: masks [B,C,h,w] (fp32 softmax) are resized to the annotation size
 * [H,W] (bilinear, align_corners=True), binarised (> pos_th; pos_th == -1 exactly: one-hot of the channel argmax) and compared with
 * the u8 annotation (255 foreground, 128 ignored, else background).  counts [B][C][3] uint64, zero-filled by the caller:
 * intersection, prediction area, label area of the foreground over the valid pixels; IoU = I / (P + L - I). */
int rcf_eval_iou_counts_f32(const float *masks, const uint8_t *ann, int B, int C, int h, int w, int H, int W, float pos_th,
                            unsigned long long *counts, void *stream);

/* ---- DAVIS J & F counts (tools/davis2016-evaluation/davis2017/metrics.py) ----------------------------------------------
 * pred, gt, void_px u8 [N][H][W], any nonzero byte = on; void_px NULL = no void pixels.  counts [N][6] int64, zero-filled by
 * the caller: inter, union (db_eval_iou), n_fg, n_gt, fg_match, gt_match (f_measure: boundary pixels of _seg2bmap(mask & !void)
 * and those within the disk X^2+Y^2 <= radius^2 of a boundary pixel of the other map).  RCF_EINVAL for radius outside
 * [0, 64], N, H or W <= 0, or a NULL pred / gt / counts, before any launch. */
int rcf_davis_counts_u8(const uint8_t *pred, const uint8_t *gt, const uint8_t *void_px, int N, int H, int W, int radius,
                        long long *counts, void *stream);

/* ---- data transform on the device ------------------------------------------------------
 * dataset/transforms.py:884-924 `Transform` (Resize :170-237 -> RandomCrop :442-508 -> RandomFlip :249-306 ->
 * PhotoMetricDistortion :557-687 -> FlowTransform :825-848 / PLTransform :865-876 -> NumpyToTensor :793-808 ->
 * TorchNormalize :850-863) as one gather per output tensor.  The random decisions are drawn by the host in the
 * reference's order and passed per sample: */
typedef struct rcf_aug_params {
    int32_t rw, rh;            /* size of the resized frame (mmcv.rescale_size of the drawn scale) */
    int32_t crop_x, crop_y;    /* RandomCrop offset inside the resized frame (0,0 and out = resized size: no crop) */
    int32_t flip;              /* horizontal flip of the crop */
    int32_t ops;               /* bit 0 brightness, 1 contrast, 2 saturation, 3 hue, 4 contrast applied last (mode 0) */
    float beta;                /* brightness offset */
    float alpha_c, alpha_s;    /* contrast / saturation gains */
    float flow_sx, flow_sy;    /* FlowTransform(scale_flow): factors on (u, v); 1 when off */
    double hue_delta;          /* python float in the reference: the hue arithmetic is fp64 */
} rcf_aug_params;
/* frames u8 [B][I][H][W][3] (decoded RGB) -> out fp32 [I][B][3][oh][ow]: (u8/255 - mean)/std of the bilinearly resized
 * (cv2 8-bit fixed point), cropped, flipped, distorted frame.  params: device array [B]; mean3/std3: host arrays. */
int rcf_aug_frames_u8(const uint8_t *frames, int B, int I, int H, int W, const rcf_aug_params *params, float *out, int oh,
                      int ow, const float *mean3, const float *std3, void *stream);
/* seg fields (nearest resize, crop, flip -- the reference does not negate u under a flip): flows fp32 [B][K][H][W][2] ->
 * [K][B][2][oh][ow];  pseudo-label masks u8 [B][K][H][W] -> fp32 [K][B][oh][ow] = u8/255 */
int rcf_aug_flows_f32(const float *flows, int B, int K, int H, int W, const rcf_aug_params *params, float *out, int oh,
                      int ow, void *stream);
int rcf_aug_masks_u8(const uint8_t *masks, int B, int K, int H, int W, const rcf_aug_params *params, float *out, int oh,
                     int ow, void *stream);

/* ---- Pillow's 8-bit resampler + IoU counts (tools/STv2-FBMS59-evaluation/eval_tool.py; csrc/pil_resample.hip) ----------
 * Image.resize of N u8 planes [h][w] to [H][W] with Pillow's integer arithmetic (libImaging/Resample.c, 8 bits per channel): a
 * horizontal and then a vertical pass, each out = clip(((1 << 21) + sum_j k[i][j] in[first_i + j]) >> 22, 0, 255) in int32, the
 * horizontal result rounded to u8 before the vertical pass.  The tables carry the filter and the scale (rcf_amd.pilresize
 * .coeff_tables transcribes Pillow's): kx int32 [W][ksx] with bx int32 [W][2] = (first tap, tap count <= ksx) per output column,
 * ky [H][ksy] / by [H][2] per output row; taps must lie inside the frame (ranges are clamped, a malformed table gives a wrong
 * picture and no access outside src).  kx == NULL: no horizontal pass (needs W == w), ky == NULL: no vertical pass (H == h), as
 * Pillow skips the pass of an axis that keeps its size.  src: element (n, y, x) at src[((n h + y) w + x) pix_stride]:
 * pix_stride 1 = packed L planes, 3 = channel 0 of interleaved RGB read in place.
 * dst (may be NULL): u8 [N][H][W].  counts (may be NULL): int64 [N][2], zero-filled by the caller, += (intersection, union) of
 * (resized >= pred_min) and (gt != 0) with gt u8 [N][H][W]; 0 <= pred_min <= 256.  Integer atomics: order-independent.
 * RCF_EINVAL before any launch: a NULL src, sizes <= 0, pix_stride not 1 or 3, neither dst nor counts, counts without gt, a table
 * without its bounds or tap count, a missing table on an axis that changes size, ksy > RCF_PIL_MAX_TAPS (the source rows of
 * one output row no longer fit the kernel's LDS window; bicubic: a reduction beyond 63 x).  Nothing allocates.
 * rcf_pil_resample_tile_rows: the output rows per block the launch uses for (h, H, ksy) -- 32, 16, ..., 1, the tallest tile whose
 * source rows fit the window; ksy = 0: no vertical pass; 0 when the call would be refused.  A pure function. */
#define RCF_PIL_MAX_TAPS 256
int rcf_pil_resample_tile_rows(int h, int H, int ksy);
int rcf_pil_resample_u8(const uint8_t *src, int N, int h, int w, int pix_stride, const int32_t *kx, const int32_t *bx, int ksx,
                        const int32_t *ky, const int32_t *by, int ksy, int H, int W, uint8_t *dst, const uint8_t *gt,
                        int pred_min, long long *counts, void *stream);

/* ---- DINO ViT forward + soft NCut -----------------------------------------
 * models/dino_vit.py:110-167,176-276 (nn.Linear / attention products, LayerNorm eps 1e-6, softmax, GELU) and
 * tools/SemanticConstraintsAndMAA/semantic_constraints.py:21-75 (soft NCut value, Adam refinement of the mask). */
/* C[M][N] (pitch ldc) (+)= A[M][K] (pitch lda) . B[N][K]^T (pitch ldb) + bias[N]; act 0 none / 1 LeakyReLU / 2 GELU(erf).
 * Runs on the implicit-GEMM conv kernel (fp32-level error).  K, lda, ldb, ldc multiples of 4.
 * amax_a / amax_b (both or neither; may be NULL): operand ranges -> fp16 pairs instead of bf16 triples (rcf_conv_shape);
 * b_pairs (may be NULL): B already split by rcf_conv_weight_pairs_f32(B, N, K, 1, 1, amax_b, ...), needs ldb == K;
 * amax_out (may be NULL): amax_out[0] = max(amax_out[0], bits(max |C written|)) -- the range of whatever reads C next. */
int rcf_gemm_nt_f32(const float *A, int lda, const float *B, int ldb, const float *bias, float *C, int ldc, int M, int N,
                    int K, int act, float slope, int beta, const unsigned *amax_a, const unsigned *amax_b,
                    const void *b_pairs, unsigned *amax_out, void *stream);
/* batch0 x batch1 independent products in one launch (attention: images x heads); strides in elements */
int rcf_gemm_nt_batched_f32(const float *A, int lda, long a_s0, long a_s1, const float *B, int ldb, long b_s0, long b_s1,
                            float *C, int ldc, long c_s0, long c_s1, int batch0, int batch1, int M, int N, int K, int act,
                            float slope, int beta, void *stream);
/* fused multi-head attention forward (scores stay on chip): out[b*T+t][h*64+d] = softmax_j(scale q_t.k_j) v_j[d];
 * qkv [B*T][3*nh*64] (q | k | v) as produced by the fused qkv linear (models/dino_vit.py:122-133).  head_dim = 64. */
int rcf_attention_fwd_f32(const float *qkv, int ld_qkv, float *out, int ld_out, int B, int T, int nh, int head_dim,
                          float scale, const unsigned *amax_qkv, unsigned *amax_out, void *stream);
/* amax_qkv: max |qkv| (rcf_absmax_f32, or the amax_out of the qkv GEMM) -> fp16-pair arithmetic (q, k, v scaled by one
 * power of two, probabilities by 2^14, 3 partial products); NULL -> bf16 triples (6).  amax_out (may be NULL): the
 * range of `out`. */
int rcf_layernorm_f32(const float *x, int x_pitch, float *y, int y_pitch, long rows, int C, const float *gamma,
                      const float *beta, float eps, unsigned *amax_out, void *stream);
/* in place: row <- softmax(scale * row[0:n]); columns [n, pitch) are zeroed */
int rcf_softmax_rows_f32(float *s, long pitch, long rows, int n, float scale, void *stream);
/* dst[c][r] = src[r][c]; dst columns [rows, dpitch) zero-filled */
int rcf_transpose2d_f32(const float *src, long spitch, float *dst, long dpitch, int rows, int cols, void *stream);
int rcf_l2_normalize_rows_f32(const float *x, long x_pitch, float *y, long y_pitch, long rows, int C, void *stream);
/* gram[i][j] <- gram[i][j] > tau ? 1 : eps */
int rcf_affinity_threshold_f32(float *gram, long pitch, int n, float tau, float eps, void *stream);
int rcf_ncut_value_grad_f32(const float *affinity, long pitch, int n, const float *x, double *u, double *rowsum,
                            int compute_rowsum, float *grad, float *value_out, void *stream);
int rcf_clamp01_f32(float *x, int n, void *stream);
/* MAA (tools/SemanticConstraintsAndMAA/maa.py:19-36): the soft-NCut terms of M masks per frame in ONE pass over the RAW Gram
 * matrices gram[frames][n][pitch], which are only read -- a_ij = (gram_ij > tau ? 1 : eps) is formed in registers and no
 * symmetry is assumed.  masks[frames][M][n], 1 <= M <= 8; out[frames][M][4] = {ncut, cut, assocA, assocB} (fp64; IEEE
 * semantics: an all-zero mask gives NaN).  pitch >= n, pitch % 4 == 0, gram 16-byte aligned.  Per-workgroup fp64 partials go
 * to `workspace` and are added in a fixed order by a second launch: no atomics, bit-identical from run to run, and a frame's
 * result does not depend on `frames` or on its position.  The grid is sized from the device's compute-unit count. */
size_t rcf_ncut_values_workspace_bytes(int frames, int n, int M);
int rcf_ncut_values_f32(const float *gram, long pitch, int n, int frames, float tau, float eps, const float *masks, int M,
                        double *out, void *workspace, size_t workspace_bytes, void *stream);

/* ---- semantic-constraint refinement for a batch of frames (tools/SemanticConstraintsAndMAA/semantic_constraints.py:21-75,
 * 299-336; csrc/semantic.hip) ---------------------------------------------------------------------------------------------
 * rcf_affinity_pack_f32: ONE read-only pass over the raw Gram matrices gram[frames][n][pitch] (pitch >= n, no alignment asked):
 * bit j of row i is set when gram_ij > tau (strict; a NaN gives 0), no symmetry assumed.  bits[frames][n][W] 32-bit words with
 * W = rcf_affinity_pack_words(n) = 2 ceil(n / 64) (bit j of a row = bit j % 32 of word j / 32; every bit from n on is 0; bits
 * 8-byte aligned); deg[frames][n] = the popcount of the row.  The bit matrix of a 6 420-token frame takes 5.2 MB. */
int rcf_affinity_pack_words(int n);
int rcf_affinity_pack_f32(const float *gram, long pitch, int n, int frames, float tau, uint32_t *bits, int32_t *deg, void *stream);
/* rcf_ncut_refine_packed_f32: `steps` Adam steps on the soft NCut of x[frames][n] (in place) against the affinity
 * a_ij = (bit ij ? 1 : eps) given as packed bits + row popcounts, for every frame of the batch.  With e = (double)eps:
 * u_i = e sum_j x_j + (1 - e) sum_{j in row i} x_j,  s_i = e n + (1 - e) deg_i,  value and gradient as rcf_ncut_value_grad_f32
 * (closed form, fp64), then the arithmetic of rcf_adam_step_f32 (betas 0.9 / 0.999, eps 1e-8, coupled weight decay, bias
 * correction with the step number) and a clamp to [0, 1].  Two launches per step for the whole batch (row sums: grid.y = frame;
 * value + gradient + Adam + clamp: one workgroup per frame); steps are separated by kernel boundaries only.  Reductions are
 * fp64 in a fixed order without atomics: a frame's result depends neither on `frames` nor on its position and is the same
 * bits on every run.  values (may be NULL): [frames][steps] fp64, the NCut BEFORE each step.  steps == 0 leaves x untouched.
 * n <= RCF_NCUT_PACKED_MAX_N (x of a frame sits in LDS); a larger n is RCF_EINVAL before any launch.  workspace: 8-byte aligned. */
#define RCF_NCUT_PACKED_MAX_N 16384
size_t rcf_ncut_refine_packed_workspace_bytes(int frames, int n);
int rcf_ncut_refine_packed_f32(const uint32_t *bits, const int32_t *deg, int n, int frames, float eps, float *x, int steps,
                               float lr, float weight_decay, double *values, void *workspace, size_t workspace_bytes,
                               void *stream);
/* The CRF / NCut-CRF merge (semantic_constraints.py:314-336) of a, b [frames][npix] fp32: counts[f] = |(a > 0.5) xor (b > 0.5)|
 * (the union minus the intersection; int64, written by the call), out[f] = trunc(fl32(fl32(a b) 255)) as u8 -- or
 * trunc(fl32(a 255)) for a frame with counts[f] > umi_th (strict).  umi_th < 0: no threshold.  Two empty masks give the product
 * (the reference's NaN > th is false).  The counts are added with integer atomics: order-independent. */
int rcf_mask_merge_u8(const float *a, const float *b, int frames, long npix, long long umi_th, uint8_t *out, long long *counts,
                      void *stream);

/* ---- PWC-Lite (models/amd/pwc_lite.py; csrc/pwc.hip, the resize adjoint in csrc/spatial.hip) -----------------------------------
 * The pieces between the native convs, rcf_correlation_* and rcf_flow_warp_*.  fp32, no atomics, every sum in a fixed order: the
 * same bits on every call.  Every entry point returns RCF_EINVAL before any launch -- sizes and ranges first, then pointers.
 * hw: pixels of one image (0 < hw < 2^30); 1 <= M <= rcf_pwc_geometry(1) masks; 0 < B <= 65535.
 * rcf_pwc_geometry(which): 0 pixels per workgroup of the pooled sums, 1 the largest M, 2 the largest C of a pooled slice, 3 pixels
 * per workgroup of pack / unpack, 4 the most channels one pack writes; 0 for any other `which`.
 *
 * Segment pooling (get_averge_feat, pwc_lite.py:85-96, all masks at once): feat an NHWC channel slice [B][hw][C] at pixel pitch
 * feat_pitch (C % 4 == 0, 4 <= C <= geometry(2), pitch % 4 == 0, 16-byte aligned), mask planar [B][M][hw]:
 *   pooled[b][m][c] = sum_p feat mask / sum_p mask,  msum[b][m] = sum_p mask      (fp64 sums; a zero sum divides by zero, no guard)
 * partials: rcf_pwc_pool_partials(B, M, C, hw) doubles (RCF_EWORKSPACE when partials_len is less; 0 for a refused shape).
 * Backward, from the forward's pooled and msum:
 *   dfeat[b][p][c] (beta ? += : =) sum_m mask dpooled / msum           (an NHWC slice at dfeat_pitch)
 *   dmask[b][m][p] = (sum_c feat dpooled - sum_c pooled dpooled) / msum */
int rcf_pwc_geometry(int which);
long rcf_pwc_pool_partials(int B, int M, int C, int hw);
int rcf_pwc_segment_pool_fwd_f32(const float *feat, int feat_pitch, const float *mask, float *pooled, float *msum, double *partials,
                                 long partials_len, int B, int M, int C, int hw, void *stream);
int rcf_pwc_segment_pool_bwd_f32(const float *feat, int feat_pitch, const float *mask, const float *pooled, const float *msum,
                                 const float *dpooled, float *dfeat, int dfeat_pitch, int beta, float *dmask, int B, int M, int C, int hw,
                                 void *stream);
/* Segment flow composition: flow[b][c][p] = sum_m mask[b][m][p] group[b][m][c] with group [B][M][2], flow planar [B][2][hw].
 * Backward: dmask[b][m][p] (beta ? += : =) sum_c dflow group (dmask may be NULL: a constant mask), dgroup[b][m][c] = sum_p mask dflow
 * through rcf_pwc_flow_partials(B, M, hw) doubles of partials. */
long rcf_pwc_flow_partials(int B, int M, int hw);
int rcf_pwc_segment_flow_fwd_f32(const float *mask, const float *group, float *flow, int B, int M, int hw, void *stream);
int rcf_pwc_segment_flow_bwd_f32(const float *mask, const float *group, const float *dflow, float *dmask, int beta, float *dgroup,
                                 double *partials, long partials_len, int B, int M, int hw, void *stream);
/* g = dy (y > 0 ? 1 : slope) on `rows` rows of C channels (C % 4 == 0), every tensor at its own pitch (% 4 == 0, >= C), 16-byte
 * aligned; y is the LeakyReLU's OUTPUT (a positive slope keeps the sign), y = +-0 takes the slope. */
int rcf_pwc_leaky_bwd_f32(const float *dy, long dy_pitch, const float *y, long y_pitch, float *g, long g_pitch, long rows, int C,
                          float slope, void *stream);
/* The estimator's input pack: planar corr [B][D][hw] and flow [B][2][hw] -> channels c0 .. c0 + D + 1 of the NHWC buffer
 * buf[B][hw][buf_pitch], then zeros up to the next multiple of 4 (the guard channels of a conv whose Cin % 4 == 0); channels outside
 * that range are left alone.  c0 % 4 == 0, buf_pitch % 4 == 0, at most geometry(4) channels.  rcf_pwc_unpack_f32 is the adjoint:
 * dcorr[b][k][p] = dbuf[b][p][c0 + k], dflow[b][c][p] = dbuf[b][p][c0 + D + c]. */
int rcf_pwc_pack_f32(const float *corr, const float *flow, float *buf, int buf_pitch, int c0, int D, int B, int hw, void *stream);
int rcf_pwc_unpack_f32(const float *dbuf, int buf_pitch, int c0, float *dcorr, float *dflow, int D, int B, int hw, void *stream);
/* The adjoint of rcf_resize_bilinear_nchw_f32 in gather form: dx [planes][Hi][Wi] = R^T dy [planes][Ho][Wo]; either align_corners
 * setting, any size ratio; an input pixel that no output tap names is written as 0. */
int rcf_resize_bilinear_nchw_bwd_f32(const float *dy, float *dx, int planes, int Hi, int Wi, int Ho, int Wo, int align_corners,
                                     void *stream);

/* ---- AMDModel's seam between the tape and the flow network (models/amd/amd_model.py:197-206, models/fcn_head.py:160-170;
 * csrc/amd.hip).  fp32, one pass each, no atomics, no sums across threads: the same bits on every call.  Every entry point returns
 * RCF_EINVAL before any launch -- sizes and ranges first, then pointers.
 * rcf_amd_geometry(which): 0 pixels per workgroup of the softmax kernels, 1 the largest M, 2 the largest I; 0 otherwise.
 * Mask softmax: logits NHWC [B I][hw][pitch] of images n = b I + i (16-byte aligned, pitch % 4 == 0, pitch >= Cp, Cp 4 or 8, the first
 * M <= Cp channels live) -> masks planar and frame-major [I][B][M][hw], masks[i][b][.][p] = softmax_c logits[b I + i][p][c]; frame i is
 * a contiguous [B][M][hw] tensor.  0 < I <= geometry(2), 0 < B, I B <= 65535, 1 <= M <= geometry(1), 0 < hw < 2^30.  A NaN or +inf logit
 * makes the masks of its pixel NaN (torch's softmax).
 * Backward: dmasks is a HOST array of I device pointers, frame i's gradient [B][M][hw] or NULL for zeros;
 *   dlogits[n][p][c] = p_c (dp_c - sum_k p_k dp_k) for c < M, 0 for M <= c < Cp; channels from Cp up to the pitch are left alone.
 * The logits are not read again. */
int rcf_amd_geometry(int which);
int rcf_amd_mask_softmax_fwd_f32(const float *logits, int pitch, float *masks, int I, int B, int M, int Cp, int hw, void *stream);
int rcf_amd_mask_softmax_bwd_f32(const float *masks, const float *const *dmasks, float *dlogits, int pitch, int I, int B, int M, int Cp,
                                 int hw, void *stream);
/* The flow network's input: normalised frames [B][2][3][Hi][Wi] -> two_frame [B][6][Ho][Wo], every channel (x std_c + mean_c) / 255
 * (mean 123.675, 116.28, 103.53; std 58.395, 57.12, 57.375) and THEN bilinear with align_corners = True, on the float32 source
 * positions of rcf_resize_bilinear_nchw_f32.  Sizes 1 .. 2^14, 0 < B <= 65535. */
int rcf_amd_frame_pair_f32(const float *frames, float *out, int B, int Hi, int Wi, int Ho, int Wo, void *stream);

/* ---- Middlebury flow colours for the training visualisation grids (flow_vis.flow_to_color as models/rcf_model.py:222-234 and
 * models/amd/amd_model.py:213-262 call it, once per sample, frame and flow kind on the host; csrc/flowvis.hip).
 * n_images flow images of h x w float32, coloured each by its own maximum radius, in at most two launches whatever n_images is: one
 * where h w <= rcf_flow_color_geometry(0), otherwise a maximum launch (atomic max on the bit pattern of the non-negative radius: the
 * same bits on every call) and a colour launch; no host synchronisation.
 * Layouts are in ELEMENTS of the tensor's own type.  Image n = g group + k (0 <= k < group) starts at g image + k member; channel c
 * (flow: u, v; colours: the three planes), row y and column x add c channel + y row + x col.  So the channel slices [:, :2] / [:, 2:] of
 * a [B, 4, h, w] tensor and an [h, w, 2] array (channel 1, col 2) are read in place, and the planes may go into a window of a wider
 * canvas: `out` points at the window's first element and nothing outside the h x w x 3 elements the layout names is written.  With
 * group > 1 the images of one grid row (the flow kinds of a sample) may sit `member` apart inside a canvas image.  Strides >= 0, col >= 1.
 * out_type: RCF_FLOW_COLOR_U8 bytes 0 .. 255, RCF_FLOW_COLOR_F32 byte / 255 rounded once to float32 (the reference's flow_color / 255.0).
 * convert_to_bgr swaps planes 0 and 2.  clip < 0: none; otherwise u, v <- clamp(., 0, clip) (np.clip(flow, 0, clip_flow)).
 * The package's rad > 1 branch (col * 0.75), dead in exact arithmetic, is never taken.  Non-finite flows (or magnitudes whose squares
 * overflow) make their image's colours meaningless but written in full and equal from call to call; other images are unaffected.
 * 1 <= h, w <= 2^14, 1 <= n_images <= 2^20, n_images % group == 0.  workspace: rcf_flow_color_workspace_bytes() bytes, 4-byte aligned,
 * zeroed in-stream by the call (0 bytes, may be NULL, in the one-launch form; the query returns 0 for a refused shape too).
 * rcf_flow_color_geometry(which): 0 the largest image (pixels) of the one-launch form, 1 pixels per workgroup of the two-launch form. */
#define RCF_FLOW_COLOR_U8 0
#define RCF_FLOW_COLOR_F32 1
typedef struct { long image, member, channel, row, col; } rcf_flow_layout;
int rcf_flow_color_geometry(int which);
size_t rcf_flow_color_workspace_bytes(int n_images, int group, int h, int w);
int rcf_flow_color_f32(const float *flow, const rcf_flow_layout *src, void *out, const rcf_flow_layout *dst, int out_type, int n_images,
                       int group, int h, int w, int convert_to_bgr, float clip, void *workspace, size_t workspace_bytes, void *stream);

/* ---- Evaluation export: every 8-bit RGB panel of a batch in ONE launch (csrc/export.hip; the image side of forward_eval,
 * models/rcf_model.py:241-273,296-315: resize + repeat + save_image's rounding once per sample and channel).
 * Sources.  masks [B][C][h][w] float32 (sample b at b mask_sample ELEMENTS, its C planes contiguous) and frames [B][3][H][W] float32
 * (sample b at b frame_sample elements: a [B, I, 3, H, W] batch's frame 0 is read in place).
 * A panel is Ho x Wo pixels of 3 bytes: its source resized with rcf_resize_bilinear_nchw_f32's arithmetic (the float32 source positions
 * and blend of that entry point, `align_corners` as given), a frame then mapped (v + 2) / 4, and rounded as torchvision.utils.save_image
 * rounds: t = v * 255, t = t + 0.5 (two float32 roundings), clamp to [0, 255], truncate.  A mask's byte goes to all three colours.
 * NaN is written as 0; +inf and every level above 255 as 255, -inf and every level below 0 as 0.  (An infinite source value gives a NaN
 * level where one of its blend weights is 0.)  Bytes are the same from call to call; panels of other planes are unaffected.
 * Destinations.  n_dst (1 .. rcf_export_geometry(3)) layouts, all written by the same launch; strides in BYTES, all >= 0, pixel >= 3.
 * Layout d holds n_slots x B panels: slot j of sample b starts at
 *     base + y row + x pixel + (b / per_row) image_row + (b % per_row) image + j slot,
 * row r and pixel c of it at + r row + c pixel.  source[j] is the mask channel (0 .. C - 1) of slot j, or RCF_EXPORT_FRAME.
 * So {image = Ho Wo 3, per_row >= B, slot = B Ho Wo 3, row = Wo 3, pixel = 3} is a contiguous [n_slots][B][Ho][Wo][3] buffer (all
 * channels, or one), and {x, y = the grid's padding, image / image_row = a grid cell's width / height, slot = Ho row, per_row = 8} the
 * windows of make_grid's canvas with the panels of a sample stacked downwards.  `bytes` is the size of the buffer behind base: a layout
 * whose last panel would end beyond it is refused; nothing outside the panels is written (the caller keeps panels from overlapping).
 * Where pixel == 3 and a run of 4 pixels starts on a dword boundary its 12 bytes are one store; otherwise bytes up to the boundary,
 * whole dwords, and a byte tail.  1 <= B <= 65535, at most 65535 panels per call, sizes 1 .. 2^14.  frames / masks may be NULL when no
 * slot names them.  rcf_export_geometry(which): 0 pixels per thread and run, 1 threads per workgroup, 2 runs per thread (a workgroup
 * takes 0 x 1 x 2 pixels of one panel, runs numbered row-major), 3 the largest n_dst; 0 otherwise. */
#define RCF_EXPORT_MAX_SLOTS 16
#define RCF_EXPORT_FRAME (-1)
typedef struct {
    unsigned char *base;
    long bytes;
    long image, image_row, slot, row, pixel;
    int x, y, per_row, n_slots;
    int source[RCF_EXPORT_MAX_SLOTS];
} rcf_export_layout;
int rcf_export_geometry(int which);
int rcf_export_panels_u8(const float *masks, long mask_sample, int C, int h, int w, const float *frames, long frame_sample, int H, int W,
                         const rcf_export_layout *dst, int n_dst, int B, int Ho, int Wo, int align_corners, void *stream);

#ifdef __cplusplus
}
#endif
#endif /* RCF_HIP_H */
