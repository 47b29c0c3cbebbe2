// Unary energies of the pydenseCRF post-processor (tools/pydenseCRF/crf.py:60-68, :169) from the u8 mask on the device.
// The four host steps -- divide by the frame's maximum, clip, -log(1 - U), -log(U) -- see only two bytes, the frame's maximum
// and the pixel's value, so the caller tabulates them once in float64 ([256][256][2], rounded to fp32: rcf_amd.offline.unary_table)
// and the device copies table entries: unary[f][p][:] = table[max_f][mask[f][p]][:].  No arithmetic on the values, hence the
// host's bits.  Two launches for all frames: the per-frame maximum (as mask_qmax_kernel of crf.hip: a few workgroups per frame,
// one atomicMax each after a relaxed look), then the gather, whose workgroups hold their frame's 2 KB table row in LDS.
//
// Both kernels walk a frame in 16-byte chunks of the MASK'S ADDRESSES, not of the frame's pixel numbers: with an odd npix frame 1
// starts at an odd address, so the chunks start at the 16-byte boundary at or below the frame's first byte and a chunk that
// sticks out of the frame at either end is read byte by byte, inside the frame only.  Every other chunk is one aligned
// 16-byte load per lane.
#include "rcf_common.h"

namespace {

constexpr int UMAX_BLOCKS = 16;                 // workgroups per frame of the maximum pass (480x854: 25 620 chunks, 6 - 7 per lane)
constexpr int UNARY_TILE = 256 * 16;            // pixels per workgroup of the gather: one chunk per lane

// the 16 bytes of chunk [c, c + 16) of a frame (c relative to the frame's first byte, frame + c 16-byte aligned); bytes outside
// [0, npix) read as 0 and are not touched
__device__ __forceinline__ uint4 load_chunk(const uint8_t *__restrict__ frame, long c, long npix) {
    if (c >= 0 && c + 16 <= npix) return *reinterpret_cast<const uint4 *>(frame + c);
    unsigned w[4] = {0u, 0u, 0u, 0u};
    for (int i = 0; i < 16; i++) {
        const long p = c + i;
        if (p >= 0 && p < npix) w[i >> 2] |= (unsigned)frame[p] << (8 * (i & 3));
    }
    return make_uint4(w[0], w[1], w[2], w[3]);
}
__device__ __forceinline__ unsigned max_byte(unsigned m, unsigned w) {
    return max(max(max(m, w & 0xffu), max((w >> 8) & 0xffu, (w >> 16) & 0xffu)), w >> 24);
}

__global__ void __launch_bounds__(256) mask_max_u8_kernel(const uint8_t *__restrict__ mask, long npix, unsigned *__restrict__ qmax) {
    const int f = blockIdx.y;
    const uint8_t *frame = mask + (long)f * npix;
    const long lead = (long)((uintptr_t)frame & 15);                     // bytes between the chunk origin and the frame
    const long chunks = (npix + lead + 15) >> 4;
    unsigned mx = 0u;
    for (long k = (long)blockIdx.x * 256 + threadIdx.x; k < chunks; k += (long)gridDim.x * 256) {
        const uint4 v = load_chunk(frame, k * 16 - lead, npix);
        mx = max_byte(max_byte(max_byte(max_byte(mx, v.x), v.y), v.z), v.w);
    }
    __shared__ unsigned wq[4];
    for (int o = 32; o > 0; o >>= 1) mx = max(mx, (unsigned)__shfl_xor((int)mx, o, 64));
    if ((threadIdx.x & 63) == 0) wq[threadIdx.x >> 6] = mx;
    __syncthreads();
    if (threadIdx.x == 0) {
        const unsigned q = max(max(wq[0], wq[1]), max(wq[2], wq[3]));
        if (q > __hip_atomic_load(qmax + f, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT)) atomicMax(qmax + f, q);
    }
}

// A workgroup takes UNARY_TILE pixels: every lane loads one chunk (16 consecutive pixels) into LDS, then the lanes of a wavefront
// store CONSECUTIVE pixels' float2 pairs (512 contiguous bytes per store instruction), 16 rounds.
__global__ void __launch_bounds__(256) unary_lut_u8_kernel(const uint8_t *__restrict__ mask, long npix,
                                                           const float2 *__restrict__ table, const unsigned *__restrict__ qmax,
                                                           float2 *__restrict__ unary) {
    __shared__ float2 row[256];
    __shared__ uint4 chunk[256];
    const int f = blockIdx.y, t = threadIdx.x;
    const uint8_t *frame = mask + (long)f * npix;
    const long lead = (long)((uintptr_t)frame & 15);
    const long p0 = (long)blockIdx.x * UNARY_TILE - lead;                 // the tile's first pixel (negative: before the frame)
    row[t] = table[(long)min(qmax[f], 255u) * 256 + t];
    chunk[t] = load_chunk(frame, p0 + 16 * t, npix);
    __syncthreads();
    const uint8_t *bytes = reinterpret_cast<const uint8_t *>(chunk);
    float2 *out = unary + (long)f * npix;
#pragma unroll
    for (int j = 0; j < 16; j++) {
        const int q = j * 256 + t;
        const long p = p0 + q;
        if (p >= 0 && p < npix) out[p] = row[bytes[q]];
    }
}

}  // namespace

extern "C" int rcf_crf_unary_lut_u8(const uint8_t *mask, int frames, long npix, const float *table, float *unary, uint32_t *scratch,
                                    void *stream) {
    if (!mask || !table || !unary || !scratch || frames <= 0 || frames > 65535 || npix <= 0) return RCF_EINVAL;
    if ((((uintptr_t)table) | ((uintptr_t)unary)) & 7) return RCF_EINVAL;               // float2 accesses
    const long tiles = (npix + 15 + UNARY_TILE - 1) / UNARY_TILE;                        // + 15: the chunk origin may lie before the frame
    if (tiles * 256 > 0xffffffffL) return RCF_EINVAL;                                    // threads of a launch: 32 bits
    hipStream_t st = rcf_stream(stream);
    if (hipMemsetAsync(scratch, 0, (size_t)frames * sizeof(uint32_t), st) != hipSuccess) return (int)hipGetLastError();
    const long chunks = (npix + 15 + 15) >> 4;
    const int mblocks = (int)(chunks < (long)UMAX_BLOCKS * 256 ? rcf_cdiv(chunks, 256) : UMAX_BLOCKS);
    hipLaunchKernelGGL(mask_max_u8_kernel, dim3(mblocks, frames), dim3(256), 0, st, mask, npix, (unsigned *)scratch);
    hipLaunchKernelGGL(unary_lut_u8_kernel, dim3((unsigned)tiles, frames), dim3(256), 0, st, mask, npix, (const float2 *)table,
                       (const unsigned *)scratch, (float2 *)unary);
    RCF_LAUNCH_CHECK();
    return 0;
}
