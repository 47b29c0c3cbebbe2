// The one copy of the bilinear resize's arithmetic that csrc/spatial.hip and csrc/amd.hip share: the float32 source position of an
// output index, the scale it is taken with, and the blend of the four taps.  The library is compiled without contraction, so the same
// lines give the same bits in every kernel that includes them.
#pragma once
#include "rcf_common.h"

namespace {

// PyTorch area_pixel_compute_source_index (UpSample.h): align_corners ? scale*dst
//   : max(scale*(dst+0.5)-0.5, 0); scale = align ? (in-1)/(out-1) : in/out.
__device__ __forceinline__ void src_index(int dst, float scale, int align, int in_size, int &i0, int &i1, float &l1) {
    float s = align ? scale * dst : fmaxf(scale * (dst + 0.5f) - 0.5f, 0.f);
    i0 = (int)s;
    if (i0 > in_size - 1) i0 = in_size - 1;
    i1 = i0 + (i0 < in_size - 1 ? 1 : 0);
    l1 = s - i0;
}
inline float host_scale(int in, int out, int align) {
    if (align) return out > 1 ? (float)(in - 1) / (float)(out - 1) : 0.f;
    return (float)in / (float)out;
}

// the bilinear blend, the horizontal blends of the two source rows first: ONE expression tree for every resize of the library
// (the exact-2x kernels of spatial.hip share its halves between outputs)
__device__ __forceinline__ float blend(float hy, float ly, float hx, float lx, float v00, float v01, float v10, float v11) {
    return hy * (hx * v00 + lx * v01) + ly * (hx * v10 + lx * v11);
}

}  // namespace
