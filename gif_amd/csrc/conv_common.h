// What the convolution sources (conv_igemm.hip, conv_wgrad.hip, conv_winograd.hip) share beyond common.h: the block
// remap and accumulator types of their kernels, and the host plumbing between a route and its launches.  Not part of the ABI.
#pragma once
#include "common.h"

namespace gif {

typedef float f32x16 __attribute__((ext_vector_type(16)));
typedef float f32x4 __attribute__((ext_vector_type(4)));  // native vector: plain vector loads/stores, never memcpy

// XCD-aware, bijective block remap (cdna guide T1): XCD k (= blockIdx % 8 by dispatch order) gets a contiguous range of logical ids, so
// consecutive logical tiles share an XCD's L2.
__device__ __forceinline__ int xcd_remap(int bid, int nwg) {
    const int nx = 8;
    int xcd = bid % nx, idx = bid / nx;
    int q = nwg / nx, r = nwg % nx;
    int base = xcd < r ? xcd * (q + 1) : r * (q + 1) + (xcd - r) * q;
    return base + idx;
}

// integer value of a GIF_* knob (common.h knob: honoured under GIF_EXPERIMENTAL=1 only), `unset` when it is not given
inline int knob_int(const char* name, int unset) {
    const char* e = knob(name);
    return e ? atoi(e) : unset;
}

// "This kernel may use `lds` bytes of dynamic LDS on the current device", then the launch.  `attr` belongs to ONE kernel instantiation
// (LdsAttr::granted is per kernel): every call site keeps a static of its own per instantiation.
template <typename K, typename P>
void launch_lds(K kern, LdsAttr& attr, dim3 grid, dim3 block, size_t lds, hipStream_t s, const P& p) {
    attr.ensure(reinterpret_cast<const void*>(kern), lds);
    hipLaunchKernelGGL(kern, grid, block, lds, s, p);
}

// the fields of gif_conv_epilogue that every conv parameter struct (GatherParams, WinoParams) carries, with the defaults of a null epilogue
template <typename P>
void fill_epilogue(P& p, const gif_conv_epilogue* e) {
    typedef decltype(p.residual) src_t;  // const void* (element type chosen by the kernel) or const float*
    p.out_scale = e ? e->out_scale : nullptr;
    p.bias = e ? e->bias : nullptr;
    p.residual = e ? static_cast<src_t>(e->residual) : nullptr;
    p.act = e ? e->act : 0;
    p.slope = e ? e->slope : 0.f;
    p.gain = e ? e->gain : 1.f;
    p.mask_src = e ? static_cast<src_t>(e->mask_src) : nullptr;
    p.mask_slope = e ? e->mask_slope : 1.f;
    p.mask_gain = e ? e->mask_gain : 1.f;
    p.dot_src = e ? static_cast<src_t>(e->dot_src) : nullptr;
}

}  // namespace gif
