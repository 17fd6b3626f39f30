// What the convolution sources (conv_igemm.hip, conv_wgrad.hip, conv_winograd.hip) share beyond common.h: the block
// remap, accumulator types and split-product order of their kernels, the host plumbing between a route and its launches, and (at the end) the f16x2 row
// exponents of h2_row.h with their wave-level forms.  Not part of the ABI.
#pragma once
#include "common.h"

namespace gif {

typedef float f32x16 __attribute__((ext_vector_type(16)));
typedef float f32x4 __attribute__((ext_vector_type(4)));  // native vector: plain vector loads/stores, never memcpy
// C/D layout of the 32x32 MFMAs: accumulator register r of lane (li, lh) holds column li, row acc_row(r, lh) of the tile
__device__ __forceinline__ constexpr int acc_row(int r, int lh) { return (r & 3) + 8 * (r >> 2) + 4 * lh; }

// XCD-aware, bijective block remap (cdna guide T1): XCD k (= blockIdx % 8 by dispatch order) gets a contiguous range of logical ids, so
// consecutive logical tiles share an XCD's L2.
__device__ __forceinline__ int xcd_remap(int bid, int nwg) {
    const int nx = 8;
    int xcd = bid % nx, idx = bid / nx;
    int q = nwg / nx, r = nwg % nx;
    int base = xcd < r ? xcd * (q + 1) : r * (q + 1) + (xcd - r) * q;
    return base + idx;
}

// order of the split products, smallest terms first: term index of the A and of the B operand of product t.
// f16x2 (terms hi, lo): lo*hi, hi*lo, hi*hi; bf16x3 (hi, mid, lo): lo*hi, hi*lo, mid*mid, mid*hi, hi*mid, hi*hi
struct X3Terms { int a, b; };
template <bool H2>
__device__ __host__ __forceinline__ constexpr X3Terms x3_terms(int t) {
    if constexpr (H2) {
        constexpr int TA3[3] = {1, 0, 0}, TB3[3] = {0, 1, 0};
        return X3Terms{TA3[t], TB3[t]};
    } else {
        constexpr int TA6[6] = {2, 0, 1, 1, 0, 0}, TB6[6] = {0, 2, 1, 0, 1, 0};
        return X3Terms{TA6[t], TB6[t]};
    }
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

// ---- f16x2 row exponents and guard: the per-lane arithmetic (h2_row.h) and its wave-level forms
#define GIF_H2_FN __device__ __host__ __forceinline__
#include "h2_row.h"

namespace gif {

// maximum |v| of the 16 k-values of one group of a row: the lane's own 8 values, then the exchange with the other lane half
__device__ __forceinline__ float h2_group_max(float v0, float v1, float v2, float v3, float v4, float v5, float v6, float v7) {
    float m = fmaxf(fmaxf(fabsf(v0), fabsf(v1)), fabsf(v2));
    m = fmaxf(fmaxf(m, fabsf(v3)), fabsf(v4));
    m = fmaxf(fmaxf(m, fabsf(v5)), fabsf(v6));
    m = fmaxf(m, fabsf(v7));
    const auto sw = __builtin_amdgcn_permlane32_swap(h2_bits(m), h2_bits(m), false, false);
    return fmaxf(__uint_as_float(sw[0]), __uint_as_float(sw[1]));
}
__device__ __forceinline__ float h2_group_max(const float* v) { return h2_group_max(v[0], v[1], v[2], v[3], v[4], v[5], v[6], v[7]); }
__device__ __forceinline__ float h2_group_max(const f32x4& a, const f32x4& b) { return h2_group_max(a[0], a[1], a[2], a[3], b[0], b[1], b[2], b[3]); }
// wave-uniform form: a scalar branch (rare after a row's first groups) around per-lane selects, no EXEC manipulation anywhere near the
// MFMA stream.  `need` is set when some row of the wave changed its exponent: the caller then rescales its accumulators.
__device__ __forceinline__ void h2_observe(int& ex, int& dl, float& sc, float& lim, float& max, unsigned& gmin, float m, bool& need) {
    h2_note(max, gmin, m);
    dl = 0;
    if (__builtin_amdgcn_ballot_w64(m > lim) != 0) {
        h2_grow(ex, dl, sc, lim, m);
        need = true;
    }
}
__device__ __forceinline__ void h2_observe(H2Row& s, float m, bool& need) { h2_observe(s.ex, s.dl, s.sc, s.lim, s.max, s.gmin, m, need); }
// Accumulator register r of a 32x32 MFMA tile holds row acc_row(r, lh) of the tile, whose state lives in the lane of that number:
// f(r, v of that lane) for the 16 registers.  The callers multiply by 2^(exponent change) or go back to the operands' own scale.
template <typename F>
__device__ __forceinline__ void h2_for_rows(int lh, int v, F&& f) {
#pragma unroll
    for (int r = 0; r < 16; ++r) f(r, __builtin_amdgcn_ds_bpermute(acc_row(r, lh) * 4, v));
}

}  // namespace gif
