// f16x2 ("h2", common.h): the ONE implementation of the running row exponent and the guard's "window" statistics that the f16x2
// kernels (conv_igemm.hip glds_body / conv3x3_rows_thin_h2, conv_wgrad.hip conv_wgrad_mfma / conv_wgrad_h2v2, conv_winograd.hip
// wino_gemm_h2) and the two f16x2 weight packers share.  Not part of the ABI.
// Plain per-lane arithmetic, for the device and for the host: the including file says how the functions are declared by defining
// GIF_H2_FN first (conv_common.h: __device__ __host__ __forceinline__, and the wave-level forms on top of this file — group maximum,
// wave-uniform observe, accumulator-row broadcast; tests/host/h2_row_check.cpp, which includes this file alone: inline).
#pragma once
#include <math.h>

namespace gif {

constexpr int kH2Target = 13;        // activations: a new row maximum lands in [2^13, 2^14)
constexpr int kH2TargetW = 14;       // weights (static): the row maximum lands in [2^14, 2^15)
constexpr float kH2Limit = 65472.f;  // rescale before |x| * 2^e reaches the f16 overflow threshold (65520)
constexpr int kH2Window = 14;        // activations: exponent-field distance (row maximum, smallest non-zero group maximum) allowed
constexpr int kH2WindowW = 16;       // weights: one binade more headroom comes from the tighter scaling target

GIF_H2_FN unsigned h2_bits(float v) { return __builtin_bit_cast(unsigned, v); }
// exponent e with m * 2^e in [2^target, 2^(target+1)), clamped to what a float scale factor can hold
GIF_H2_FN int h2_exp_for(unsigned m_bits, int target) {
    const int e = target + 127 - (int)((m_bits >> 23) & 0xffu);
    return e > 126 ? 126 : (e < -126 ? -126 : e);
}
GIF_H2_FN constexpr float h2_pow2(int e) { return __builtin_bit_cast(float, (unsigned)(e + 127) << 23); }  // -126 <= e <= 127

// State of one GEMM row (lanes li and li + 32 of a wave feed the same row and agree): exponent, its pending change, the float 2^ex,
// the largest |a| the exponent can take, and the guard's statistics (row maximum, smallest non-zero group maximum as bits - 1).
// The functions below exist on the FIELDS as well (a kernel that indexes its rows by a value that is a constant only after unrolling,
// conv_wgrad_mfma, keeps one array per field: an array of H2Row costs it registers, or scratch memory).
struct H2Row {
    int ex = 126, dl = 0;
    float sc = h2_pow2(126), lim = kH2Limit * h2_pow2(-126), max = 0.f;
    unsigned gmin = 0xFFFFFFFFu;
};
// window statistics of one 16-element K group with maximum m
GIF_H2_FN void h2_note(float& max, unsigned& gmin, float m) {
    max = fmaxf(max, m);
    gmin = __builtin_elementwise_min(gmin, h2_bits(m) - 1u);  // an all-zero group (0 - 1 = 0xffffffff) never wins
}
GIF_H2_FN void h2_note(H2Row& s, float m) { h2_note(s.max, s.gmin, m); }
// THE exponent rule: a row that outgrew its exponent (m > lim) takes the one that puts m into [2^kH2Target, 2^(kH2Target+1)); every
// other row keeps its own (a select, so that lanes of a wave can run it together)
GIF_H2_FN void h2_grow(int& ex, int& dl, float& sc, float& lim, float m) {
    const int ne = m > lim ? h2_exp_for(h2_bits(m), kH2Target) : ex;
    dl = ne - ex;
    ex = ne;
    sc = h2_pow2(ne);
    lim = ldexpf(kH2Limit, -ne);
}
GIF_H2_FN void h2_grow(H2Row& s, float m) { h2_grow(s.ex, s.dl, s.sc, s.lim, m); }
// private form (a thread owns its row: plain divergence): two groups under one decision; true when the exponent changed
GIF_H2_FN bool h2_observe_private(H2Row& s, float m0, float m1) {
    const float m = fmaxf(m0, m1);
    s.max = fmaxf(s.max, m);
    s.gmin = __builtin_elementwise_min(s.gmin, __builtin_elementwise_min(h2_bits(m0) - 1u, h2_bits(m1) - 1u));
    s.dl = 0;
    if (m > s.lim) {
        h2_grow(s, m);
        return true;
    }
    return false;
}
// guard: one of the row's 16-element K groups lies more than 2^kH2Window below the row maximum (its values no longer carry 22 bits)
GIF_H2_FN bool h2_wide(float max, unsigned gmin) { return (int)(h2_bits(max) >> 23) - (int)((gmin + 1u) >> 23) > kH2Window; }
GIF_H2_FN bool h2_wide(const H2Row& s) { return h2_wide(s.max, s.gmin); }
// weight side (static rows, chosen by the packing kernels): the row's exponent from its maximum, and the row's flag: a non-zero
// group whose maximum gm lies more than 2^kH2WindowW below the row maximum makes the row `narrow`
GIF_H2_FN int h2_weight_exp(float rowmax) { return h2_exp_for(h2_bits(rowmax), kH2TargetW); }
GIF_H2_FN void h2_weight_note(float rowmax, float gm, bool& narrow) {
    if (gm > 0.f && (int)(h2_bits(rowmax) >> 23) - (int)(h2_bits(gm) >> 23) > kH2WindowW) narrow = true;
}

}  // namespace gif
