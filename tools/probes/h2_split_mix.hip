// f16x2 split: can "two floats and a power-of-two scale -> packed hi dword, packed lo dword" be formed with the mixed-precision
// FMAs v_fma_mixlo_f16 / v_fma_mixhi_f16 instead of packed fp32, bit for bit, and is it cheaper beside MFMAs?
//   (P) gif::split_pair_h2 as it stood:  v_pk_mul_f32, v_cvt_pk_f16_f32, 2 v_cvt_f32_f16, v_pk_fma_f32, v_cvt_pk_f16_f32   6 VALU
//   (S) gif::split_pair_h2_scalar as it stood:  2 v_mul_f32, cvt_pk, 2 cvt, 2 v_fma_f32 / v_sub_f32, cvt_pk                8 VALU
//   (C) v_pk_mul_f32 + v_cvt_pk_f16_f32 for hi, mixlo / mixhi for lo                                                        4 VALU
//   (B) mixlo / mixhi with addend -0.0 for hi (neg modifier on the inline constant 0), mixlo / mixhi for lo                 4 VALU
//   (b) as (B), the -0.0 in an SGPR                                                                                         4 VALU
//   (A) 2 v_mul_f32 + v_cvt_pk_f16_f32 for hi, mixlo / mixhi for lo                                                         5 VALU
//   (C') (A') as (C), (A), but lo = f16(x * 1.0 - hi) from the ROUNDED product x = fl32(a * sc) instead of f16(a * sc - hi)  4 / 5 VALU
// Bits: every form against ref_split() below (multiply, convert, subtract, convert, each step pinned) over all 2^32 patterns of a0 (a1: a
// fixed bijection of the same pattern) under eight scales, bare and with the split between two v_mfma_f32_32x32x16_f16 on independent
// registers, two workgroups of 256 threads per CU.  hi is compared for every finite a, lo wherever the reference hi is finite.
// Cycles: the interleave of conv_igemm.hip's glds_body::group (12 MFMAs, LEAD 4, one piece behind each of the next MFMAs, sched_barrier(0)
// pins), operands in registers, two waves per SIMD, s_memtime around the loop and the wall time of the launch; three rounds, arms alternating.
// Build: hipcc -O3 -std=c++17 --offload-arch=gfx950 -o tools/probes/h2_split_mix tools/probes/h2_split_mix.hip
// Run:   tools/probes/h2_split_mix [bits|cycles|all]
#include <hip/hip_runtime.h>
#include <algorithm>
#include <cstdio>
#include <cstring>
#include <vector>
typedef float f32x2 __attribute__((ext_vector_type(2)));
typedef float f32x16 __attribute__((ext_vector_type(16)));
typedef _Float16 f16x2 __attribute__((ext_vector_type(2)));
typedef _Float16 f16x8 __attribute__((ext_vector_type(8)));
typedef unsigned u32x4 __attribute__((ext_vector_type(4)));
typedef unsigned long long u64;

enum { FP = 0, FS, FC, FB, FBS, FA, FC2, FA2, NFORM, FNONE = NFORM };
static const char* kFormName[NFORM + 1] = {"(P) packed, before", "(S) scalar, before", "(C) pk_mul+cvt_pk, mix lo", "(B) mix hi (neg(0)), mix lo",
                                           "(b) mix hi (-0.0 in SGPR), mix lo", "(A) 2 mul+cvt_pk, mix lo", "(C') pk_mul+cvt_pk, mix lo of x",
                                           "(A') 2 mul+cvt_pk, mix lo of x", "(-) no split (MFMAs only)"};

// ---- the reference: the split restated, one operation per step ----------------------------------------------------------------------------
__device__ __forceinline__ void ref_split(const float a, const float sc, unsigned short& hi, unsigned short& lo, float& x, float& r) {
    // (the empty asm statements pin the four steps: left alone hipcc contracts the subtraction into an FMA and, worse, forms hi with
    // v_fma_mixlo_f16 and a +0.0 addend, which turns a = -0 into +0)
    x = a * sc;
    asm volatile("" : "+v"(x));
    const _Float16 h = (_Float16)x;
    float hf = (float)h;
    asm volatile("" : "+v"(hf));
    r = x - hf;
    asm volatile("" : "+v"(r));
    const _Float16 l = (_Float16)r;
    hi = __builtin_bit_cast(unsigned short, h);
    lo = __builtin_bit_cast(unsigned short, l);
}

// ---- the forms --------------------------------------------------------------------------------------------------------------------------
// lo dword = {f16(a1 * sc - h.hi16), f16(a0 * sc - h.lo16)}: one fp32 FMA with an f16 addend and one rounding per element
__device__ __forceinline__ unsigned mix_lo(const float a0, const float a1, const float sc, const unsigned h) {
    unsigned l = 0;
#if defined(__HIP_DEVICE_COMPILE__)
    asm("v_fma_mixlo_f16 %0, %1, %3, -%4 op_sel_hi:[0,0,1]\n\t"
        "v_fma_mixhi_f16 %0, %2, %3, -%4 op_sel:[0,0,1] op_sel_hi:[0,0,1]"
        : "=&v"(l) : "v"(a0), "v"(a1), "v"(sc), "v"(h));
#endif
    return l;
}
// the same from the rounded products x = fl32(a * sc): {f16(x1 - h.hi16), f16(x0 - h.lo16)} — the subtraction of the reference (exact in fp32) and
// its conversion in one instruction; differs from mix_lo only where a * sc is not an fp32 number
__device__ __forceinline__ unsigned mix_lo_x(const float x0, const float x1, const unsigned h) {
    unsigned l = 0;
#if defined(__HIP_DEVICE_COMPILE__)
    asm("v_fma_mixlo_f16 %0, %1, 1.0, -%3 op_sel_hi:[0,0,1]\n\t"
        "v_fma_mixhi_f16 %0, %2, 1.0, -%3 op_sel:[0,0,1] op_sel_hi:[0,0,1]"
        : "=&v"(l) : "v"(x0), "v"(x1), "v"(h));
#endif
    return l;
}
template <int FORM>
__device__ __forceinline__ void split_form(const float a0, const float a1, const float sc, unsigned& hi, unsigned& lo) {
    if constexpr (FORM == FP) {
        // (the two packed instructions as hipcc compiled the first gif::split_pair_h2 inside conv_gather_mfma_glds, spelled out: left to itself
        // it forms the products here with two v_mul_f32)
        const f32x2 a = {a0, a1}, s2 = {sc, sc};
        f32x2 x = a * s2, r;
#if defined(__HIP_DEVICE_COMPILE__)
        asm("v_pk_mul_f32 %0, %1, %2 op_sel_hi:[1,0]" : "=v"(x) : "v"(a), "v"(s2));
#endif
        const f16x2 h = __builtin_convertvector(x, f16x2);
        const f32x2 hf = {(float)h[0], (float)h[1]};
        r = x - hf;
#if defined(__HIP_DEVICE_COMPILE__)
        asm("v_pk_fma_f32 %0, %1, %2, %3 op_sel_hi:[1,0,1] neg_lo:[0,0,1] neg_hi:[0,0,1]" : "=v"(r) : "v"(a), "v"(s2), "v"(hf));
#endif
        hi = __builtin_bit_cast(unsigned, h);
        lo = __builtin_bit_cast(unsigned, __builtin_convertvector(r, f16x2));
    } else if constexpr (FORM == FS) {
        float x0 = a0 * sc;
        asm volatile("" : "+v"(x0));
        const float x1 = a1 * sc;
        const f16x2 h = __builtin_convertvector(f32x2{x0, x1}, f16x2);
        float r0 = x0 - (float)h[0];
        asm volatile("" : "+v"(r0));
        const float r1 = x1 - (float)h[1];
        hi = __builtin_bit_cast(unsigned, h);
        lo = __builtin_bit_cast(unsigned, __builtin_convertvector(f32x2{r0, r1}, f16x2));
    } else if constexpr (FORM == FC) {
        const f32x2 a = {a0, a1}, s2 = {sc, sc};
        f32x2 x = a * s2;
#if defined(__HIP_DEVICE_COMPILE__)
        asm("v_pk_mul_f32 %0, %1, %2 op_sel_hi:[1,0]" : "=v"(x) : "v"(a), "v"(s2));
#endif
        hi = __builtin_bit_cast(unsigned, __builtin_convertvector(x, f16x2));
        lo = mix_lo(a0, a1, sc, hi);
    } else if constexpr (FORM == FA) {
        float x0 = a0 * sc;
        asm volatile("" : "+v"(x0));
        const float x1 = a1 * sc;
        hi = __builtin_bit_cast(unsigned, __builtin_convertvector(f32x2{x0, x1}, f16x2));
        lo = mix_lo(a0, a1, sc, hi);
    } else if constexpr (FORM == FC2) {
        const f32x2 a = {a0, a1}, s2 = {sc, sc};
        f32x2 x = a * s2;
#if defined(__HIP_DEVICE_COMPILE__)
        asm("v_pk_mul_f32 %0, %1, %2 op_sel_hi:[1,0]" : "=v"(x) : "v"(a), "v"(s2));
#endif
        hi = __builtin_bit_cast(unsigned, __builtin_convertvector(x, f16x2));
        lo = mix_lo_x(x[0], x[1], hi);
    } else if constexpr (FORM == FA2) {
        float x0 = a0 * sc;
        asm volatile("" : "+v"(x0));
        const float x1 = a1 * sc;
        hi = __builtin_bit_cast(unsigned, __builtin_convertvector(f32x2{x0, x1}, f16x2));
        lo = mix_lo_x(x0, x1, hi);
    } else if constexpr (FORM == FB) {
        unsigned h = 0, l = 0;  // (one statement: hipcc puts an s_nop in front of every asm statement that follows a VALU instruction)
#if defined(__HIP_DEVICE_COMPILE__)
        asm("v_fma_mixlo_f16 %0, %2, %4, neg(0)\n\t"
            "v_fma_mixhi_f16 %0, %3, %4, neg(0)\n\t"
            "v_fma_mixlo_f16 %1, %2, %4, -%0 op_sel_hi:[0,0,1]\n\t"
            "v_fma_mixhi_f16 %1, %3, %4, -%0 op_sel:[0,0,1] op_sel_hi:[0,0,1]"
            : "=&v"(h), "=&v"(l) : "v"(a0), "v"(a1), "v"(sc));
#endif
        hi = h;
        lo = l;
    } else if constexpr (FORM == FBS) {
        unsigned h = 0, l = 0;
#if defined(__HIP_DEVICE_COMPILE__)
        asm("v_fma_mixlo_f16 %0, %2, %4, %5\n\t"
            "v_fma_mixhi_f16 %0, %3, %4, %5\n\t"
            "v_fma_mixlo_f16 %1, %2, %4, -%0 op_sel_hi:[0,0,1]\n\t"
            "v_fma_mixhi_f16 %1, %3, %4, -%0 op_sel:[0,0,1] op_sel_hi:[0,0,1]"
            : "=&v"(h), "=&v"(l) : "v"(a0), "v"(a1), "v"(sc), "s"(0x80000000u));
#endif
        hi = h;
        lo = l;
    }
}

// ---- bits -------------------------------------------------------------------------------------------------------------------------------
// counters of one (form, scale, setting)
enum { C_HI_CMP = 0, C_HI_BAD, C_LO_CMP, C_LO_BAD, C_EXCL, C_NONFIN, C_NEG0, C_NEG0_BAD, C_SUB32, C_SUB32_BAD, C_LOSUB, C_LOSUB_BAD,
       C_TIEHI, C_TIEHI_BAD, C_TIELO, C_TIELO_BAD, NCNT };
static const char* kCntName[NCNT] = {"hi compared", "hi mismatches", "lo compared", "lo mismatches", "excluded (finite a, reference hi infinite)",
                                     "non-finite a (not compared)", "a = -0", "  mismatches", "a f32-subnormal", "  mismatches",
                                     "reference lo f16-subnormal", "  mismatches", "tie at the hi rounding", "  mismatches",
                                     "tie at the lo rounding", "  mismatches"};
// |v| lies exactly half-way between two neighbouring f16 values (res: what the rounding left, exact)
__device__ __forceinline__ bool is_tie(const float v, const float res) {
    const int ex = (int)((__float_as_uint(v) >> 23) & 0xffu) - 127;
    if (ex >= 16 || res == 0.f) return false;  // (beyond the f16 range every value "rounds" to the maximum or infinity)
    const int qe = ex - 10 < -24 ? -24 : ex - 10;
    return fabsf(res) == __uint_as_float((unsigned)(qe - 1 + 127) << 23);
}
__device__ __forceinline__ void tally(u64* c, const unsigned a_bits, const float sc, const unsigned short gh, const unsigned short gl) {
    if ((a_bits & 0x7f800000u) == 0x7f800000u) { ++c[C_NONFIN]; return; }
    unsigned short rh, rl;
    float x, r;
    ref_split(__uint_as_float(a_bits), sc, rh, rl, x, r);
    const bool hi_bad = gh != rh;
    ++c[C_HI_CMP];
    c[C_HI_BAD] += hi_bad;
    const bool lo_cmp = (rh & 0x7c00u) != 0x7c00u;
    const bool lo_bad = lo_cmp && gl != rl;
    c[C_LO_CMP] += lo_cmp;
    c[C_LO_BAD] += lo_bad;
    c[C_EXCL] += !lo_cmp;
    const bool bad = hi_bad || lo_bad;
    if (a_bits == 0x80000000u) { ++c[C_NEG0]; c[C_NEG0_BAD] += bad; }
    if ((a_bits & 0x7f800000u) == 0 && (a_bits & 0x007fffffu) != 0) { ++c[C_SUB32]; c[C_SUB32_BAD] += bad; }
    if (lo_cmp) {
        if ((rl & 0x7c00u) == 0 && (rl & 0x03ffu) != 0) { ++c[C_LOSUB]; c[C_LOSUB_BAD] += bad; }
        if (is_tie(x, r)) { ++c[C_TIEHI]; c[C_TIEHI_BAD] += bad; }
        const float r2 = r - (float)__builtin_bit_cast(_Float16, rl);
        if (is_tie(r, r2)) { ++c[C_TIELO]; c[C_TIELO_BAD] += bad; }
    }
}
template <int FORM, bool MFMA>
__global__ void __launch_bounds__(256, 2) sweep(const float sc, u64* __restrict__ cnt, float* __restrict__ sink) {
    const unsigned gid = blockIdx.x * 256 + threadIdx.x, stride = gridDim.x * 256;
    u64 c[NCNT];
    for (int k = 0; k < NCNT; ++k) c[k] = 0;
    f32x16 acc0, acc1;
    for (int r = 0; r < 16; ++r) { acc0[r] = 0.f; acc1[r] = 0.f; }
    f16x8 fa, fb;
    for (int k = 0; k < 8; ++k) { fa[k] = (_Float16)(0.001f * (float)((gid + k) & 15)); fb[k] = (_Float16)(0.002f * (float)((gid * 3 + k) & 7)); }
    for (u64 i = gid; i < (1ull << 32); i += stride) {
        const unsigned b0 = (unsigned)i, b1 = b0 * 0x9E3779B1u + 0x7F4A7C15u;  // (odd multiplier: a1 runs through all patterns as well)
        float a0 = __uint_as_float(b0), a1 = __uint_as_float(b1), s = sc;
        asm volatile("" : "+v"(a0), "+v"(a1), "+v"(s));
        unsigned h, l;
        if constexpr (MFMA) {
            acc0 = __builtin_amdgcn_mfma_f32_32x32x16_f16(fa, fb, acc0, 0, 0, 0);
            __builtin_amdgcn_sched_barrier(0);
            split_form<FORM>(a0, a1, s, h, l);
            __builtin_amdgcn_sched_barrier(0);
            acc1 = __builtin_amdgcn_mfma_f32_32x32x16_f16(fb, fa, acc1, 0, 0, 0);
            __builtin_amdgcn_sched_barrier(0);
        } else {
            split_form<FORM>(a0, a1, s, h, l);
        }
        tally(c, b0, sc, (unsigned short)(h & 0xffffu), (unsigned short)(l & 0xffffu));
        tally(c, b1, sc, (unsigned short)(h >> 16), (unsigned short)(l >> 16));
    }
    for (int k = 0; k < NCNT; ++k)
        if (c[k]) atomicAdd(&cnt[k], c[k]);
    float t = 0.f;
    for (int r = 0; r < 16; ++r) t += acc0[r] + acc1[r];
    if (t == 12345.678f) sink[gid] = t;
}

// ---- cycles -----------------------------------------------------------------------------------------------------------------------------
constexpr int kGroups = 512;  // 12-MFMA groups per wave and launch
template <int FORM>
__global__ void __launch_bounds__(256, 2) cycles(const float* __restrict__ in, u64* __restrict__ ticks, float* __restrict__ sink) {
    const int gid = blockIdx.x * 256 + threadIdx.x;
    f32x2 ra[4];  // (pairs in adjacent registers, as the kernels' f32x4 LDS reads leave them: the packed forms stay packed)
    for (int k = 0; k < 8; ++k) ra[k / 2][k % 2] = in[(gid * 8 + k) & 65535];
    float sc = __uint_as_float((unsigned)(127 + 8 + (in[gid & 65535] > 0.f ? 1 : 0)) << 23);  // per-lane, as h_sc in the kernels
    f32x16 acc[4];
    for (int j = 0; j < 4; ++j)
        for (int r = 0; r < 16; ++r) acc[j][r] = 0.f;
    u32x4 sa[2][2], sb[2][4];
    for (int t = 0; t < 2; ++t)
        for (int j = 0; j < 4; ++j)
            for (int e = 0; e < 4; ++e) {
                const f16x2 v = {(_Float16)(0.001f * (float)((gid + e + j) & 7)), (_Float16)(0.0005f * (float)((gid * 5 + e + t) & 7))};
                sb[t][j][e] = __builtin_bit_cast(unsigned, v);
            }
    for (int s = 0; s < 2; ++s)
        for (int t = 0; t < 2; ++t)
            for (int e = 0; e < 4; ++e) sa[s][t][e] = sb[t][s][e];
    auto group = [&](const int slot, const int nslot) __attribute__((always_inline)) {
        constexpr int TA3[3] = {1, 0, 0}, TB3[3] = {0, 1, 0};
        constexpr int LEAD = 4;
        int n = 0, piece = -1;  // (piece -1: the slot of the kernels' tracking step, left empty here)
#pragma unroll
        for (int t = 0; t < 3; ++t)
#pragma unroll
            for (int j = 0; j < 4; ++j) {
                acc[j] = __builtin_amdgcn_mfma_f32_32x32x16_f16(__builtin_bit_cast(f16x8, sa[slot][TA3[t]]), __builtin_bit_cast(f16x8, sb[TB3[t]][j]),
                                                                acc[j], 0, 0, 0);
                __builtin_amdgcn_sched_barrier(0);
                ++n;
                if (n >= LEAD && piece < 4) {
                    if (piece >= 0) {
                        if constexpr (FORM != FNONE) {
                            asm volatile("" : "+v"(ra[piece]));  // (fresh values as far as the compiler knows: nothing is hoisted)
                            unsigned h, l;
                            split_form<FORM>(ra[piece][0], ra[piece][1], sc, h, l);
                            sa[nslot][0][piece] = h;
                            sa[nslot][1][piece] = l;
                        }
                    }
                    ++piece;
                    __builtin_amdgcn_sched_barrier(0);
                }
            }
    };
    const u64 t0 = __builtin_amdgcn_s_memtime();
    asm volatile("s_waitcnt lgkmcnt(0)" ::: "memory");
    __builtin_amdgcn_sched_barrier(0);
    for (int it = 0; it < kGroups / 2; ++it) {
        group(0, 1);
        group(1, 0);
    }
    __builtin_amdgcn_sched_barrier(0);
    const u64 t1 = __builtin_amdgcn_s_memtime();
    asm volatile("s_waitcnt lgkmcnt(0)" ::: "memory");
    if ((threadIdx.x & 63) == 0) ticks[gid >> 6] = t1 - t0;
    float t = 0.f;
    for (int j = 0; j < 4; ++j)
        for (int r = 0; r < 16; ++r) t += acc[j][r];
    if (t == 12345.678f) sink[gid] = t;
}

// ---- host -------------------------------------------------------------------------------------------------------------------------------
#define CHECK(x)                                                                                   \
    do {                                                                                           \
        hipError_t e_ = (x);                                                                       \
        if (e_ != hipSuccess) { printf("%s: %s\n", #x, hipGetErrorString(e_)); return 1; }         \
    } while (0)
static const int kScales[8] = {-126, -113, -30, -1, 0, 13, 30, 126};
static float pow2f(int e) { unsigned b = (unsigned)(e + 127) << 23; float f; memcpy(&f, &b, 4); return f; }

template <int FORM, bool MFMA>
static int run_sweep(int blocks, u64* d_cnt, float* sink, u64 (*tot)[NCNT]) {
    for (int s = 0; s < 8; ++s) {
        CHECK(hipMemset(d_cnt, 0, NCNT * sizeof(u64)));
        hipLaunchKernelGGL((sweep<FORM, MFMA>), dim3(blocks), dim3(256), 0, 0, pow2f(kScales[s]), d_cnt, sink);
        CHECK(hipGetLastError());
        CHECK(hipMemcpy(tot[s], d_cnt, NCNT * sizeof(u64), hipMemcpyDeviceToHost));
    }
    return 0;
}
static int report_sweep(int form, bool mfma, u64 (*tot)[NCNT]) {
    u64 bad = 0;
    for (int s = 0; s < 8; ++s) bad += tot[s][C_HI_BAD] + tot[s][C_LO_BAD];
    printf("%-36s %-18s total mismatches %llu %s\n", kFormName[form], mfma ? "between two MFMAs" : "bare", bad, bad ? "OUT" : "ok");
    printf("    %-44s", "scale 2^e, e =");
    for (int s = 0; s < 8; ++s) printf(" %11d", kScales[s]);
    printf("\n");
    for (int k = 0; k < NCNT; ++k) {
        printf("    %-44s", kCntName[k]);
        for (int s = 0; s < 8; ++s) printf(" %11llu", tot[s][k]);
        printf("\n");
    }
    return bad != 0;
}
template <int FORM>
static int run_bits(int blocks, u64* d_cnt, float* sink, int* out) {
    static u64 tot[8][NCNT];
    if (run_sweep<FORM, false>(blocks, d_cnt, sink, tot)) return 1;
    out[FORM] |= report_sweep(FORM, false, tot);
    if (run_sweep<FORM, true>(blocks, d_cnt, sink, tot)) return 1;
    out[FORM] |= report_sweep(FORM, true, tot);
    return 0;
}
template <int FORM>
static int run_cycles(int blocks, const float* in, u64* d_ticks, float* sink, double* cyc, double* ms) {
    hipEvent_t e0, e1;
    CHECK(hipEventCreate(&e0));
    CHECK(hipEventCreate(&e1));
    hipLaunchKernelGGL((cycles<FORM>), dim3(blocks), dim3(256), 0, 0, in, d_ticks, sink);  // warm-up
    CHECK(hipDeviceSynchronize());
    CHECK(hipEventRecord(e0));
    hipLaunchKernelGGL((cycles<FORM>), dim3(blocks), dim3(256), 0, 0, in, d_ticks, sink);
    CHECK(hipEventRecord(e1));
    CHECK(hipEventSynchronize(e1));
    float t;
    CHECK(hipEventElapsedTime(&t, e0, e1));
    std::vector<u64> h(blocks * 4);
    CHECK(hipMemcpy(h.data(), d_ticks, h.size() * sizeof(u64), hipMemcpyDeviceToHost));
    std::sort(h.begin(), h.end());
    *cyc = (double)h[h.size() / 2] / kGroups;  // median over the waves
    *ms = t;
    CHECK(hipEventDestroy(e0));
    CHECK(hipEventDestroy(e1));
    return 0;
}

int main(int argc, char** argv) {
    const bool bits = argc < 2 || !strcmp(argv[1], "bits") || !strcmp(argv[1], "all");
    const bool cyc = argc < 2 || !strcmp(argv[1], "cycles") || !strcmp(argv[1], "all");
    hipDeviceProp_t prop;
    CHECK(hipGetDeviceProperties(&prop, 0));
    const int cus = prop.multiProcessorCount;
    printf("%s, %d CUs\n", prop.gcnArchName, cus);
    float *in, *sink;
    u64 *d_cnt, *d_ticks;
    std::vector<float> h(65536);
    for (int i = 0; i < 65536; ++i) h[i] = (float)((i * 2654435761u) >> 8 & 0xFFFF) / 4096.f - 8.f;
    CHECK(hipMalloc(&in, 65536 * 4));
    CHECK(hipMalloc(&sink, (size_t)cus * 16 * 256 * 4));
    CHECK(hipMalloc(&d_cnt, NCNT * sizeof(u64)));
    CHECK(hipMalloc(&d_ticks, (size_t)cus * 2 * 4 * sizeof(u64)));
    CHECK(hipMemcpy(in, h.data(), 65536 * 4, hipMemcpyHostToDevice));
    int out[NFORM] = {};
    if (bits) {
        printf("\n== bits: all 2^32 patterns of a0 (a1 = a0 * 0x9E3779B1 + 0x7F4A7C15 as a pattern), counts per element ==\n");
        const int blocks = cus * 16;
        if (run_bits<FP>(blocks, d_cnt, sink, out) || run_bits<FS>(blocks, d_cnt, sink, out) || run_bits<FC>(blocks, d_cnt, sink, out) ||
            run_bits<FB>(blocks, d_cnt, sink, out) || run_bits<FBS>(blocks, d_cnt, sink, out) || run_bits<FA>(blocks, d_cnt, sink, out) ||
            run_bits<FC2>(blocks, d_cnt, sink, out) || run_bits<FA2>(blocks, d_cnt, sink, out))
            return 1;
        printf("\nsurvivors:");
        for (int f = 0; f < NFORM; ++f)
            if (!out[f]) printf("  %s;", kFormName[f]);
        printf("\n");
    }
    if (cyc) {
        printf("\n== cycles per 12-MFMA group (median over %d waves, %d groups each; two workgroups of 256 per CU), wall ms of the launch ==\n",
               cus * 2 * 4, kGroups);
        double c[3][NFORM + 1], ms[3][NFORM + 1];
        for (int r = 0; r < 3; ++r) {
            if (run_cycles<FP>(cus * 2, in, d_ticks, sink, &c[r][FP], &ms[r][FP]) || run_cycles<FS>(cus * 2, in, d_ticks, sink, &c[r][FS], &ms[r][FS]) ||
                run_cycles<FC>(cus * 2, in, d_ticks, sink, &c[r][FC], &ms[r][FC]) || run_cycles<FB>(cus * 2, in, d_ticks, sink, &c[r][FB], &ms[r][FB]) ||
                run_cycles<FBS>(cus * 2, in, d_ticks, sink, &c[r][FBS], &ms[r][FBS]) ||
                run_cycles<FA>(cus * 2, in, d_ticks, sink, &c[r][FA], &ms[r][FA]) ||
                run_cycles<FC2>(cus * 2, in, d_ticks, sink, &c[r][FC2], &ms[r][FC2]) ||
                run_cycles<FA2>(cus * 2, in, d_ticks, sink, &c[r][FA2], &ms[r][FA2]) ||
                run_cycles<FNONE>(cus * 2, in, d_ticks, sink, &c[r][FNONE], &ms[r][FNONE]))
                return 1;
        }
        printf("%-36s %27s %10s   %27s\n", "form", "cycles / group, rounds 1-3", "spread", "wall ms, rounds 1-3");
        for (int f = 0; f <= NFORM; ++f) {
            const double lo = std::min(c[0][f], std::min(c[1][f], c[2][f])), hi = std::max(c[0][f], std::max(c[1][f], c[2][f]));
            printf("%-36s %8.1f %8.1f %8.1f %10.1f   %8.3f %8.3f %8.3f\n", kFormName[f], c[0][f], c[1][f], c[2][f], hi - lo, ms[0][f], ms[1][f],
                   ms[2][f]);
        }
    }
    return 0;
}
