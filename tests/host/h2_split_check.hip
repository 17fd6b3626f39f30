// gif::split_pair_h2 (gif_amd/csrc/common.h) on the GPU, for tests/test_gpu_h2_split.py:  h2_split_check FILE
//   sweep   all 2^32 bit patterns of a0 (a1: a fixed bijection of the same pattern) under eight power-of-two scales against ref_split() below,
//           which restates the split one operation per step: multiply, convert, subtract, convert.  hi is compared for every finite a, lo
//           wherever the reference hi is finite (an overflowed hi leaves inf - inf behind).  Once bare, once with the split between two
//           v_mfma_f32_32x32x16_f16 on independent registers at two workgroups of 256 threads per CU.  One line per setting and scale:
//           "sweep <bare|mfma> e <e> hi_cmp N hi_bad N lo_cmp N lo_bad N excluded N nonfinite N" (counts per element)
//   table   FILE holds one "a0 a1 sc" triple of hexadecimal fp32 patterns per line; one line "table <hi dword> <lo dword>" for each
#include <cstdio>
#include <cstring>
#include <vector>

#include "common.h"

typedef float f32x16 __attribute__((ext_vector_type(16)));
typedef unsigned long long u64;

__device__ __forceinline__ void ref_split(const float a, const float sc, unsigned short& hi, unsigned short& lo) {
    // (the empty asm statements pin the four steps: left alone hipcc contracts the subtraction into an FMA and forms hi with
    // v_fma_mixlo_f16 and a +0.0 addend, which turns a = -0 into +0)
    float x = a * sc;
    asm volatile("" : "+v"(x));
    const _Float16 h = (_Float16)x;
    float hf = (float)h;
    asm volatile("" : "+v"(hf));
    float r = x - hf;
    asm volatile("" : "+v"(r));
    const _Float16 l = (_Float16)r;
    hi = __builtin_bit_cast(unsigned short, h);
    lo = __builtin_bit_cast(unsigned short, l);
}

enum { C_HI_CMP = 0, C_HI_BAD, C_LO_CMP, C_LO_BAD, C_EXCL, C_NONFIN, NCNT };
__device__ __forceinline__ void tally(u64* c, const unsigned a_bits, const float sc, const unsigned short gh, const unsigned short gl) {
    if ((a_bits & 0x7f800000u) == 0x7f800000u) { ++c[C_NONFIN]; return; }
    unsigned short rh, rl;
    ref_split(__uint_as_float(a_bits), sc, rh, rl);
    const bool lo_cmp = (rh & 0x7c00u) != 0x7c00u;
    ++c[C_HI_CMP];
    c[C_HI_BAD] += gh != rh;
    c[C_LO_CMP] += lo_cmp;
    c[C_LO_BAD] += lo_cmp && gl != rl;
    c[C_EXCL] += !lo_cmp;
}

template <bool MFMA>
__global__ void __launch_bounds__(256, 2) sweep(const float sc, u64* __restrict__ cnt, float* __restrict__ sink) {
    const unsigned gid = blockIdx.x * 256 + threadIdx.x, stride = gridDim.x * 256;
    u64 c0 = 0, c1 = 0, c2 = 0, c3 = 0, c4 = 0, c5 = 0;
    f32x16 acc0, acc1;
    for (int r = 0; r < 16; ++r) { acc0[r] = 0.f; acc1[r] = 0.f; }
    gif::f16x8_t fa, fb;
    for (int k = 0; k < 8; ++k) { fa[k] = (_Float16)(0.001f * (float)((gid + k) & 15)); fb[k] = (_Float16)(0.002f * (float)((gid * 3 + k) & 7)); }
    for (u64 i = gid; i < (1ull << 32); i += stride) {
        const unsigned b0 = (unsigned)i, b1 = b0 * 0x9E3779B1u + 0x7F4A7C15u;  // (odd multiplier: a1 runs through all patterns as well)
        float a0 = __uint_as_float(b0), a1 = __uint_as_float(b1), s = sc;
        asm volatile("" : "+v"(a0), "+v"(a1), "+v"(s));
        unsigned h, l;
        if constexpr (MFMA) {
            acc0 = __builtin_amdgcn_mfma_f32_32x32x16_f16(fa, fb, acc0, 0, 0, 0);
            __builtin_amdgcn_sched_barrier(0);
            gif::split_pair_h2(a0, a1, s, h, l);
            __builtin_amdgcn_sched_barrier(0);
            acc1 = __builtin_amdgcn_mfma_f32_32x32x16_f16(fb, fa, acc1, 0, 0, 0);
            __builtin_amdgcn_sched_barrier(0);
        } else {
            gif::split_pair_h2(a0, a1, s, h, l);
        }
        u64 c[NCNT] = {0, 0, 0, 0, 0, 0};
        tally(c, b0, sc, (unsigned short)(h & 0xffffu), (unsigned short)(l & 0xffffu));
        tally(c, b1, sc, (unsigned short)(h >> 16), (unsigned short)(l >> 16));
        c0 += c[0]; c1 += c[1]; c2 += c[2]; c3 += c[3]; c4 += c[4]; c5 += c[5];
    }
    atomicAdd(&cnt[0], c0); atomicAdd(&cnt[1], c1); atomicAdd(&cnt[2], c2);
    atomicAdd(&cnt[3], c3); atomicAdd(&cnt[4], c4); atomicAdd(&cnt[5], c5);
    float t = 0.f;
    for (int r = 0; r < 16; ++r) t += acc0[r] + acc1[r];
    if (t == 12345.678f) sink[gid] = t;
}

__global__ void table(const unsigned* __restrict__ in, unsigned* __restrict__ out, const int n) {
    const int i = blockIdx.x * 64 + threadIdx.x;
    if (i >= n) return;
    unsigned h, l;
    gif::split_pair_h2(__uint_as_float(in[3 * i]), __uint_as_float(in[3 * i + 1]), __uint_as_float(in[3 * i + 2]), h, l);
    out[2 * i] = h;
    out[2 * i + 1] = l;
}

#define CHECK(x)                                                                                            \
    do {                                                                                                    \
        hipError_t e_ = (x);                                                                                \
        if (e_ != hipSuccess) { fprintf(stderr, "%s: %s\n", #x, hipGetErrorString(e_)); return 1; }         \
    } while (0)

static int run_sweep() {
    static const int scales[8] = {-126, -113, -30, -1, 0, 13, 30, 126};
    hipDeviceProp_t prop;
    CHECK(hipGetDeviceProperties(&prop, 0));
    const int blocks = prop.multiProcessorCount * 16;
    u64* cnt;
    float* sink;
    CHECK(hipMalloc(&cnt, NCNT * sizeof(u64)));
    CHECK(hipMalloc(&sink, (size_t)blocks * 256 * sizeof(float)));
    for (int mfma = 0; mfma < 2; ++mfma)
        for (int s = 0; s < 8; ++s) {
            const unsigned bits = (unsigned)(scales[s] + 127) << 23;
            float sc;
            memcpy(&sc, &bits, 4);
            CHECK(hipMemset(cnt, 0, NCNT * sizeof(u64)));
            if (mfma) hipLaunchKernelGGL(sweep<true>, dim3(blocks), dim3(256), 0, 0, sc, cnt, sink);
            else hipLaunchKernelGGL(sweep<false>, dim3(blocks), dim3(256), 0, 0, sc, cnt, sink);
            CHECK(hipGetLastError());
            u64 h[NCNT];
            CHECK(hipMemcpy(h, cnt, sizeof(h), hipMemcpyDeviceToHost));
            printf("sweep %s e %d hi_cmp %llu hi_bad %llu lo_cmp %llu lo_bad %llu excluded %llu nonfinite %llu\n", mfma ? "mfma" : "bare", scales[s],
                   h[C_HI_CMP], h[C_HI_BAD], h[C_LO_CMP], h[C_LO_BAD], h[C_EXCL], h[C_NONFIN]);
        }
    CHECK(hipFree(cnt));
    CHECK(hipFree(sink));
    return 0;
}

static int run_table(const char* path) {
    std::vector<unsigned> in;
    FILE* f = fopen(path, "r");
    if (!f) { fprintf(stderr, "cannot open %s\n", path); return 1; }
    unsigned a0, a1, sc;
    while (fscanf(f, "%x %x %x", &a0, &a1, &sc) == 3) { in.push_back(a0); in.push_back(a1); in.push_back(sc); }
    fclose(f);
    const int n = (int)(in.size() / 3);
    if (n == 0) { fprintf(stderr, "%s holds no cases\n", path); return 1; }
    unsigned *d_in, *d_out;
    CHECK(hipMalloc(&d_in, in.size() * sizeof(unsigned)));
    CHECK(hipMalloc(&d_out, (size_t)n * 2 * sizeof(unsigned)));
    CHECK(hipMemcpy(d_in, in.data(), in.size() * sizeof(unsigned), hipMemcpyHostToDevice));
    hipLaunchKernelGGL(table, dim3((n + 63) / 64), dim3(64), 0, 0, d_in, d_out, n);
    CHECK(hipGetLastError());
    std::vector<unsigned> out((size_t)n * 2);
    CHECK(hipMemcpy(out.data(), d_out, out.size() * sizeof(unsigned), hipMemcpyDeviceToHost));
    for (int i = 0; i < n; ++i) printf("table %08x %08x\n", out[2 * i], out[2 * i + 1]);
    CHECK(hipFree(d_in));
    CHECK(hipFree(d_out));
    return 0;
}

int main(int argc, char** argv) {
    if (argc != 2) {
        fprintf(stderr, "usage: h2_split_check FILE\n");
        return 2;
    }
    const int rc = run_sweep();
    return rc ? rc : run_table(argv[1]);
}
