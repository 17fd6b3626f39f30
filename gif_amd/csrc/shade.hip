// Deferred shading of the FLAME condition's texture render for gfx950: per covered pixel, the albedo texture
// sampled at the rasterised UV coordinate times second-order spherical-harmonics irradiance of the rasterised normal
// (Ramamoorthi & Hanrahan 2001; the form DECA's 9 x 3 light codes are written for).  The renderer that does this in the
// reference sits in its absent `photometric_optimization` submodule, so there is no line to cite: the definition is the one in
// include/gif_hip.h, restated in float64 by tests/shading_ref.py.
//
// Both kernels are pointwise over pixels, one lane per pixel of planar NCHW images (every load and store of a wave is one
// contiguous 256-byte row segment), one workgroup inside ONE sample: the sample's 27 light coefficients have a wave-uniform
// address and arrive in scalar registers; the constants k_i are folded into the per-lane basis.  The albedo taps are gathers
// (screen-coherent UVs keep them in L2).
//   forward   256 pixels per workgroup; 33 bytes of HBM per pixel (uv 8, normal 12, mask 1, out 12).
//   backward  1024 pixels per workgroup (four coalesced rounds per lane, so the 27-value wave reduction is paid once per four
//             pixels): g_uv and g_nrm pointwise; g_sh as one partial row per workgroup (xor butterfly over the wave, the four
//             waves through LDS in wave order) summed by gif::reduce_partials in a fixed order; g_albedo by fp32 atomicAdd of
//             the four taps of each channel — the ONE non-deterministic output, computed only when asked for.
#include "common.h"

#pragma clang fp contract(off)  // one rounding sequence whichever outputs a launch computes; the FMAs below are explicit

namespace {

// k_i = A_l * Y_lm, A = (1, 2 pi / 3, pi / 4) (DECA's table: band 0's factor pi is left to the light code):  1/sqrt(4 pi);  (2 pi / 3) sqrt(3 / (4 pi));  (pi / 4) 3 sqrt(5 / (12 pi));
// (pi / 4) (3 / 2) sqrt(5 / (12 pi));  (pi / 4) (1 / 2) sqrt(5 / (4 pi))
constexpr float kK0 = (float)0.28209479177387814;
constexpr float kK1 = (float)1.0233267079464883;
constexpr float kK2 = (float)0.8580855308097834;
constexpr float kK7 = (float)0.4290427654048917;
constexpr float kK8 = (float)0.24770795610037571;

constexpr int kBwdRounds = 4;  // pixels per lane of the backward kernel

// k_i * basis_i(n), basis = (1, x, y, z, xy, xz, yz, x^2 - y^2, 3 z^2 - 1)
__device__ __forceinline__ void sh_basis(float x, float y, float z, float kb[9]) {
    kb[0] = kK0;
    kb[1] = kK1 * x;
    kb[2] = kK1 * y;
    kb[3] = kK1 * z;
    kb[4] = kK2 * (x * y);
    kb[5] = kK2 * (x * z);
    kb[6] = kK2 * (y * z);
    kb[7] = kK7 * ((x - y) * (x + y));
    kb[8] = kK8 * fmaf(3.f * z, z, -1.f);
}

// One axis of grid_sample(bilinear, zeros, align_corners=False): texel position ((g + 1) T - 1) / 2, its cell f = floor and
// fraction a; ok0 / ok1: taps f and f + 1 lie in [0, T - 1].  Float comparisons: a NaN coordinate fails all of them ("outside").
struct Axis {
    float f, a;
    bool ok0, ok1;
};
__device__ __forceinline__ Axis axis_of(float g, int T) {
    const float i = ((g + 1.f) * (float)T - 1.f) * 0.5f;
    Axis r;
    r.f = floorf(i);
    r.a = i - r.f;
    r.ok0 = r.f >= 0.f && r.f <= (float)(T - 1);
    r.ok1 = r.f >= -1.f && r.f <= (float)(T - 2);
    return r;
}

struct Cell {
    long i00;                  // offset of tap (y0, x0) inside a T x T plane (negative where y0 or x0 is -1: only the taps
                               // whose flag is set are addressed, and those add T and / or 1 back)
    bool t00, t01, t10, t11;   // tap (y, x) inside the texture
    float w00, w01, w10, w11;  // bilinear weights (0 for a tap outside)
    float ax, ay;
};
__device__ __forceinline__ Cell cell_of(float gx, float gy, int T) {
    const Axis X = axis_of(gx, T), Y = axis_of(gy, T);
    Cell c;
    c.ax = X.a; c.ay = Y.a;
    c.t00 = X.ok0 && Y.ok0; c.t01 = X.ok1 && Y.ok0; c.t10 = X.ok0 && Y.ok1; c.t11 = X.ok1 && Y.ok1;
    c.w00 = c.t00 ? (1.f - X.a) * (1.f - Y.a) : 0.f;
    c.w01 = c.t01 ? X.a * (1.f - Y.a) : 0.f;
    c.w10 = c.t10 ? (1.f - X.a) * Y.a : 0.f;
    c.w11 = c.t11 ? X.a * Y.a : 0.f;
    // (any in-range tap implies f >= -1 on both axes, so the conversions are of small integers wherever i00 is used)
    const long x0 = (X.ok0 || X.ok1) ? (long)X.f : 0, y0 = (Y.ok0 || Y.ok1) ? (long)Y.f : 0;
    c.i00 = y0 * (long)T + x0;
    return c;
}

// the four taps of one channel plane (0 for a tap outside: nothing is read there)
__device__ __forceinline__ void taps_of(const float* __restrict__ plane, const Cell& c, int T, float t[4]) {
    t[0] = c.t00 ? plane[c.i00] : 0.f;
    t[1] = c.t01 ? plane[c.i00 + 1] : 0.f;
    t[2] = c.t10 ? plane[c.i00 + T] : 0.f;
    t[3] = c.t11 ? plane[c.i00 + T + 1] : 0.f;
}
__device__ __forceinline__ float bilinear(const Cell& c, const float t[4]) {
    return fmaf(c.w11, t[3], fmaf(c.w10, t[2], fmaf(c.w01, t[1], c.w00 * t[0])));
}
__device__ __forceinline__ float shading_of(const float kb[9], const float* __restrict__ shb, int ch) {
    float s = kb[0] * shb[ch];
#pragma unroll
    for (int i = 1; i < 9; ++i) s = fmaf(kb[i], shb[3 * i + ch], s);
    return s;
}

__global__ void __launch_bounds__(256) shade_sh_kernel(const float* __restrict__ uv, const float* __restrict__ nrm,
                                                       const uint8_t* __restrict__ mask, const float* __restrict__ albedo,
                                                       const float* __restrict__ sh, float* __restrict__ out, int HW, int nblk,
                                                       int per_sample_albedo, int T, float nrm_mul, float nrm_add) {
    const int b = blockIdx.x / nblk, blk = blockIdx.x - b * nblk;
    const int p = blk * 256 + (int)threadIdx.x;
    if (p >= HW) return;
    const int base = b * 3 * HW + p;  // (B * 3 * H * W < 2^31 is checked by the entry point)
    float o[3] = {0.f, 0.f, 0.f};
    if (mask[b * HW + p]) {
        const float* shb = sh + b * 27;
        float kb[9];
        sh_basis(nrm_mul * nrm[base] + nrm_add, nrm_mul * nrm[base + HW] + nrm_add, nrm_mul * nrm[base + 2 * HW] + nrm_add, kb);
        const Cell c = cell_of(uv[base], uv[base + HW], T);
        const float* al = albedo + (size_t)(per_sample_albedo ? b : 0) * 3 * T * T;
#pragma unroll
        for (int ch = 0; ch < 3; ++ch) {
            float t[4];
            taps_of(al + (size_t)ch * T * T, c, T, t);
            o[ch] = bilinear(c, t) * shading_of(kb, shb, ch);
        }
    }
    out[base] = o[0];
    out[base + HW] = o[1];
    out[base + 2 * HW] = o[2];
}

struct ShadeBwd {
    const float *uv, *nrm, *albedo, *sh, *g_out;
    const uint8_t* mask;
    float *g_uv, *g_nrm, *g_albedo, *part;  // each may be null; part [B][nblk][27]
    int HW, nblk, per_sample_albedo, T;
    float nrm_mul, nrm_add;
};

__global__ void __launch_bounds__(256) shade_sh_bwd_kernel(const ShadeBwd a) {
    __shared__ float red[4][27];
    const int b = blockIdx.x / a.nblk, blk = blockIdx.x - b * a.nblk;
    const int HW = a.HW, T = a.T;
    const float* __restrict__ shb = a.sh + b * 27;
    const size_t plane = (size_t)T * T, abase = (size_t)(a.per_sample_albedo ? b : 0) * 3 * plane;
    const bool want_n = a.g_nrm != nullptr, want_sh = a.part != nullptr;
    float acc[27];
#pragma unroll
    for (int k = 0; k < 27; ++k) acc[k] = 0.f;
#pragma unroll 1
    for (int r = 0; r < kBwdRounds; ++r) {
        const int p = (blk * kBwdRounds + r) * 256 + (int)threadIdx.x;
        if (p >= HW) break;  // (later rounds lie further out)
        const int base = b * 3 * HW + p;
        float gu = 0.f, gv = 0.f, gn[3] = {0.f, 0.f, 0.f};
        if (a.mask[b * HW + p]) {
            const float x = a.nrm_mul * a.nrm[base] + a.nrm_add, y = a.nrm_mul * a.nrm[base + HW] + a.nrm_add,
                        z = a.nrm_mul * a.nrm[base + 2 * HW] + a.nrm_add;
            float kb[9];
            sh_basis(x, y, z, kb);
            const Cell c = cell_of(a.uv[base], a.uv[base + HW], T);
            float gs[3];  // dL / d shading_c = g_c * a_c
            float dax = 0.f, day = 0.f;
#pragma unroll
            for (int ch = 0; ch < 3; ++ch) {
                float t[4];
                taps_of(a.albedo + abase + (size_t)ch * plane, c, T, t);
                const float g = a.g_out[base + ch * HW];
                gs[ch] = g * bilinear(c, t);
                const float ga = g * shading_of(kb, shb, ch);  // dL / d a_c
                // d a_c / d(texel x), d(texel y): a tap outside counts as a 0 texel, as in grid_sample's backward
                dax = fmaf(ga, fmaf(c.ay, t[3] - t[2], (1.f - c.ay) * (t[1] - t[0])), dax);
                day = fmaf(ga, fmaf(c.ax, t[3] - t[1], (1.f - c.ax) * (t[2] - t[0])), day);
                if (a.g_albedo) {
                    float* gp = a.g_albedo + abase + (size_t)ch * plane;
                    if (c.t00) atomicAdd(gp + c.i00, c.w00 * ga);
                    if (c.t01) atomicAdd(gp + c.i00 + 1, c.w01 * ga);
                    if (c.t10) atomicAdd(gp + c.i00 + T, c.w10 * ga);
                    if (c.t11) atomicAdd(gp + c.i00 + T + 1, c.w11 * ga);
                }
            }
            gu = 0.5f * (float)T * dax;  // d(texel) / d(grid) = T / 2
            gv = 0.5f * (float)T * day;
            if (want_sh) {
#pragma unroll
                for (int i = 0; i < 9; ++i) {
#pragma unroll
                    for (int ch = 0; ch < 3; ++ch) acc[3 * i + ch] = fmaf(kb[i], gs[ch], acc[3 * i + ch]);
                }
            }
            if (want_n) {
                float G[9];  // dL / d basis_i = k_i sum_c sh[i][c] gs_c   (G[0] unused: the constant term)
                const float k[9] = {kK0, kK1, kK1, kK1, kK2, kK2, kK2, kK7, kK8};
#pragma unroll
                for (int i = 1; i < 9; ++i)
                    G[i] = k[i] * fmaf(shb[3 * i + 2], gs[2], fmaf(shb[3 * i + 1], gs[1], shb[3 * i] * gs[0]));
                gn[0] = a.nrm_mul * fmaf(2.f * G[7], x, fmaf(G[5], z, fmaf(G[4], y, G[1])));
                gn[1] = a.nrm_mul * fmaf(-2.f * G[7], y, fmaf(G[6], z, fmaf(G[4], x, G[2])));
                gn[2] = a.nrm_mul * fmaf(6.f * G[8], z, fmaf(G[6], y, fmaf(G[5], x, G[3])));
            }
        }
        if (a.g_uv) {
            a.g_uv[base] = gu;
            a.g_uv[base + HW] = gv;
            a.g_uv[base + 2 * HW] = 0.f;
        }
        if (want_n) {
            a.g_nrm[base] = gn[0];
            a.g_nrm[base + HW] = gn[1];
            a.g_nrm[base + 2 * HW] = gn[2];
        }
    }
    if (!want_sh) return;  // (uniform over the grid)
#pragma unroll
    for (int k = 0; k < 27; ++k) {
        float v = acc[k];
#pragma unroll
        for (int off = 32; off > 0; off >>= 1) v += __shfl_xor(v, off, 64);
        acc[k] = v;
    }
    if ((threadIdx.x & 63) == 0) {
#pragma unroll
        for (int k = 0; k < 27; ++k) red[threadIdx.x >> 6][k] = acc[k];
    }
    __syncthreads();
    if (threadIdx.x < 27)
        a.part[((size_t)b * a.nblk + blk) * 27 + threadIdx.x] =
            (red[0][threadIdx.x] + red[1][threadIdx.x]) + (red[2][threadIdx.x] + red[3][threadIdx.x]);
}

inline int bwd_blocks(int H, int W) { return gif::cdiv((long)H * W, 256 * kBwdRounds); }

// the checks both entry points share; 1: nothing to do, 0: go on
int shade_dims(const char* what, int B, int Ba, int H, int W, int T) {
    GIF_REQUIRE(B >= 0 && H >= 0 && W >= 0 && T >= 0, "%s: bad dims (B=%d H=%d W=%d T=%d)", what, B, H, W, T);
    GIF_REQUIRE(Ba == 1 || Ba == B, "%s: Ba = %d must be 1 or B = %d", what, Ba, B);
    GIF_REQUIRE((int64_t)B * 3 * H * W < ((int64_t)1 << 31), "%s: B * 3 * H * W must stay below 2^31", what);
    return ((int64_t)B * H * W == 0) ? 1 : 0;
}

}  // namespace

extern "C" int gif_shade_sh_f32(const float* uv, const float* nrm, const uint8_t* mask, const float* albedo, const float* sh,
                                float* out, int B, int Ba, int H, int W, int T, float nrm_mul, float nrm_add,
                                gif_stream_t stream) {
    const int rc = shade_dims("shade_sh", B, Ba, H, W, T);
    if (rc) return rc < 0 ? rc : 0;
    GIF_REQUIRE(uv && nrm && mask && sh && out && (albedo || T == 0), "shade_sh: null pointer");
    const int HW = H * W, nblk = gif::cdiv(HW, 256);
    shade_sh_kernel<<<(unsigned)((int64_t)nblk * B), 256, 0, gif::as_stream(stream)>>>(uv, nrm, mask, albedo, sh, out, HW, nblk,
                                                                                      Ba == B, T, nrm_mul, nrm_add);
    return gif::check_launch("shade_sh");
}

extern "C" int64_t gif_shade_sh_bwd_workspace_bytes(int B, int H, int W) {
    if (B <= 0 || H <= 0 || W <= 0) return 0;
    return ((int64_t)B * bwd_blocks(H, W) + gif_ew::reduce_tmp_rows(B)) * 27 * (int64_t)sizeof(float);
}

extern "C" int gif_shade_sh_bwd_f32(const float* uv, const float* nrm, const uint8_t* mask, const float* albedo,
                                    const float* sh, const float* g_out, float* g_uv, float* g_nrm, float* g_albedo,
                                    float* g_sh, int B, int Ba, int H, int W, int T, float nrm_mul, float nrm_add,
                                    void* workspace, gif_stream_t stream) {
    const int rc = shade_dims("shade_sh_bwd", B, Ba, H, W, T);
    if (rc < 0) return rc;
    GIF_REQUIRE(!(g_albedo && T == 0), "shade_sh_bwd: g_albedo of an empty texture (T = 0)");
    const bool work = rc == 0 && (g_uv || g_nrm || g_albedo || g_sh);
    if (work) {
        GIF_REQUIRE(uv && nrm && mask && sh && g_out && (albedo || T == 0), "shade_sh_bwd: null pointer");
        GIF_REQUIRE(!g_sh || workspace, "shade_sh_bwd: g_sh needs the workspace");
    }
    hipStream_t s = gif::as_stream(stream);
    if (g_albedo) {  // zeroed inside, also when no pixel adds to it
        hipError_t me = hipMemsetAsync(g_albedo, 0, (size_t)Ba * 3 * T * T * sizeof(float), s);
        if (me != hipSuccess) { gif::set_error("shade_sh_bwd memset: %s", hipGetErrorString(me)); return (int)me; }
    }
    if (rc == 1 && g_sh && B > 0) {  // no pixel: 27 empty sums per sample (no kernel runs that would write them)
        hipError_t me = hipMemsetAsync(g_sh, 0, (size_t)B * 27 * sizeof(float), s);
        if (me != hipSuccess) { gif::set_error("shade_sh_bwd memset: %s", hipGetErrorString(me)); return (int)me; }
    }
    if (!work) return 0;
    ShadeBwd a{};
    a.uv = uv; a.nrm = nrm; a.albedo = albedo; a.sh = sh; a.g_out = g_out; a.mask = mask;
    a.g_uv = g_uv; a.g_nrm = g_nrm; a.g_albedo = g_albedo; a.part = g_sh ? (float*)workspace : nullptr;
    a.HW = H * W; a.nblk = bwd_blocks(H, W); a.per_sample_albedo = Ba == B; a.T = T; a.nrm_mul = nrm_mul; a.nrm_add = nrm_add;
    shade_sh_bwd_kernel<<<(unsigned)((int64_t)a.nblk * B), 256, 0, s>>>(a);
    if (int e = gif::check_launch("shade_sh_bwd")) return e;
    if (g_sh) return gif::reduce_partials(a.part, g_sh, B, a.nblk, 27, a.part + (size_t)B * a.nblk * 27, gif_ew::reduce_tmp_rows(B), s);
    return 0;
}
