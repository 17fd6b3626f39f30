// FLAME landmarks for gfx950: static and dynamic-contour landmarks of a skinned mesh, forward and backward.
// The published definition (smplx lbs.vertices2landmarks / find_dynamic_lmk_idx_and_bcoords), not a port:
//   landmark[b,l] = sum_{i<3} bary[l,i] verts[b, vid[l,i]]      vid = the three vertex ids of the landmark's embedding face
// The first Ld landmarks of a sample come from row `row[b]` of a table of R = 2M + 1 rows, chosen from the yaw of the world
// rotation of joint `yaw_joint` (the rotation part of A[b, yaw_joint], elements 0, 4, 8 = its first column); the Ls that follow are
// static.  Two entry points: gif_flame_landmarks_f32 (row choice and gather in one launch, one workgroup per sample) and
// gif_flame_landmarks_bwd_f32 (the scatter to g_verts: duplicates resolved in LDS in a fixed order, no float atomics, every element
// of g_verts written).  A few hundred gathers per sample: latency-bound, plain fp32 VALU.
#include "common.h"

namespace {

constexpr int kMaxJ = 8;

// row of the dynamic table for the world rotation whose row-major 3x4 entry starts at `a`: yaw in degrees, clamped from above at
// M, rounded half-to-even (rintf), negative values folded behind the positive ones.  Always inside 0..R-1.
__device__ __forceinline__ int yaw_row(const float* a, int R) {
    const int M = (R - 1) / 2;
    const float r00 = a[0], r10 = a[4], r20 = a[8];
    const float yaw = -atan2f(-r20, sqrtf(r00 * r00 + r10 * r10)) * 57.29577951308232f;
    if (!(fabsf(yaw) <= 3.0e38f)) return 0;  // NaN (from a non-finite A): fminf would turn it into M
    const float y = rintf(fminf(yaw, (float)M));
    const int row = y >= 0.f ? (int)y : (y < -(float)M ? 2 * M : M - (int)y);  // (-0 >= 0: row 0)
    return min(max(row, 0), R - 1);
}

// (vertex id, weight) of corner k of landmark l in the sample's tables
__device__ __forceinline__ void corner(const int32_t* __restrict__ dyn_vid, const float* __restrict__ dyn_bary,
                                       const int32_t* __restrict__ st_vid, const float* __restrict__ st_bary, int row, int Ld, int l,
                                       int k, int& vid, float& w) {
    if (l < Ld) {
        const long o = ((long)row * Ld + l) * 3 + k;
        vid = dyn_vid[o];
        w = dyn_bary[o];
    } else {
        const long o = (long)(l - Ld) * 3 + k;
        vid = st_vid[o];
        w = st_bary[o];
    }
}

// ---------------------------------------------------------------------------------------------------------------- forward
// One workgroup per sample; lane = one output component (landmark l, axis c), 3 (Ld + Ls) of them in steps of 256.  Lane 0 chooses
// the row and publishes it through LDS.  A vertex id outside 0..V-1 contributes nothing (the Python layer rejects such tables).
__global__ void __launch_bounds__(256) flame_landmarks_kernel(const float* __restrict__ verts, const float* __restrict__ A,
                                                              const int32_t* __restrict__ dyn_vid, const float* __restrict__ dyn_bary,
                                                              const int32_t* __restrict__ st_vid, const float* __restrict__ st_bary,
                                                              float* __restrict__ lmk, int32_t* __restrict__ row_out, int V, int J,
                                                              int yaw_joint, int R, int Ld, int Ls) {
    __shared__ int s_row;
    const int b = blockIdx.x, tid = threadIdx.x;
    if (tid == 0) {
        const int r = Ld > 0 ? yaw_row(A + ((long)b * J + yaw_joint) * 12, R) : 0;
        s_row = r;
        if (row_out) row_out[b] = r;
    }
    __syncthreads();
    const int row = s_row;
    const int n = 3 * (Ld + Ls);
    const float* vb = verts + (long)b * V * 3;
    for (int e = tid; e < n; e += 256) {
        const int l = e / 3, c = e - 3 * l;
        float p[3];
#pragma unroll
        for (int k = 0; k < 3; ++k) {
            int vid;
            float w;
            corner(dyn_vid, dyn_bary, st_vid, st_bary, row, Ld, l, k, vid, w);
            p[k] = (vid >= 0 && vid < V) ? w * vb[(long)vid * 3 + c] : 0.f;
        }
        lmk[(long)b * n + e] = (p[0] + p[1]) + p[2];
    }
}

// --------------------------------------------------------------------------------------------------------------- backward
// g_verts[b,v] = sum over the (landmark, corner) pairs that name v of bary g_lmk[b,l], in the pairs' order.  Workgroup (b, y) owns
// kLV vertices of sample b: their accumulators live in LDS (zeroed, then written out whole, so untouched vertices get exact zeros).
// The sample's n = 3 (Ld + Ls) pairs are staged in LDS as {vertex id, bary g} (kLC at a time; n <= kLC, FLAME's 408 included, is
// staged once).  Lane i takes pair i: if its vertex is in the workgroup's range it walks ALL pairs in order — one broadcast
// 16-byte LDS read each — adds those with its vertex id, and is the vertex's owner iff no earlier pair names it.  Only the owner
// writes: one writer per vertex, one summation order, whatever the duplicates.  O(n^2 / 256) steps per lane: ~650 at n = 408.
constexpr int kLV = 1024, kLC = 1024;

__global__ void __launch_bounds__(256) flame_landmarks_bwd_kernel(const float* __restrict__ g_lmk, const int32_t* __restrict__ row_in,
                                                                  const int32_t* __restrict__ dyn_vid, const float* __restrict__ dyn_bary,
                                                                  const int32_t* __restrict__ st_vid, const float* __restrict__ st_bary,
                                                                  float* __restrict__ g_verts, int V, int R, int Ld, int Ls) {
    __shared__ float acc[3 * kLV];
    __shared__ __attribute__((aligned(16))) float4 con[kLC];
    const int b = blockIdx.x, tid = threadIdx.x;
    const int v0 = blockIdx.y * kLV, nv = min(kLV, V - v0);
    const int L = Ld + Ls, n = 3 * L;
    const int row = Ld > 0 ? min(max(row_in[b], 0), R - 1) : 0;
    for (int i = tid; i < 3 * nv; i += 256) acc[i] = 0.f;
    const bool once = n <= kLC;
    for (int i0 = 0; i0 < n; i0 += 256) {
        const int i = i0 + tid;
        int my = -1;
        if (i < n) {
            int vid;
            float w;
            corner(dyn_vid, dyn_bary, st_vid, st_bary, row, Ld, i / 3, i % 3, vid, w);
            if (vid >= v0 && vid < v0 + nv) my = vid;
        }
        bool owner = my >= 0;
        float s0 = 0.f, s1 = 0.f, s2 = 0.f;
        for (int j0 = 0; j0 < n; j0 += kLC) {
            const int jn = min(kLC, n - j0);
            if (!once || i0 == 0) {  // workgroup-uniform
                __syncthreads();     // the previous tile's readers are done (first pass: acc is zeroed)
                for (int j = tid; j < jn; j += 256) {
                    const int l = (j0 + j) / 3;
                    int vid;
                    float w;
                    corner(dyn_vid, dyn_bary, st_vid, st_bary, row, Ld, l, (j0 + j) - 3 * l, vid, w);
                    const float* g = g_lmk + ((long)b * L + l) * 3;
                    con[j] = make_float4(__int_as_float(vid), w * g[0], w * g[1], w * g[2]);
                }
                __syncthreads();
            }
            if (my >= 0) {
#pragma unroll 4
                for (int j = 0; j < jn; ++j) {
                    const float4 q = con[j];
                    const bool hit = __float_as_int(q.x) == my;
                    if (hit && j0 + j < i) owner = false;
                    s0 += hit ? q.y : 0.f;
                    s1 += hit ? q.z : 0.f;
                    s2 += hit ? q.w : 0.f;
                }
            }
        }
        if (owner) {
            float* a = &acc[3 * (my - v0)];
            a[0] = s0;
            a[1] = s1;
            a[2] = s2;
        }
    }
    __syncthreads();
    float* out = g_verts + ((long)b * V + v0) * 3;
    for (int i = tid; i < 3 * nv; i += 256) out[i] = acc[i];
}

inline bool landmark_dims_ok(int B, int V, int R, int Ld, int Ls) { return B >= 0 && V >= 0 && R >= 0 && Ld >= 0 && Ls >= 0; }

}  // namespace

extern "C" int gif_flame_landmarks_f32(const float* verts, const float* A, const int32_t* dyn_vid, const float* dyn_bary,
                                       const int32_t* st_vid, const float* st_bary, float* lmk, int32_t* row, int B, int V, int J,
                                       int yaw_joint, int R, int Ld, int Ls, gif_stream_t stream) {
    GIF_REQUIRE(landmark_dims_ok(B, V, R, Ld, Ls), "flame_landmarks: bad dims (B=%d V=%d R=%d Ld=%d Ls=%d)", B, V, R, Ld, Ls);
    GIF_REQUIRE(J >= 1 && J <= kMaxJ, "flame_landmarks: J = %d (J in 1..8)", J);
    GIF_REQUIRE(yaw_joint >= 0 && yaw_joint < J, "flame_landmarks: yaw_joint = %d outside 0..J-1 = %d", yaw_joint, J - 1);
    GIF_REQUIRE(Ld == 0 || (R & 1), "flame_landmarks: R = %d rows, the dynamic table needs an odd number (2 M + 1)", R);
    if (B == 0 || Ld + Ls == 0) return 0;
    GIF_REQUIRE((long)R * Ld * 3 < (1L << 31) && ((long)Ld + Ls) * 3 < (1L << 31) && (long)V * 3 < (1L << 31),
                "flame_landmarks: 3 R Ld, 3 (Ld + Ls) and 3 V must fit 31 bits");
    GIF_REQUIRE(lmk && (verts || V == 0) && (Ld == 0 || (A && dyn_vid && dyn_bary)) && (Ls == 0 || (st_vid && st_bary)),
                "flame_landmarks: null pointer");
    flame_landmarks_kernel<<<B, 256, 0, gif::as_stream(stream)>>>(verts, A, dyn_vid, dyn_bary, st_vid, st_bary, lmk, row, V, J,
                                                                  yaw_joint, R, Ld, Ls);
    return gif::check_launch("flame_landmarks");
}

extern "C" int gif_flame_landmarks_bwd_f32(const float* g_lmk, const int32_t* row, const int32_t* dyn_vid, const float* dyn_bary,
                                           const int32_t* st_vid, const float* st_bary, float* g_verts, int B, int V, int R, int Ld,
                                           int Ls, gif_stream_t stream) {
    GIF_REQUIRE(landmark_dims_ok(B, V, R, Ld, Ls), "flame_landmarks_bwd: bad dims (B=%d V=%d R=%d Ld=%d Ls=%d)", B, V, R, Ld, Ls);
    GIF_REQUIRE(Ld == 0 || (R & 1), "flame_landmarks_bwd: R = %d rows, the dynamic table needs an odd number (2 M + 1)", R);
    if (B == 0 || V == 0) return 0;
    GIF_REQUIRE((long)R * Ld * 3 < (1L << 31) && ((long)Ld + Ls) * 3 < (1L << 31) && (long)V * 3 < (1L << 31) &&
                    gif::cdiv(V, kLV) <= 65535,
                "flame_landmarks_bwd: 3 R Ld, 3 (Ld + Ls) and 3 V must fit 31 bits, V <= 67107840");
    GIF_REQUIRE(g_verts, "flame_landmarks_bwd: null pointer");
    hipStream_t s = gif::as_stream(stream);
    if (Ld + Ls == 0) {  // empty sums
        hipError_t e = hipMemsetAsync(g_verts, 0, (size_t)B * V * 3 * sizeof(float), s);
        if (e != hipSuccess) { gif::set_error("flame_landmarks_bwd memset: %s", hipGetErrorString(e)); return (int)e; }
        return 0;
    }
    GIF_REQUIRE(g_lmk && (Ld == 0 || (row && dyn_vid && dyn_bary)) && (Ls == 0 || (st_vid && st_bary)),
                "flame_landmarks_bwd: null pointer");
    flame_landmarks_bwd_kernel<<<dim3(B, gif::cdiv(V, kLV)), 256, 0, s>>>(g_lmk, row, dyn_vid, dyn_bary, st_vid, st_bary, g_verts, V,
                                                                         R, Ld, Ls);
    return gif::check_launch("flame_landmarks_bwd");
}
