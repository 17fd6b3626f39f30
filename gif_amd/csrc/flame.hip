// The FLAME layer for gfx950: blend shapes, pose correctives and linear blend skinning, forward and backward.
// The published algorithm (FLAME, Li et al. 2017, in the smplx formulation), not a port: the reference keeps its layer in an absent
// submodule.  Per sample, with betas = cat(shape, expression) and pose_feature = (R_1..R_{J-1} - I):
//   v_posed = v_template + dirs^T . coef           coef = cat(betas, pose_feature), dirs = [K blend-shape rows ; P corrective rows]
//   vertex  = (sum_j lbs_w[v,j] A_j) . [v_posed, 1]  A_j = the chain's relative transforms, 3x4 row-major
// Three entry points: gif_flame_joints_f32 (betas, rotations, pose feature and the kinematic chain, one small workgroup per sample),
// gif_flame_skin_f32 (the two lines above in one launch) and gif_flame_skin_bwd_f32 (their transposes: reductions over V by
// per-workgroup partial sums and a fixed-order second pass, no float atomics); a fourth, gif_pose_chain_bwd_f32, is the backward of the
// first (its per-sample arithmetic is in flame_chain.h, shared with a host check).  All fp32 VALU: 0.18 GFLOP over 11 MB of constants
// at B = 32, V = 5023, K = 150 — latency- and bytes-bound, nothing for the matrix cores.
#include "common.h"

#define GIF_CHAIN_FN __host__ __device__ __forceinline__
#include "flame_chain.h"

namespace {

constexpr int kMaxJ = 8;
constexpr int kBC = 32;  // samples in flight per workgroup: 8 per wave

// ---------------------------------------------------------------------------------------------------------------- forward
// A workgroup owns kTV vertices = kTC components, one component per lane (48 of a wave's 64 lanes: a tile of 16 vertices is what
// gives V = 5023 its 314 workgroups on 256 CUs), and walks the batch in chunks of kBC samples, 8 per wave.  coef is staged in LDS
// kKC columns at a time (any KP fits; each pass is summed on its own and then added: blocked sums, a shorter rounding walk than
// KP terms in a row), A once per chunk; a wave's reads of them are one address for all lanes (coef) or one of
// three consecutive 16-byte rows (A): broadcasts, no bank conflict.  Every wave reads the same dirs rows (coalesced, 192 bytes per
// row): HBM sees the tile once per sample chunk, the other three reads hit the L1.
constexpr int kTV = 16, kTC = 3 * kTV, kKC = 64;

__global__ void __launch_bounds__(256) flame_skin_kernel(const float* __restrict__ tmpl, const float* __restrict__ dirs,
                                                         const float* __restrict__ lbs_w, const float* __restrict__ coef,
                                                         const float* __restrict__ A, float* __restrict__ verts,
                                                         float* __restrict__ v_posed, int B, int V, int KP, int J) {
    __shared__ __attribute__((aligned(16))) float cf[kBC][kKC];
    __shared__ __attribute__((aligned(16))) float As[kBC][kMaxJ * 12];
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const long C3 = 3L * V;
    const long c = (long)blockIdx.x * kTC + lane;
    const bool live = lane < kTC && c < C3;
    const int vl = (lane < kTC ? lane : kTC - 1) / 3, r = (lane < kTC ? lane : kTC - 1) - 3 * vl;
    float w[kMaxJ];
#pragma unroll
    for (int j = 0; j < kMaxJ; ++j) w[j] = (live && j < J) ? lbs_w[((long)blockIdx.x * kTV + vl) * J + j] : 0.f;
    const float t0 = live ? tmpl[c] : 0.f;
    const int J12 = J * 12;

    for (int b0 = 0; b0 < B; b0 += kBC) {
        const int nb = min(kBC, B - b0);
        const bool busy = wave * 8 < nb;  // wave-uniform
        __syncthreads();                  // the previous chunk's readers of As are done
        for (int i = tid; i < kBC * J12; i += 256) {
            const int bl = i / J12, e = i - bl * J12;
            As[bl][e] = bl < nb ? A[(long)(b0 + bl) * J12 + e] : 0.f;
        }
        __syncthreads();
        float acc[8];
#pragma unroll
        for (int s = 0; s < 8; ++s) acc[s] = t0;
        for (int k0 = 0; k0 < KP; k0 += kKC) {
            const int kn = min(kKC, KP - k0);
            if (k0) __syncthreads();  // the previous pass's readers of cf are done
            for (int i = tid; i < kBC * kKC; i += 256) {
                const int bl = i / kKC, kk = i - bl * kKC;
                cf[bl][kk] = (bl < nb && kk < kn) ? coef[(long)(b0 + bl) * KP + k0 + kk] : 0.f;
            }
            __syncthreads();
            if (busy) {
                const float* dp = dirs + (long)k0 * C3 + c;
                float part[8] = {0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f};
#pragma unroll 2
                for (int kk = 0; kk < kn; kk += 4) {
                    float d[4];
#pragma unroll
                    for (int i = 0; i < 4; ++i) d[i] = (live && kk + i < kn) ? dp[(long)(kk + i) * C3] : 0.f;
#pragma unroll
                    for (int s = 0; s < 8; ++s) {
                        const float4 q = *reinterpret_cast<const float4*>(&cf[wave * 8 + s][kk]);
                        part[s] += d[0] * q.x;
                        part[s] += d[1] * q.y;
                        part[s] += d[2] * q.z;
                        part[s] += d[3] * q.w;
                    }
                }
#pragma unroll
                for (int s = 0; s < 8; ++s) acc[s] += part[s];
            }
        }
        if (busy) {
#pragma unroll
            for (int s = 0; s < 8; ++s) {
                const int bl = wave * 8 + s;
                if (bl < nb) {  // wave-uniform
                    const float x = __shfl(acc[s], 3 * vl, 64), y = __shfl(acc[s], 3 * vl + 1, 64), z = __shfl(acc[s], 3 * vl + 2, 64);
                    float4 T = make_float4(0.f, 0.f, 0.f, 0.f);
#pragma unroll
                    for (int j = 0; j < kMaxJ; ++j) {
                        if (j < J) {
                            const float4 a = *reinterpret_cast<const float4*>(&As[bl][j * 12 + 4 * r]);
                            T.x += w[j] * a.x; T.y += w[j] * a.y; T.z += w[j] * a.z; T.w += w[j] * a.w;
                        }
                    }
                    if (live) {
                        const long o = (long)(b0 + bl) * C3 + c;
                        verts[o] = T.x * x + T.y * y + T.z * z + T.w;
                        if (v_posed) v_posed[o] = acc[s];
                    }
                }
            }
        }
    }
}

// --------------------------------------------------------------------------------------------------------------- backward
// g_coef[b,k] = sum_c dirs[k,c] g_v_posed[b,c], g_v_posed[b,v] = (sum_j lbs_w[v,j] A[b,j].R)^T g_verts[b,v].
// Workgroup (x, y): kBV vertices (96 components) x kBK rows of dirs, staged in LDS once (odd row stride: lane = row reads are
// conflict-free) and used for every sample chunk.  Per chunk: g_v_posed of the tile into LDS, then lane = row k, wave = 8 samples.
// Partial sums part[x][b][k]; gif::reduce_partials adds them over x in a fixed order.
constexpr int kBV = 32, kBVC = 3 * kBV, kBK = 64;
constexpr long kRedTmp = gif_ew::reduce_tmp_rows_single();  // scratch rows behind each region's partial rows (Y = 1 reductions)

__global__ void __launch_bounds__(256) flame_skin_bwd_coef_kernel(const float* __restrict__ dirs, const float* __restrict__ lbs_w,
                                                                  const float* __restrict__ A, const float* __restrict__ g_verts,
                                                                  float* __restrict__ part, int B, int V, int KP, int J) {
    __shared__ float D[kBK][kBVC + 1];
    __shared__ __attribute__((aligned(16))) float gv[kBC][kBVC];
    __shared__ float As[kBC][kMaxJ * 12];
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const long C3 = 3L * V;
    const long v0 = (long)blockIdx.x * kBV, c0 = 3 * v0;
    const int k0 = blockIdx.y * kBK;
    const int J12 = J * 12;
    for (int i = tid; i < kBK * kBVC; i += 256) {
        const int kk = i / kBVC, cc = i - kk * kBVC;
        D[kk][cc] = (k0 + kk < KP && c0 + cc < C3) ? dirs[(long)(k0 + kk) * C3 + c0 + cc] : 0.f;
    }
    for (int b0 = 0; b0 < B; b0 += kBC) {
        const int nb = min(kBC, B - b0);
        __syncthreads();  // the previous chunk's readers of gv / As are done (first chunk: D is staged)
        for (int i = tid; i < kBC * J12; i += 256) {
            const int bl = i / J12, e = i - bl * J12;
            As[bl][e] = bl < nb ? A[(long)(b0 + bl) * J12 + e] : 0.f;
        }
        __syncthreads();
        for (int i = tid; i < kBC * kBV; i += 256) {
            const int vl = i & (kBV - 1), bl = i / kBV;
            const long v = v0 + vl;
            float o0 = 0.f, o1 = 0.f, o2 = 0.f;
            if (v < V && bl < nb) {
                const float* g = g_verts + (long)(b0 + bl) * C3 + 3 * v;
                const float g0 = g[0], g1 = g[1], g2 = g[2];
                for (int j = 0; j < J; ++j) {
                    const float wj = lbs_w[v * J + j];
                    const float* a = &As[bl][j * 12];
                    o0 += wj * (a[0] * g0 + a[4] * g1 + a[8] * g2);
                    o1 += wj * (a[1] * g0 + a[5] * g1 + a[9] * g2);
                    o2 += wj * (a[2] * g0 + a[6] * g1 + a[10] * g2);
                }
            }
            gv[bl][3 * vl] = o0;
            gv[bl][3 * vl + 1] = o1;
            gv[bl][3 * vl + 2] = o2;
        }
        __syncthreads();
        if (wave * 8 < nb) {  // wave-uniform
            float acc[8] = {0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f};
#pragma unroll 2
            for (int cc = 0; cc < kBVC; cc += 4) {
                const float d0 = D[lane][cc], d1 = D[lane][cc + 1], d2 = D[lane][cc + 2], d3 = D[lane][cc + 3];
#pragma unroll
                for (int s = 0; s < 8; ++s) {
                    const float4 q = *reinterpret_cast<const float4*>(&gv[wave * 8 + s][cc]);
                    acc[s] += d0 * q.x;
                    acc[s] += d1 * q.y;
                    acc[s] += d2 * q.z;
                    acc[s] += d3 * q.w;
                }
            }
            if (k0 + lane < KP) {
#pragma unroll
                for (int s = 0; s < 8; ++s) {
                    const int bl = wave * 8 + s;
                    if (bl < nb) part[((long)blockIdx.x * B + b0 + bl) * KP + k0 + lane] = acc[s];
                }
            }
        }
    }
}

// g_A[b,j] = sum_v lbs_w[v,j] g_verts[b,v] (x) [v_posed[b,v], 1].  Workgroup (x, y): 64 vertices (one per lane) x 4 samples (one per
// wave); the 12 J products are summed over the wave by a fixed xor tree.  Partial sums part[x][b][j][12], added over x afterwards.
__global__ void __launch_bounds__(256) flame_skin_bwd_A_kernel(const float* __restrict__ lbs_w, const float* __restrict__ g_verts,
                                                               const float* __restrict__ v_posed, float* __restrict__ part, int B,
                                                               int V, int J) {
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const int b = blockIdx.y * 4 + wave;
    if (b >= B) return;  // wave-uniform; the kernel has no barrier
    const long v = (long)blockIdx.x * 64 + lane;
    float g[3] = {0.f, 0.f, 0.f}, p[4] = {0.f, 0.f, 0.f, 1.f};
    if (v < V) {
        const long o = (long)b * 3 * V + 3 * v;
#pragma unroll
        for (int i = 0; i < 3; ++i) { g[i] = g_verts[o + i]; p[i] = v_posed[o + i]; }
    }
    for (int j = 0; j < J; ++j) {
        const float wj = v < V ? lbs_w[v * J + j] : 0.f;
        float keep = 0.f;
#pragma unroll
        for (int e = 0; e < 12; ++e) {
            float x = wj * g[e >> 2] * p[e & 3];
#pragma unroll
            for (int off = 32; off > 0; off >>= 1) x += __shfl_xor(x, off, 64);
            if (lane == e) keep = x;
        }
        if (lane < 12) part[(((long)blockIdx.x * B + b) * J + j) * 12 + lane] = keep;
    }
}

// ----------------------------------------------------------------------------------------------------------------- joints
struct JointsParams {
    const float *J0, *Jdirs;       // [J][3], [K][3J]
    const float* src[5];           // shape, expression, pose, neck, eye: [B][.] with a row stride; null = zeros
    long ld[5];
    float *A, *coef;               // [B][J][12], [B][KP]
    int parents[kMaxJ];
    int n_shape, K, KP, J;
};

// axis-angle of joint j in FLAME's order: global and jaw from pose_params, neck, the two eyes; joints past the fifth do not rotate
__device__ __forceinline__ float pose_elem(const JointsParams& p, int b, int j, int i) {
    int s, o;
    if (j == 0) { s = 2; o = i; }
    else if (j == 1) { s = 3; o = i; }
    else if (j == 2) { s = 2; o = 3 + i; }
    else if (j < 5) { s = 4; o = 3 * (j - 3) + i; }
    else return 0.f;
    return p.src[s] ? p.src[s][b * p.ld[s] + o] : 0.f;
}

// One workgroup per sample.  joints = J0 + Jdirs . betas in 8 interleaved partial sums of K / 8 terms (fixed order), Rodrigues in
// the smplx form (angle = |r + 1e-8|), then the chain on one lane: J <= 8 dependent 3x4 products.
__global__ void __launch_bounds__(256) flame_joints_kernel(const JointsParams p) {
    __shared__ float red[8][32];
    __shared__ float jt[kMaxJ * 3], R[kMaxJ][9], G[kMaxJ][12], Ao[kMaxJ * 12];
    const int b = blockIdx.x, tid = threadIdx.x, o = tid & 31, grp = tid >> 5;
    const int J3 = 3 * p.J;
    float sum = 0.f;
    for (int k = grp; k < p.K; k += 8) {
        float beta;
        if (k < p.n_shape) beta = p.src[0] ? p.src[0][b * p.ld[0] + k] : 0.f;
        else beta = p.src[1] ? p.src[1][b * p.ld[1] + k - p.n_shape] : 0.f;
        if (o < J3) sum += p.Jdirs[(long)k * J3 + o] * beta;
        if (o == 0) p.coef[(long)b * p.KP + k] = beta;
    }
    red[grp][o] = sum;
    if (tid < p.J) {
        const float r0 = pose_elem(p, b, tid, 0), r1 = pose_elem(p, b, tid, 1), r2 = pose_elem(p, b, tid, 2);
        const float e0 = r0 + 1e-8f, e1 = r1 + 1e-8f, e2 = r2 + 1e-8f;
        const float angle = sqrtf(e0 * e0 + e1 * e1 + e2 * e2);
        const float x = r0 / angle, y = r1 / angle, z = r2 / angle;
        const float s = sinf(angle), c1 = 1.f - cosf(angle);
        // K = [[0,-z,y],[z,0,-x],[-y,x,0]], R = I + s K + (1 - c) K^2
        float* Rj = R[tid];
        Rj[0] = 1.f + c1 * (-(y * y) - z * z); Rj[1] = -s * z + c1 * (x * y);        Rj[2] = s * y + c1 * (x * z);
        Rj[3] = s * z + c1 * (x * y);          Rj[4] = 1.f + c1 * (-(x * x) - z * z); Rj[5] = -s * x + c1 * (y * z);
        Rj[6] = -s * y + c1 * (x * z);         Rj[7] = s * x + c1 * (y * z);          Rj[8] = 1.f + c1 * (-(x * x) - y * y);
        if (tid >= 1) {
            float* pf = p.coef + (long)b * p.KP + p.K + 9 * (tid - 1);
#pragma unroll
            for (int e = 0; e < 9; ++e) pf[e] = Rj[e] - ((e & 3) == 0 ? 1.f : 0.f);
        }
    }
    __syncthreads();
    if (tid < J3) {
        jt[tid] = p.J0[tid] + (((red[0][tid] + red[1][tid]) + (red[2][tid] + red[3][tid])) +
                               ((red[4][tid] + red[5][tid]) + (red[6][tid] + red[7][tid])));
    }
    __syncthreads();
    if (tid == 0) {
        for (int j = 0; j < p.J; ++j) {
            const int pa = p.parents[j];
            float rel[3];
            for (int i = 0; i < 3; ++i) rel[i] = jt[3 * j + i] - (pa >= 0 ? jt[3 * pa + i] : 0.f);
            for (int i = 0; i < 3; ++i) {
                if (pa < 0) {
                    for (int q = 0; q < 3; ++q) G[j][4 * i + q] = R[j][3 * i + q];
                    G[j][4 * i + 3] = rel[i];
                } else {
                    const float* gp = &G[pa][4 * i];
                    for (int q = 0; q < 3; ++q) G[j][4 * i + q] = gp[0] * R[j][q] + gp[1] * R[j][3 + q] + gp[2] * R[j][6 + q];
                    G[j][4 * i + 3] = gp[0] * rel[0] + gp[1] * rel[1] + gp[2] * rel[2] + gp[3];
                }
            }
            for (int i = 0; i < 3; ++i) {
                const float* gj = &G[j][4 * i];
                for (int q = 0; q < 3; ++q) Ao[12 * j + 4 * i + q] = gj[q];
                Ao[12 * j + 4 * i + 3] = gj[3] - (gj[0] * jt[3 * j] + gj[1] * jt[3 * j + 1] + gj[2] * jt[3 * j + 2]);
            }
        }
    }
    __syncthreads();
    if (tid < 12 * p.J) p.A[(long)b * 12 * p.J + tid] = Ao[tid];
}

// ------------------------------------------------------------------------------------------------------- joints, backward
struct JointsBwdParams {
    const float *J0, *Jdirs;       // as the forward
    const float* src[5];
    long ld[5];
    const float *g_A, *g_coef;     // [B][J][12], [B][KP]
    float* out[5];                 // g_shape, g_expr, g_pose [B][6], g_neck [B][3], g_eye [B][6]: contiguous, null = not computed
    int parents[kMaxJ];
    int n_shape, K, KP, J;
};

// (group, offset) of the axis-angle of joint j, pose_elem's table; joints past the fifth have none
__device__ __forceinline__ bool pose_slot(int j, int* s, int* o) {
    if (j == 0) { *s = 2; *o = 0; }
    else if (j == 1) { *s = 3; *o = 0; }
    else if (j == 2) { *s = 2; *o = 3; }
    else if (j < 5) { *s = 4; *o = 3 * (j - 3); }
    else return false;
    return true;
}

// One workgroup per sample, nothing saved by the forward: joints (the forward's 8 interleaved partial sums) and rotations are
// recomputed, lane 0 walks the chain back (flame_chain.h: J <= 8 dependent 3x3 products), one lane per joint takes Rodrigues'
// derivative, then lanes over k contract g_jt with Jdirs.  Every sum has one owner and a fixed order: no atomics.
__global__ void __launch_bounds__(256) flame_joints_bwd_kernel(const JointsBwdParams p) {
    __shared__ float red[8][32];
    __shared__ float jt[kMaxJ * 3], r[kMaxJ * 3], R[kMaxJ * 9], GR[kMaxJ * 9], gA[kMaxJ * 12], gF[kMaxJ * 9];
    __shared__ float gR[kMaxJ * 9], gGt[kMaxJ * 3], gjt[kMaxJ * 3], gr[kMaxJ * 3];
    __shared__ int par[kMaxJ];
    const int b = blockIdx.x, tid = threadIdx.x, o = tid & 31, grp = tid >> 5;
    const int J = p.J, J3 = 3 * J, P = 9 * (J - 1);
    float sum = 0.f;
    for (int k = grp; k < p.K; k += 8) {
        float beta;
        if (k < p.n_shape) beta = p.src[0] ? p.src[0][b * p.ld[0] + k] : 0.f;
        else beta = p.src[1] ? p.src[1][b * p.ld[1] + k - p.n_shape] : 0.f;
        if (o < J3) sum += p.Jdirs[(long)k * J3 + o] * beta;
    }
    red[grp][o] = sum;
    if (tid < J) {
        int s, off;
        const bool has = pose_slot(tid, &s, &off);
        for (int i = 0; i < 3; ++i) r[3 * tid + i] = (has && p.src[s]) ? p.src[s][b * p.ld[s] + off + i] : 0.f;
        gif::chain_rodrigues(&r[3 * tid], &R[9 * tid]);
        par[tid] = p.parents[tid];
    }
    if (tid < 12 * J) gA[tid] = p.g_A[(long)b * 12 * J + tid];
    if (tid < P) gF[tid] = p.g_coef[(long)b * p.KP + p.K + tid];
    __syncthreads();
    if (tid < J3) {
        jt[tid] = p.J0[tid] + (((red[0][tid] + red[1][tid]) + (red[2][tid] + red[3][tid])) +
                               ((red[4][tid] + red[5][tid]) + (red[6][tid] + red[7][tid])));
    }
    __syncthreads();
    if (tid == 0) {
        gif::chain_world_rotations(J, par, R, GR);
        gif::chain_reverse(J, par, jt, R, GR, gA, P ? gF : nullptr, gR, gGt, gjt);
    }
    __syncthreads();
    if (tid < J) gif::chain_rodrigues_bwd(&r[3 * tid], &gR[9 * tid], &gr[3 * tid]);
    for (int k = tid; k < p.K; k += 256) {  // g_betas[k] = g_coef[k] + Jdirs[k] . g_jt, o = 0 .. 3J-1 in order
        float* dst = k < p.n_shape ? p.out[0] : p.out[1];
        if (!dst) continue;
        float acc = p.g_coef[(long)b * p.KP + k];
        const float* d = p.Jdirs + (long)k * J3;
        for (int q = 0; q < J3; ++q) acc += d[q] * gjt[q];
        if (k < p.n_shape) dst[(long)b * p.n_shape + k] = acc;
        else dst[(long)b * (p.K - p.n_shape) + k - p.n_shape] = acc;
    }
    __syncthreads();
    if (tid < 15) {  // the 15 pose entries, every one written: a joint the model does not have, or has past the fifth, leaves zeros
        const int j = tid / 3, i = tid - 3 * j;
        int s, off;
        pose_slot(j, &s, &off);
        const int width = s == 3 ? 3 : 6;
        if (p.out[s]) p.out[s][(long)b * width + off + i] = j < J ? gr[3 * j + i] : 0.f;
    }
}

inline bool flame_dims_ok(int B, int V, int KP, int J) {
    return B >= 0 && V >= 0 && KP >= 0 && J >= 1 && J <= kMaxJ && KP >= 9 * (J - 1);
}

}  // namespace

extern "C" int gif_flame_skin_f32(const float* tmpl, const float* dirs, const float* lbs_w, const float* coef, const float* A,
                                  float* verts, float* v_posed, int B, int V, int KP, int J, gif_stream_t stream) {
    GIF_REQUIRE(flame_dims_ok(B, V, KP, J), "flame_skin: bad dims (B=%d V=%d KP=%d J=%d; J in 1..8, KP >= 9 (J - 1))", B, V, KP, J);
    if (B == 0 || V == 0) return 0;
    GIF_REQUIRE(tmpl && lbs_w && A && verts && (dirs || KP == 0) && (coef || KP == 0), "flame_skin: null pointer");
    GIF_REQUIRE((long)B * KP < (1L << 31) && (long)V * 3 < (1L << 31), "flame_skin: B * KP and 3 V must fit 31 bits");
    flame_skin_kernel<<<gif::cdiv(V, kTV), 256, 0, gif::as_stream(stream)>>>(tmpl, dirs, lbs_w, coef, A, verts, v_posed, B, V, KP, J);
    return gif::check_launch("flame_skin");
}

extern "C" int64_t gif_flame_skin_bwd_workspace_bytes(int B, int V, int KP, int J) {
    if (!flame_dims_ok(B, V, KP, J) || B == 0 || V == 0) return 0;
    // per region: the partial rows of its first pass + the rows gif::reduce_partials may need for a long reduction
    const int64_t coef_rows = gif::cdiv(V, kBV) + kRedTmp, a_rows = gif::cdiv(V, 64) + kRedTmp;
    return (coef_rows * B * KP + a_rows * B * J * 12) * (int64_t)sizeof(float);
}

extern "C" int gif_flame_skin_bwd_f32(const float* dirs, const float* lbs_w, const float* A, const float* g_verts,
                                      const float* v_posed, float* g_coef, float* g_A, int B, int V, int KP, int J,
                                      void* workspace, gif_stream_t stream) {
    GIF_REQUIRE(flame_dims_ok(B, V, KP, J), "flame_skin_bwd: bad dims (B=%d V=%d KP=%d J=%d; J in 1..8, KP >= 9 (J - 1))", B, V, KP, J);
    if (B == 0) return 0;
    GIF_REQUIRE((long)B * KP < (1L << 31) && (long)V * 3 < (1L << 31) && B <= 4 * 65535,
                "flame_skin_bwd: B * KP and 3 V must fit 31 bits, B <= 262140");
    hipStream_t s = gif::as_stream(stream);
    if (V == 0) {  // empty sums
        hipError_t e = hipSuccess;
        if (g_coef && KP) e = hipMemsetAsync(g_coef, 0, (size_t)B * KP * sizeof(float), s);
        if (e == hipSuccess && g_A) e = hipMemsetAsync(g_A, 0, (size_t)B * J * 12 * sizeof(float), s);
        if (e != hipSuccess) { gif::set_error("flame_skin_bwd memset: %s", hipGetErrorString(e)); return (int)e; }
        return 0;
    }
    GIF_REQUIRE(lbs_w && g_verts && workspace, "flame_skin_bwd: null pointer");
    GIF_REQUIRE(!g_coef || KP == 0 || (dirs && A), "flame_skin_bwd: g_coef needs dirs and A");
    GIF_REQUIRE(!g_A || v_posed, "flame_skin_bwd: g_A needs v_posed");
    float* ws = static_cast<float*>(workspace);
    const int nc = gif::cdiv(V, kBV), na = gif::cdiv(V, 64);
    float* part_a = ws + (size_t)(nc + kRedTmp) * B * KP;
    if (g_coef && KP) {
        flame_skin_bwd_coef_kernel<<<dim3(nc, gif::cdiv(KP, kBK)), 256, 0, s>>>(dirs, lbs_w, A, g_verts, ws, B, V, KP, J);
        int rc = gif::reduce_partials(ws, g_coef, 1, nc, B * KP, ws + (size_t)nc * B * KP, kRedTmp, s);
        if (rc) return rc;
    }
    if (g_A) {
        flame_skin_bwd_A_kernel<<<dim3(na, gif::cdiv(B, 4)), 256, 0, s>>>(lbs_w, g_verts, v_posed, part_a, B, V, J);
        int rc = gif::reduce_partials(part_a, g_A, 1, na, B * J * 12, part_a + (size_t)na * B * J * 12, kRedTmp, s);
        if (rc) return rc;
    }
    return gif::check_launch("flame_skin_bwd");
}

extern "C" int gif_flame_joints_f32(const float* J0, const float* Jdirs, const int32_t* parents, const float* shape,
                                    int64_t ld_shape, int n_shape, const float* expr, int64_t ld_expr, int n_exp,
                                    const float* pose, int64_t ld_pose, const float* neck, int64_t ld_neck, const float* eye,
                                    int64_t ld_eye, float* A, float* coef, int B, int KP, int J, gif_stream_t stream) {
    GIF_REQUIRE(B >= 0 && n_shape >= 0 && n_exp >= 0 && J >= 1 && J <= kMaxJ, "flame_joints: bad dims (B=%d J=%d; J in 1..8)", B, J);
    GIF_REQUIRE((long)n_shape + n_exp + 9 * (J - 1) == KP, "flame_joints: KP = %d is not n_shape + n_exp + 9 (J - 1)", KP);
    GIF_REQUIRE(parents, "flame_joints: null parents");
    for (int j = 0; j < J; ++j)
        GIF_REQUIRE(parents[j] < j && parents[j] >= -1, "flame_joints: parents[%d] = %d is not an earlier joint", j, parents[j]);
    if (B == 0) return 0;
    GIF_REQUIRE(J0 && A && (coef || KP == 0) && (Jdirs || n_shape + n_exp == 0), "flame_joints: null pointer");
    JointsParams p{};
    p.J0 = J0; p.Jdirs = Jdirs; p.A = A; p.coef = coef;
    p.src[0] = shape; p.src[1] = expr; p.src[2] = pose; p.src[3] = neck; p.src[4] = eye;
    p.ld[0] = ld_shape; p.ld[1] = ld_expr; p.ld[2] = ld_pose; p.ld[3] = ld_neck; p.ld[4] = ld_eye;
    for (int j = 0; j < J; ++j) p.parents[j] = parents[j];
    p.n_shape = n_shape; p.K = n_shape + n_exp; p.KP = KP; p.J = J;
    flame_joints_kernel<<<B, 256, 0, gif::as_stream(stream)>>>(p);
    return gif::check_launch("flame_joints");
}

extern "C" int gif_pose_chain_bwd_f32(const float* J0, const float* Jdirs, const int32_t* parents, const float* shape,
                                      int64_t ld_shape, int n_shape, const float* expr, int64_t ld_expr, int n_exp,
                                      const float* pose, int64_t ld_pose, const float* neck, int64_t ld_neck, const float* eye,
                                      int64_t ld_eye, const float* g_A, const float* g_coef, float* g_shape, float* g_expr,
                                      float* g_pose, float* g_neck, float* g_eye, int B, int KP, int J, gif_stream_t stream) {
    GIF_REQUIRE(B >= 0 && n_shape >= 0 && n_exp >= 0 && J >= 1 && J <= kMaxJ, "pose_chain_bwd: bad dims (B=%d J=%d; J in 1..8)", B, J);
    GIF_REQUIRE((long)n_shape + n_exp + 9 * (J - 1) == KP, "pose_chain_bwd: bad dims (KP = %d is not n_shape + n_exp + 9 (J - 1))", KP);
    if (B == 0 || !(g_shape || g_expr || g_pose || g_neck || g_eye)) return 0;
    GIF_REQUIRE(parents, "pose_chain_bwd: null pointer (parents)");
    for (int j = 0; j < J; ++j)
        GIF_REQUIRE(parents[j] < j && parents[j] >= -1, "pose_chain_bwd: parents[%d] = %d is not an earlier joint", j, parents[j]);
    GIF_REQUIRE(J0 && g_A && (g_coef || KP == 0) && (Jdirs || n_shape + n_exp == 0), "pose_chain_bwd: null pointer");
    GIF_REQUIRE((long)B * KP < (1L << 31), "pose_chain_bwd: B * KP must fit 31 bits");
    JointsBwdParams p{};
    p.J0 = J0; p.Jdirs = Jdirs; p.g_A = g_A; p.g_coef = g_coef;
    p.src[0] = shape; p.src[1] = expr; p.src[2] = pose; p.src[3] = neck; p.src[4] = eye;
    p.ld[0] = ld_shape; p.ld[1] = ld_expr; p.ld[2] = ld_pose; p.ld[3] = ld_neck; p.ld[4] = ld_eye;
    p.out[0] = n_shape ? g_shape : nullptr; p.out[1] = n_exp ? g_expr : nullptr; p.out[2] = g_pose; p.out[3] = g_neck; p.out[4] = g_eye;
    for (int j = 0; j < J; ++j) p.parents[j] = parents[j];
    p.n_shape = n_shape; p.K = n_shape + n_exp; p.KP = KP; p.J = J;
    flame_joints_bwd_kernel<<<B, 256, 0, gif::as_stream(stream)>>>(p);
    return gif::check_launch("pose_chain_bwd");
}
