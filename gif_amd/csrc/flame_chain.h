// The FLAME pose chain of one sample, backward: the arithmetic gif_pose_chain_bwd_f32 (flame.hip) runs per sample,
// as plain functions for the device and for the host.  Not part of the ABI.  The including file says how the functions are declared
// by defining GIF_CHAIN_FN first (flame.hip: __host__ __device__ __forceinline__; tests/host/flame_chain_check.cpp, which includes
// this file alone: inline).
// Forward, in flame_joints_kernel's names (row-major 3x3 R, joints jt [J][3], parents[j] < j, a root has parent -1):
//   R_j  = I + sin(a) K + (1 - cos(a)) K^2,  a = |r_j + 1e-8|,  K = skew(r_j / a)              (Rodrigues, the smplx form)
//   GR_j = GR_p R_j,  Gt_j = GR_p (jt_j - jt_p) + Gt_p;  a root: GR_j = R_j, Gt_j = jt_j
//   A_j  = [GR_j | Gt_j - GR_j jt_j],  F_j = R_j - I (the pose feature, j >= 1)
// Backward: g_A [J][12] and g_F [J - 1][9] -> g_jt [J][3] and g_r [J][3].  Gt itself is not needed: only GR enters a derivative.
#pragma once
#include <math.h>

namespace gif {

// R [9] = Rodrigues(r [3]), written as flame_joints_kernel writes it
GIF_CHAIN_FN void chain_rodrigues(const float* r, float* R) {
    const float e0 = r[0] + 1e-8f, e1 = r[1] + 1e-8f, e2 = r[2] + 1e-8f;
    const float angle = sqrtf(e0 * e0 + e1 * e1 + e2 * e2);
    const float x = r[0] / angle, y = r[1] / angle, z = r[2] / angle;
    const float s = sinf(angle), c1 = 1.f - cosf(angle);
    R[0] = 1.f + c1 * (-(y * y) - z * z); R[1] = -s * z + c1 * (x * y);        R[2] = s * y + c1 * (x * z);
    R[3] = s * z + c1 * (x * y);          R[4] = 1.f + c1 * (-(x * x) - z * z); R[5] = -s * x + c1 * (y * z);
    R[6] = -s * y + c1 * (x * z);         R[7] = s * x + c1 * (y * z);          R[8] = 1.f + c1 * (-(x * x) - y * y);
}

// g_r [3] = (d R / d r)^T g [9]: the derivative of the lines above as they stand.  The direction d = r / a is NOT a unit vector
// (a is the norm of r + 1e-8), so K^2 = d d^T - |d|^2 I and nothing is simplified with |d| = 1.  r = 0 gives a = 1.7e-8, d = 0 and
// the finite value autograd gives: (sin(a) / a) times the antisymmetric part of g.
GIF_CHAIN_FN void chain_rodrigues_bwd(const float* r, const float* g, float* gr) {
    const float e0 = r[0] + 1e-8f, e1 = r[1] + 1e-8f, e2 = r[2] + 1e-8f;
    const float angle = sqrtf(e0 * e0 + e1 * e1 + e2 * e2);
    const float x = r[0] / angle, y = r[1] / angle, z = r[2] / angle;
    const float s = sinf(angle), c = cosf(angle), c1 = 1.f - c;
    const float ax = g[7] - g[5], ay = g[2] - g[6], az = g[3] - g[1];     // antisymmetric part: what sin(a) K sees
    const float sxy = g[1] + g[3], sxz = g[2] + g[6], syz = g[5] + g[7];  // symmetric off-diagonal sums: what K^2 sees
    const float gs = x * ax + y * ay + z * az;
    const float gc1 = g[0] * (-(y * y) - z * z) + g[4] * (-(x * x) - z * z) + g[8] * (-(x * x) - y * y) +
                      sxy * (x * y) + sxz * (x * z) + syz * (y * z);
    const float gx = s * ax + c1 * (-2.f * x * (g[4] + g[8]) + y * sxy + z * sxz);
    const float gy = s * ay + c1 * (-2.f * y * (g[0] + g[8]) + x * sxy + z * syz);
    const float gz = s * az + c1 * (-2.f * z * (g[0] + g[4]) + x * sxz + y * syz);
    // d = r / a: d d / d a = -d / a;  d a / d r = (r + 1e-8) / a
    const float ga = gs * c + gc1 * s - (gx * x + gy * y + gz * z) / angle;
    gr[0] = gx / angle + ga * (e0 / angle);
    gr[1] = gy / angle + ga * (e1 / angle);
    gr[2] = gz / angle + ga * (e2 / angle);
}

// GR [J][9]: the world rotations, the forward kernel's products
GIF_CHAIN_FN void chain_world_rotations(int J, const int* parents, const float* R, float* GR) {
    for (int j = 0; j < J; ++j) {
        const int pa = parents[j];
        const float* Rj = R + 9 * j;
        for (int i = 0; i < 3; ++i) {
            for (int q = 0; q < 3; ++q) {
                if (pa < 0) {
                    GR[9 * j + 3 * i + q] = Rj[3 * i + q];
                } else {
                    const float* gp = GR + 9 * pa + 3 * i;
                    GR[9 * j + 3 * i + q] = gp[0] * Rj[q] + gp[1] * Rj[3 + q] + gp[2] * Rj[6 + q];
                }
            }
        }
    }
}

// The reverse walk.  In: jt [J][3], R, GR [J][9], g_A [J][12], g_F [J - 1][9] (null = zeros).  Out: g_R [J][9] = dL/d R_j and g_jt
// [J][3]; g_Gt [J][3] is scratch.  g_R doubles as the accumulator of dL/d GR_j: joint j turns its own block into dL/d R_j after its
// parent has taken what it needs from it, and no later joint (all have smaller indices) reads it again.  One thread, fixed order.
GIF_CHAIN_FN void chain_reverse(int J, const int* parents, const float* jt, const float* R, const float* GR, const float* g_A,
                                const float* g_F, float* g_R, float* g_Gt, float* g_jt) {
    for (int j = 0; j < J; ++j) {  // seeds: A_j = [GR_j | Gt_j - GR_j jt_j]
        const float t0 = g_A[12 * j + 3], t1 = g_A[12 * j + 7], t2 = g_A[12 * j + 11];
        const float* G = GR + 9 * j;
        for (int i = 0; i < 3; ++i) {
            const float ti = g_A[12 * j + 4 * i + 3];
            g_Gt[3 * j + i] = ti;
            for (int q = 0; q < 3; ++q) g_R[9 * j + 3 * i + q] = g_A[12 * j + 4 * i + q] - ti * jt[3 * j + q];
        }
        for (int q = 0; q < 3; ++q) g_jt[3 * j + q] = -(G[q] * t0 + G[3 + q] * t1 + G[6 + q] * t2);
    }
    for (int j = J - 1; j >= 0; --j) {
        const int pa = parents[j];
        float* gG = g_R + 9 * j;
        const float* gt = g_Gt + 3 * j;
        if (pa >= 0) {
            const float* Rj = R + 9 * j;
            const float* Gp = GR + 9 * pa;
            float rel[3], out[9];
            for (int q = 0; q < 3; ++q) rel[q] = jt[3 * j + q] - jt[3 * pa + q];
            for (int i = 0; i < 3; ++i) {  // GR_j = GR_p R_j, Gt_j = GR_p rel + Gt_p: the parent's share
                for (int q = 0; q < 3; ++q)
                    g_R[9 * pa + 3 * i + q] += gG[3 * i] * Rj[3 * q] + gG[3 * i + 1] * Rj[3 * q + 1] + gG[3 * i + 2] * Rj[3 * q + 2] +
                                               gt[i] * rel[q];
                g_Gt[3 * pa + i] += gt[i];
            }
            for (int q = 0; q < 3; ++q) {
                const float grel = Gp[q] * gt[0] + Gp[3 + q] * gt[1] + Gp[6 + q] * gt[2];
                g_jt[3 * j + q] += grel;
                g_jt[3 * pa + q] -= grel;
            }
            for (int m = 0; m < 3; ++m)  // g_R_j = GR_p^T g_GR_j
                for (int q = 0; q < 3; ++q) out[3 * m + q] = Gp[m] * gG[q] + Gp[3 + m] * gG[3 + q] + Gp[6 + m] * gG[6 + q];
            for (int e = 0; e < 9; ++e) gG[e] = out[e];
        } else {
            for (int q = 0; q < 3; ++q) g_jt[3 * j + q] += gt[q];
        }
        if (g_F && j >= 1)
            for (int e = 0; e < 9; ++e) gG[e] += g_F[9 * (j - 1) + e];
    }
}

}  // namespace gif
