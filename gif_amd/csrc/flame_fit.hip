// The landmark term of a FLAME fit for gfx950: projection, weighted squared distance and its gradient in one launch.
//   p[b,l]  = (s (x + tx), -s (y + ty))            lmk [B][L][3] = (x, y, z), cam [B][3] = (s, tx, ty): project_landmarks' first two
//   loss[b] = sum_l w[b,l] |p[b,l] - target[b,l]|^2
// and, from the same registers, g_lmk = d loss[b] / d lmk[b] (z component 0) and g_cam = d loss[b] / d cam[b].  A landmark whose
// weight is exactly 0 is skipped: it adds exact zeros whatever its target holds (NaN marks a missing detection).
// One workgroup per sample, lane = landmark (l = lane, lane + 256, ...: any L), four running sums per lane, then a fixed tree over
// the 256 lanes in LDS: run-to-run identical bits, no atomics.  A few hundred FMAs per sample: latency-bound fp32 VALU.
#include "common.h"

namespace {

__global__ void __launch_bounds__(256) landmark_loss_kernel(const float* __restrict__ lmk, const float* __restrict__ cam,
                                                            const float* __restrict__ target, const float* __restrict__ weight,
                                                            float* __restrict__ loss, float* __restrict__ g_lmk,
                                                            float* __restrict__ g_cam, int L) {
    __shared__ float red[4][256];
    const int b = blockIdx.x, tid = threadIdx.x;
    const float s = cam[3 * b], tx = cam[3 * b + 1], ty = cam[3 * b + 2];
    float acc = 0.f, gs = 0.f, gtx = 0.f, gty = 0.f;
    for (int l = tid; l < L; l += 256) {
        const long i = (long)b * L + l;
        const float w = weight ? weight[i] : 1.f;
        float gx = 0.f, gy = 0.f;
        if (w != 0.f) {
            const float ux = lmk[3 * i] + tx, uy = lmk[3 * i + 1] + ty;
            const float dx = s * ux - target[2 * i], dy = -(s * uy) - target[2 * i + 1];
            const float wx = 2.f * w * dx, wy = 2.f * w * dy;
            acc += w * (dx * dx + dy * dy);
            gs += wx * ux - wy * uy;
            gx = wx * s;
            gy = -(wy * s);
            gtx += gx;
            gty += gy;
        }
        if (g_lmk) {
            g_lmk[3 * i] = gx;
            g_lmk[3 * i + 1] = gy;
            g_lmk[3 * i + 2] = 0.f;
        }
    }
    red[0][tid] = acc; red[1][tid] = gs; red[2][tid] = gtx; red[3][tid] = gty;
    __syncthreads();
    for (int n = 128; n > 0; n >>= 1) {
        if (tid < n) {
#pragma unroll
            for (int q = 0; q < 4; ++q) red[q][tid] += red[q][tid + n];
        }
        __syncthreads();
    }
    if (tid == 0) loss[b] = red[0][0];
    if (g_cam && tid < 3) g_cam[3 * b + tid] = red[1 + tid][0];
}

}  // namespace

extern "C" int gif_landmark_loss_f32(const float* lmk, const float* cam, const float* target, const float* weight, float* loss,
                                     float* g_lmk, float* g_cam, int B, int L, gif_stream_t stream) {
    GIF_REQUIRE(B >= 0 && L >= 0, "landmark_loss: bad dims (B=%d L=%d)", B, L);
    if (B == 0) return 0;
    hipStream_t s = gif::as_stream(stream);
    if (L == 0) {  // empty sums
        hipError_t e = hipSuccess;
        if (loss) e = hipMemsetAsync(loss, 0, (size_t)B * sizeof(float), s);
        if (e == hipSuccess && g_cam) e = hipMemsetAsync(g_cam, 0, (size_t)B * 3 * sizeof(float), s);
        if (e != hipSuccess) { gif::set_error("landmark_loss memset: %s", hipGetErrorString(e)); return (int)e; }
        return 0;
    }
    GIF_REQUIRE(lmk && cam && target && loss, "landmark_loss: null pointer");
    GIF_REQUIRE((long)B * L * 3 < (1L << 31), "landmark_loss: 3 B L must fit 31 bits");
    landmark_loss_kernel<<<B, 256, 0, s>>>(lmk, cam, target, weight, loss, g_lmk, g_cam, L);
    return gif::check_launch("landmark_loss");
}
