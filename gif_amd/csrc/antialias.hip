// Analytic edge antialiasing over the rasteriser's output (gif_antialias_f32 and its backward; the definition is in
// include/gif_hip.h and DESIGN.md §3o).  A post-pass: the rasteriser's kernels and outputs are untouched.
//
// A PAIR is a pixel and its right or lower neighbour with different face indices.  aa_pair below is the whole definition of
// what a pair does: front pixel A, the silhouette edge of tri[A] that crosses the segment A -> B nearest to A, its position a.
// It is a pure function of the inputs, so every kernel that needs a pair evaluates it again and gets the same bits:
//   forward      : one lane per pixel gathers what its (up to four) pairs add to it — both pixels of a pair evaluate the pair, only
//                  the receiver adds; no scatter, no atomics.  Almost every pixel leaves after four face-index compares.
//   d image      : the same gather transposed: a pixel is receiver or donor of each of its pairs.
//   d vertices   : every pair's front pixel A has tri[A] = f and lies in f's clamped bounding box, so one wave per
//                  (image, face, 64-row band) walks the band's rows of the box, keeps the pairs whose front pixel it stands on,
//                  and a fixed xor butterfly sums the lanes; one lane per (image, face) then adds the bands in band order.  The
//                  scheme of gif_rasterize_colors_bwd_f32 (deterministic, no float atomics) without its band-range function:
//                  that one's text is pinned inside rasterize.hip (tests/test_cpu_wiring.py), and a second copy could drift, so
//                  here EVERY (face, band) partial is written — zeros where the box misses the band — and all are added.
// FP contraction is off: t, a and the front-face test decide branches, and a float32 run of the definition must decide alike.
//
// The WALKING variants (gif_antialias_walk_f32 and its backward) are the same kernels with WALK = true: a pair is
// then aa_pair_walk, which goes on from tri[A] across non-silhouette edges, at most max_hops times, to the face that owns the
// outline edge.  The hit's face need no longer be tri[A], so the vertex-gradient wave of face g walks g's bounding box grown by
// one pixel (A lies at most one pixel from the crossing point on g's edge), evaluates the pairs of every covered pixel in it and
// keeps those whose front pixel it stands on and whose hit face is g.  WALK = false: the kernels described above, nothing else.
#include "common.h"
#include "raster_common.h"

#pragma clang fp contract(off)

namespace {

struct AaHit {
    float a, t, den, du, s;  // crossing position; edge parameter; Q.v - P.v; Q.u - P.u; B.u - A.u (u: the pair's axis, v: the other)
    int f, k;                // front face and its chosen edge: corners (k+1)%3 -> (k+2)%3
    bool a_is_p;             // the front pixel is the pair's first (left / upper) pixel
};

// The pair of pixel p = (px, py) and q = p + (1, 0) (axis 0) or p + (0, 1) (axis 1); tp != tq are their face indices.  All
// pointers are those of the pair's image.  false: the pair blends nothing.
__device__ __forceinline__ bool aa_pair(const float* __restrict__ depth, const float* __restrict__ fv, const int32_t* __restrict__ adj,
                                        int F, int W, int px, int py, int axis, int tp, int tq, AaHit& h) {
    const int qx = px + (axis == 0 ? 1 : 0), qy = py + (axis == 0 ? 0 : 1);
    bool a_is_p;
    if (tq < 0) a_is_p = true;
    else if (tp < 0) a_is_p = false;
    else a_is_p = depth[(long)py * W + px] <= depth[(long)qy * W + qx];
    const int f = a_is_p ? tp : tq;
    if (f < 0 || f >= F) return false;  // (a face index the mesh does not have: nothing to intersect)
    const int ax = a_is_p ? px : qx, ay = a_is_p ? py : qy;
    const float Au = (float)(axis == 0 ? ax : ay), Av = (float)(axis == 0 ? ay : ax);
    const float s = a_is_p ? 1.f : -1.f;
    const Face<float> fc = load_face(fv + (long)f * 9);
    const float X[3] = {fc.x0, fc.x1, fc.x2}, Y[3] = {fc.y0, fc.y1, fc.y2};
    bool hit = false;
    float best = 0.f;
#pragma unroll
    for (int k = 0; k < 3; ++k) {
        const int i = (k + 1) % 3, j = (k + 2) % 3;
        const float Pu = axis == 0 ? X[i] : Y[i], Pv = axis == 0 ? Y[i] : X[i];
        const float Qu = axis == 0 ? X[j] : Y[j], Qv = axis == 0 ? Y[j] : X[j];
        const float den = Qv - Pv;
        if (den == 0.f) continue;
        const float t = (Av - Pv) / den;
        const float du = Qu - Pu;
        const float us = Pu + t * du;
        const float a = (us - Au) * s;
        if (!(t >= 0.f && t <= 1.f && a >= 0.f && a <= 1.f)) continue;
        if (hit && !(a < best)) continue;  // smallest a; the lowest k keeps a tie
        const int n = adj[(long)f * 3 + k];
        if (n >= 0 && n < F && front_facing(load_face(fv + (long)n * 9))) continue;  // not a silhouette edge in this image
        hit = true;
        best = a;
        h.a = a; h.t = t; h.den = den; h.du = du; h.k = k;
    }
    h.s = s; h.f = f; h.a_is_p = a_is_p;
    return hit;
}

// aa_pair with the walk of DESIGN.md §3p: where the face `cur` (first tri[A]) has no silhouette edge among its candidates, leave it
// through the candidate nearest to A and ask the neighbour, at most max_hops times; the edge the walk came in through is left
// out; reaching tri[B] ends the walk with nothing (no outline between the two pixels).  h.f is the face that owns the hit edge.
// With max_hops = 0 this makes aa_pair's operations in aa_pair's order.  No array is indexed by a run-time value: no scratch.
__device__ __forceinline__ bool aa_pair_walk(const float* __restrict__ depth, const float* __restrict__ fv,
                                             const int32_t* __restrict__ adj, int F, int W, int px, int py, int axis, int tp, int tq,
                                             int max_hops, AaHit& h) {
    const int qx = px + (axis == 0 ? 1 : 0), qy = py + (axis == 0 ? 0 : 1);
    bool a_is_p;
    if (tq < 0) a_is_p = true;
    else if (tp < 0) a_is_p = false;
    else a_is_p = depth[(long)py * W + px] <= depth[(long)qy * W + qx];
    const int f = a_is_p ? tp : tq, tb = a_is_p ? tq : tp;
    if (f < 0 || f >= F) return false;
    const int ax = a_is_p ? px : qx, ay = a_is_p ? py : qy;
    const float Au = (float)(axis == 0 ? ax : ay), Av = (float)(axis == 0 ? ay : ax);
    const float s = a_is_p ? 1.f : -1.f;
    h.s = s; h.a_is_p = a_is_p;
    int cur = f, prev = -1;
    for (int hop = 0;; ++hop) {
        const Face<float> fc = load_face(fv + (long)cur * 9);
        const float X[3] = {fc.x0, fc.x1, fc.x2}, Y[3] = {fc.y0, fc.y1, fc.y2};
        bool hit = false, leaves = false;  // a silhouette candidate; any other candidate (the way on)
        float best = 0.f, lbest = 0.f;
        int next = -1;
#pragma unroll
        for (int k = 0; k < 3; ++k) {
            const int i = (k + 1) % 3, j = (k + 2) % 3;
            const int n = adj[(long)cur * 3 + k];
            if (hop > 0 && n == prev) continue;  // the edge the walk came in through
            const float Pu = axis == 0 ? X[i] : Y[i], Pv = axis == 0 ? Y[i] : X[i];
            const float Qu = axis == 0 ? X[j] : Y[j], Qv = axis == 0 ? Y[j] : X[j];
            const float den = Qv - Pv;
            if (den == 0.f) continue;
            const float t = (Av - Pv) / den;
            const float du = Qu - Pu;
            const float us = Pu + t * du;
            const float a = (us - Au) * s;
            if (!(t >= 0.f && t <= 1.f && a >= 0.f && a <= 1.f)) continue;
            if (hit && !(a < best)) continue;  // neither a nearer silhouette edge nor, after a hit, of any use as the way on
            if (n >= 0 && n < F && front_facing(load_face(fv + (long)n * 9))) {  // not a silhouette edge in this image
                if (hit || (leaves && !(a < lbest))) continue;  // smallest a; the lowest k keeps a tie
                leaves = true;
                lbest = a;
                next = n;
                continue;
            }
            hit = true;
            best = a;
            h.a = a; h.t = t; h.den = den; h.du = du; h.k = k;
        }
        if (hit) { h.f = cur; return true; }
        if (!leaves || hop >= max_hops || next == tb) return false;
        prev = cur;
        cur = next;
    }
}

// receiver / weight of a hit: a < 0.5: A receives from B with 0.5 - a, else B receives from A with a - 0.5
__device__ __forceinline__ bool aa_receiver_is_a(const AaHit& h) { return h.a < 0.5f; }
__device__ __forceinline__ float aa_weight(const AaHit& h) { return h.a < 0.5f ? 0.5f - h.a : h.a - 0.5f; }

constexpr int kAaThreads = 256;

// The four pairs of pixel (x, y), in the fixed order left, right, upper, lower: other pixel's offset in the image, the pair's first
// pixel and axis, and whether this pixel is the pair's first.
struct AaNeighbour {
    int dx, dy, axis;
    bool me_first;
};
__device__ __forceinline__ AaNeighbour aa_neighbour(int i) {
    switch (i) {
        case 0: return {-1, 0, 0, false};
        case 1: return {1, 0, 0, true};
        case 2: return {0, -1, 1, false};
        default: return {0, 1, 1, true};
    }
}

// BWD = false: out = antialias(image).  BWD = true: `image` is grad_out and `out` is grad_image (the transposed gather).
// WALK: pairs are aa_pair_walk's with max_hops (else max_hops is not read).
template <bool BWD, bool WALK>
__global__ void __launch_bounds__(kAaThreads)
aa_gather(const float* __restrict__ image, const int32_t* __restrict__ tri, const float* __restrict__ depth,
          const float* __restrict__ fv, const int32_t* __restrict__ adj, float* __restrict__ out, long npix, int C, int F, int H,
          int W, int max_hops) {
    const long gp = (long)blockIdx.x * kAaThreads + threadIdx.x;
    if (gp >= npix) return;
    const long hw = (long)H * W;
    const int b = (int)(gp / hw);
    const int p = (int)(gp - b * hw);
    const int y = p / W, x = p - y * W;
    const int32_t* tb = tri + b * hw;
    const int tme = tb[p];
    float wt[4];   // per pair that touches this pixel: the blend weight ...
    long src[4];   // ... the pair's other pixel ...
    bool act[4];   // ... whether the pair touches this pixel at all ...
    bool self[4];  // ... and whether this pixel is the pair's receiver (else its donor: BWD only)
#pragma unroll
    for (int i = 0; i < 4; ++i) {
        act[i] = false; self[i] = false; wt[i] = 0.f; src[i] = 0;
        const AaNeighbour nb = aa_neighbour(i);
        const int ox = x + nb.dx, oy = y + nb.dy;
        if (ox < 0 || ox >= W || oy < 0 || oy >= H) continue;
        const int tother = tb[(long)oy * W + ox];
        if (tother == tme) continue;
        AaHit h;
        const int qx = nb.me_first ? x : ox, qy = nb.me_first ? y : oy;  // the pair's first pixel and the two face indices
        const int t0 = nb.me_first ? tme : tother, t1 = nb.me_first ? tother : tme;
        const bool ok = WALK ? aa_pair_walk(depth + b * hw, fv + (long)b * F * 9, adj, F, W, qx, qy, nb.axis, t0, t1, max_hops, h)
                             : aa_pair(depth + b * hw, fv + (long)b * F * 9, adj, F, W, qx, qy, nb.axis, t0, t1, h);
        if (!ok) continue;
        const bool me_is_a = h.a_is_p == nb.me_first;
        self[i] = aa_receiver_is_a(h) == me_is_a;
        act[i] = BWD || self[i];
        wt[i] = aa_weight(h);
        src[i] = (long)oy * W + ox;
    }
    const float* ib = image + (long)b * C * hw;
    float* ob = out + (long)b * C * hw;
    const bool any = act[0] || act[1] || act[2] || act[3];
    for (int c = 0; c < C; ++c) {
        const float v = ib[c * hw + p];
        float o = v;
        if (any) {
#pragma unroll
            for (int i = 0; i < 4; ++i) {
                if (!act[i]) continue;
                // out[r] = img[r] + w (img[d] - img[r]); transposed: d img[r] -= w g[r], d img[d] += w g[r]
                if (!BWD) o += wt[i] * (ib[c * hw + src[i]] - v);
                else o += self[i] ? -(wt[i] * v) : wt[i] * ib[c * hw + src[i]];
            }
        }
        ob[c * hw + p] = o;
    }
}

constexpr int kAaWaves = 4;   // waves (faces) per band workgroup
constexpr int kAaSums = 6;    // x, y of three corners
constexpr int kAaStride = 8;  // floats per (face, band) partial
constexpr int kAaBand = 64;   // rows per band: a wave walks at most 64 rows x W pixels

inline int aa_bands(int H) { return (H + kAaBand - 1) / kAaBand; }

// WALK: the box is grown by one pixel on every side before it is clamped (not empty even where the face covers no pixel centre),
// every covered pixel in it is a possible front pixel, and a pair counts for this wave if its hit face is fi.
template <bool WALK>
__global__ void __launch_bounds__(kAaWaves * 64)
aa_bwd_band(const float* __restrict__ image, const int32_t* __restrict__ tri, const float* __restrict__ depth,
            const float* __restrict__ fv, const int32_t* __restrict__ adj, const float* __restrict__ g, float* __restrict__ part,
            int C, int F, int H, int W, int bands, int max_hops) {
    const int lane = threadIdx.x & 63;
    const int fi = blockIdx.x * kAaWaves + (threadIdx.x >> 6), band = blockIdx.y, b = blockIdx.z;
    if (fi >= F) return;  // whole wave: fi is uniform across it
    const long fo = (long)b * F + fi;
    const float* fvb = fv + (long)b * F * 9;
    const Face<float> f = load_face(fvb + (long)fi * 9);
    // the band's rows of the face's clamped bounding box; none for a face the rasteriser never lists (it wins no pixel) or a box
    // outside the band: the partial is written all the same (zeros), so the second pass needs no band range
    int x_min = 0, x_max = -1, y_min = 0, y_max = -1;
    if (front_facing(f)) {
        if (!WALK) {
            face_bbox(f, H, W, x_min, x_max, y_min, y_max);
        } else {
            x_min = max((int)ceil(fmin(f.x0, fmin(f.x1, f.x2))) - 1, 0);
            x_max = min((int)floor(fmax(f.x0, fmax(f.x1, f.x2))) + 1, W - 1);
            y_min = max((int)ceil(fmin(f.y0, fmin(f.y1, f.y2))) - 1, 0);
            y_max = min((int)floor(fmax(f.y0, fmax(f.y1, f.y2))) + 1, H - 1);
        }
    }
    const int r0 = max(y_min, band * kAaBand), r1 = min(y_max, band * kAaBand + kAaBand - 1);
    const int cols = x_max - x_min + 1, n = (cols > 0 && r1 >= r0) ? (r1 - r0 + 1) * cols : 0;
    if (n == 0) {  // whole wave: n is uniform across it
        if (lane < kAaSums) part[(fo * bands + band) * kAaStride + lane] = 0.f;
        return;
    }
    const long hw = (long)H * W;
    const int32_t* tb = tri + b * hw;
    const float* ib = image + (long)b * C * hw;
    const float* gb = g + (long)b * C * hw;
    float acc[kAaSums];
#pragma unroll
    for (int k = 0; k < kAaSums; ++k) acc[k] = 0.f;
    for (int p = lane; p < n; p += 64) {
        const int y = r0 + p / cols, x = x_min + p % cols;
        const long me = (long)y * W + x;
        const int tme = WALK ? tb[me] : fi;
        if (WALK ? tme < 0 : tb[me] != fi) continue;
#pragma unroll
        for (int i = 0; i < 4; ++i) {
            const AaNeighbour nb = aa_neighbour(i);
            const int ox = x + nb.dx, oy = y + nb.dy;
            if (ox < 0 || ox >= W || oy < 0 || oy >= H) continue;
            const long other = (long)oy * W + ox;
            const int tother = tb[other];
            if (tother == tme) continue;
            AaHit h;
            const int qx = nb.me_first ? x : ox, qy = nb.me_first ? y : oy;  // the pair's first pixel and the two face indices
            const int t0 = nb.me_first ? tme : tother, t1 = nb.me_first ? tother : tme;
            const bool ok = WALK ? aa_pair_walk(depth + b * hw, fvb, adj, F, W, qx, qy, nb.axis, t0, t1, max_hops, h)
                                 : aa_pair(depth + b * hw, fvb, adj, F, W, qx, qy, nb.axis, t0, t1, h);
            // not the pair's front pixel: the pair is counted where its front pixel is; WALK: another face owns the hit edge
            if (!ok || h.a_is_p != nb.me_first || (WALK && h.f != fi)) continue;
            const bool recv_a = aa_receiver_is_a(h);
            const long r = recv_a ? me : other, d = recv_a ? other : me;
            float dot = 0.f;
            for (int c = 0; c < C; ++c) dot += gb[c * hw + r] * (ib[c * hw + d] - ib[c * hw + r]);
            const float ga = recv_a ? -dot : dot;  // weight = |a - 0.5|
            // a = (us - A.u) s, us = P.u + t du, du = Q.u - P.u, t = (A.v - P.v) / den, den = Q.v - P.v
            const float gus = ga * h.s;
            const float gt = gus * h.du;
            const float gQu = gus * h.t, gPu = gus - gQu;
            const float gnum = gt / h.den;
            const float gQv = -(gnum * h.t), gPv = -gnum - gQv;
            const float gPx = nb.axis == 0 ? gPu : gPv, gPy = nb.axis == 0 ? gPv : gPu;
            const float gQx = nb.axis == 0 ? gQu : gQv, gQy = nb.axis == 0 ? gQv : gQu;
#pragma unroll
            for (int j = 0; j < 3; ++j) {
                if (j == (h.k + 1) % 3) { acc[2 * j] += gPx; acc[2 * j + 1] += gPy; }
                if (j == (h.k + 2) % 3) { acc[2 * j] += gQx; acc[2 * j + 1] += gQy; }
            }
        }
    }
#pragma unroll
    for (int m = 32; m > 0; m >>= 1)
#pragma unroll
        for (int k = 0; k < kAaSums; ++k) acc[k] += __shfl_xor(acc[k], m, 64);
    if (lane == 0) {
        float* o = part + (fo * bands + band) * kAaStride;
#pragma unroll
        for (int k = 0; k < kAaSums; ++k) o[k] = acc[k];
    }
}

__global__ void __launch_bounds__(256)
aa_bwd_reduce(const float* __restrict__ part, float* __restrict__ gfv, long faces, int bands) {
    const long fo = (long)blockIdx.x * blockDim.x + threadIdx.x;
    if (fo >= faces) return;
    float s[kAaSums];
#pragma unroll
    for (int k = 0; k < kAaSums; ++k) s[k] = 0.f;
    for (int band = 0; band < bands; ++band) {  // every (face, band) partial was written
        const float* pp = part + (fo * bands + band) * kAaStride;
#pragma unroll
        for (int k = 0; k < kAaSums; ++k) s[k] += pp[k];
    }
    float* o = gfv + fo * 9;
#pragma unroll
    for (int j = 0; j < 3; ++j) {
        o[3 * j + 0] = s[2 * j];
        o[3 * j + 1] = s[2 * j + 1];
        o[3 * j + 2] = 0.f;  // depth only chooses the front pixel
    }
}

int aa_check_dims(const char* who, int B, int C, int F, int H, int W) {
    GIF_REQUIRE(B >= 0 && F >= 0 && H > 0 && W > 0 && C >= 1, "%s: bad dims B=%d C=%d F=%d H=%d W=%d", who, B, C, F, H, W);
    GIF_REQUIRE((long)H * W < (1L << 31) && (long)B * C * H * W < (1L << 40) && (long)B * H * W < (1L << 31) * kAaThreads,
                "%s: image too large", who);
    return 0;
}

constexpr int kAaMaxHops = 64;

// max_hops < 0: the pairs of aa_pair (gif_antialias_f32); else the walking pairs (gif_antialias_walk_f32)
int aa_forward(const char* who, const float* image, const int32_t* tri, const float* depth, const float* face_vertices,
               const int32_t* edge_adj, float* out, int B, int C, int F, int H, int W, int max_hops, gif_stream_t stream) {
    if (B == 0) return 0;
    hipStream_t s = gif::as_stream(stream);
    if (F == 0) {  // no faces: no pairs
        if (!image || !out) return 0;
        hipError_t e = hipMemcpyAsync(out, image, (size_t)B * C * H * W * sizeof(float), hipMemcpyDeviceToDevice, s);
        if (e != hipSuccess) { gif::set_error("%s copy: %s", who, hipGetErrorString(e)); return (int)e; }
        return 0;
    }
    GIF_REQUIRE(image && tri && depth && face_vertices && edge_adj && out, "%s: null pointer", who);
    GIF_REQUIRE(image != out, "%s: out must not alias image", who);
    const long npix = (long)B * H * W;
    const unsigned grid = (unsigned)gif::cdiv(npix, kAaThreads);
    if (max_hops < 0)
        aa_gather<false, false><<<grid, kAaThreads, 0, s>>>(image, tri, depth, face_vertices, edge_adj, out, npix, C, F, H, W, 0);
    else
        aa_gather<false, true><<<grid, kAaThreads, 0, s>>>(image, tri, depth, face_vertices, edge_adj, out, npix, C, F, H, W,
                                                           max_hops);
    return gif::check_launch(who);
}

int aa_backward(const char* who, const float* image, const int32_t* tri, const float* depth, const float* face_vertices,
                const int32_t* edge_adj, const float* grad_out, float* grad_image, float* grad_face_vertices, int B, int C, int F,
                int H, int W, int max_hops, void* workspace, gif_stream_t stream) {
    if (B == 0) return 0;
    hipStream_t s = gif::as_stream(stream);
    if (F == 0) {
        if (!grad_out || !grad_image) return 0;
        hipError_t e = hipMemcpyAsync(grad_image, grad_out, (size_t)B * C * H * W * sizeof(float), hipMemcpyDeviceToDevice, s);
        if (e != hipSuccess) { gif::set_error("%s copy: %s", who, hipGetErrorString(e)); return (int)e; }
        return 0;
    }
    GIF_REQUIRE(tri && depth && face_vertices && edge_adj && grad_out, "%s: null pointer", who);
    GIF_REQUIRE(grad_image || grad_face_vertices, "%s: no output", who);
    GIF_REQUIRE(grad_image != grad_out, "%s: grad_image must not alias grad_out", who);
    const int bands = aa_bands(H);
    if (grad_face_vertices) {
        GIF_REQUIRE(image && workspace, "%s: the vertex gradient needs image and workspace", who);
        GIF_REQUIRE(((uintptr_t)workspace & 3) == 0, "%s: workspace must be 4-byte aligned", who);
        GIF_REQUIRE(B <= 65535 && bands <= 65535 && (long)B * F * bands * kAaStride < (1L << 40), "%s: too many images / faces", who);
    }
    if (grad_image) {
        const long npix = (long)B * H * W;
        const unsigned grid = (unsigned)gif::cdiv(npix, kAaThreads);
        if (max_hops < 0)
            aa_gather<true, false><<<grid, kAaThreads, 0, s>>>(grad_out, tri, depth, face_vertices, edge_adj, grad_image, npix, C, F,
                                                               H, W, 0);
        else
            aa_gather<true, true><<<grid, kAaThreads, 0, s>>>(grad_out, tri, depth, face_vertices, edge_adj, grad_image, npix, C, F,
                                                              H, W, max_hops);
    }
    if (grad_face_vertices) {
        float* part = reinterpret_cast<float*>(workspace);
        const dim3 grid((unsigned)gif::cdiv(F, kAaWaves), (unsigned)bands, (unsigned)B);
        if (max_hops < 0)
            aa_bwd_band<false><<<grid, kAaWaves * 64, 0, s>>>(image, tri, depth, face_vertices, edge_adj, grad_out, part, C, F, H, W,
                                                              bands, 0);
        else
            aa_bwd_band<true><<<grid, kAaWaves * 64, 0, s>>>(image, tri, depth, face_vertices, edge_adj, grad_out, part, C, F, H, W,
                                                             bands, max_hops);
        aa_bwd_reduce<<<gif::cdiv((long)B * F, 256), 256, 0, s>>>(part, grad_face_vertices, (long)B * F, bands);
    }
    return gif::check_launch(who);
}

}  // namespace

extern "C" {

int gif_antialias_f32(const float* image, const int32_t* tri, const float* depth, const float* face_vertices,
                      const int32_t* edge_adj, float* out, int B, int C, int F, int H, int W, gif_stream_t stream) {
    if (int rc = aa_check_dims("antialias", B, C, F, H, W)) return rc;
    return aa_forward("antialias", image, tri, depth, face_vertices, edge_adj, out, B, C, F, H, W, -1, stream);
}

int gif_antialias_walk_f32(const float* image, const int32_t* tri, const float* depth, const float* face_vertices,
                           const int32_t* edge_adj, float* out, int B, int C, int F, int H, int W, int max_hops,
                           gif_stream_t stream) {
    if (int rc = aa_check_dims("antialias_walk", B, C, F, H, W)) return rc;
    GIF_REQUIRE(max_hops >= 0 && max_hops <= kAaMaxHops, "antialias_walk: max_hops %d outside 0 .. %d", max_hops, kAaMaxHops);
    return aa_forward("antialias_walk", image, tri, depth, face_vertices, edge_adj, out, B, C, F, H, W, max_hops, stream);
}

int64_t gif_antialias_bwd_workspace_bytes(int B, int F, int H, int W) {
    if (B <= 0 || F <= 0 || H <= 0 || W <= 0) return 8;
    return (int64_t)B * F * aa_bands(H) * kAaStride * 4;
}

int gif_antialias_bwd_f32(const float* image, const int32_t* tri, const float* depth, const float* face_vertices,
                          const int32_t* edge_adj, const float* grad_out, float* grad_image, float* grad_face_vertices, int B,
                          int C, int F, int H, int W, void* workspace, gif_stream_t stream) {
    if (int rc = aa_check_dims("antialias_bwd", B, C, F, H, W)) return rc;
    return aa_backward("antialias_bwd", image, tri, depth, face_vertices, edge_adj, grad_out, grad_image, grad_face_vertices, B, C, F,
                       H, W, -1, workspace, stream);
}

int gif_antialias_walk_bwd_f32(const float* image, const int32_t* tri, const float* depth, const float* face_vertices,
                               const int32_t* edge_adj, const float* grad_out, float* grad_image, float* grad_face_vertices, int B,
                               int C, int F, int H, int W, int max_hops, void* workspace, gif_stream_t stream) {
    if (int rc = aa_check_dims("antialias_walk_bwd", B, C, F, H, W)) return rc;
    GIF_REQUIRE(max_hops >= 0 && max_hops <= kAaMaxHops, "antialias_walk_bwd: max_hops %d outside 0 .. %d", max_hops, kAaMaxHops);
    return aa_backward("antialias_walk_bwd", image, tri, depth, face_vertices, edge_adj, grad_out, grad_image, grad_face_vertices, B,
                       C, F, H, W, max_hops, workspace, stream);
}
}
