// Face geometry shared by the rasteriser (rasterize.hip) and the pass that reads its buffers (antialias.hip): the reference's
// front-face test and clamped bounding box.  Arithmetic follows the reference operation by operation with FP contraction off (a
// comparison decides every branch here), so both sources see the same bits.
#pragma once
#include "common.h"

#pragma clang fp contract(off)

namespace {

template <typename T>
struct Face {
    T x0, y0, z0, x1, y1, z1, x2, y2, z2;
};

template <typename T>
__device__ __forceinline__ Face<T> load_face(const T* __restrict__ p) {
    Face<T> f;
    f.x0 = p[0]; f.y0 = p[1]; f.z0 = p[2];
    f.x1 = p[3]; f.y1 = p[4]; f.z1 = p[5];
    f.x2 = p[6]; f.y2 = p[7]; f.z2 = p[8];
    return f;
}

// check_face_frontside, .cu:31-34
template <typename T>
__device__ __forceinline__ bool front_facing(const Face<T>& f) {
    return (f.y2 - f.y0) * (f.x1 - f.x0) < (f.y1 - f.y0) * (f.x2 - f.x0);
}

// bbox of a face clamped to the image, .cu:133-136
template <typename T>
__device__ __forceinline__ void face_bbox(const Face<T>& f, int H, int W, int& x_min, int& x_max, int& y_min, int& y_max) {
    x_min = max((int)ceil(fmin(f.x0, fmin(f.x1, f.x2))), 0);
    x_max = min((int)floor(fmax(f.x0, fmax(f.x1, f.x2))), W - 1);
    y_min = max((int)ceil(fmin(f.y0, fmin(f.y1, f.y2))), 0);
    y_max = min((int)floor(fmax(f.y0, fmax(f.y1, f.y2))), H - 1);
}

}  // namespace
