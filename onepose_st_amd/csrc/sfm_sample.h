// The keypoint-to-cell and grid-sample arithmetic of the SfM matcher, written once: loftr_sfm.hip (one image pair per call, sizes and
// scales as launch arguments) and sfm_fine.hip (a whole pair list, sizes and scales looked up per row) must give the same ids and the
// same samples bit for bit, so both call these functions and keep only their argument structs, look-ups, bad-id accounting and stores.
//
// Every step is written in the reference's order of operations and rounding (loftr_for_sfm/loftr.py:79-167,
// utils/sample_feature_from_featuremap.py:6-80), in the keypoints' own dtype.  Contraction into FMA is switched off inside each function
// body, not at file scope: the main library compiles its other files with contraction on, and a file-scope pragma here would reach them.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

namespace sfmsample {

typedef float f32x4 __attribute__((ext_vector_type(4)));

__device__ __forceinline__ float rint_t(float v) { return rintf(v); }          // torch.round / nearbyint: half to even
__device__ __forceinline__ double rint_t(double v) { return rint(v); }

// torch.clip(v, 0, vmax) (NaN stays NaN)
template <typename T>
__device__ __forceinline__ T clip(T v, T vmax) {
    return v < T(0) ? T(0) : (v > vmax ? vmax : v);
}

// the coarse cell of a clipped keypoint: sx, sy = scale * scale[b_ids][:, [1, 0]] (x by the w factor, y by the h factor, f32), the
// division in the promoted dtype, round half to even, row * wc + column; .long() truncates, and -1 flags NaN, negatives and >= 9.0e18
template <typename T>
__device__ __forceinline__ long long cell_id(T x, T y, float sx, float sy, int wc) {
#pragma clang fp contract(off)
    const T rx = rint_t(x / (T)sx), ry = rint_t(y / (T)sy);
    const T v = ry * (T)wc + rx;
    return (v >= T(0) && v < T(9.0e18)) ? (long long)v : -1;
}

// coord_normalization (scale 1): ((k - 0.5 + 0.5) / (extent - 1)) * 2 - 1 in the keypoints' dtype, then .float()
template <typename T>
__device__ __forceinline__ float normalise(T k, float extent) {
#pragma clang fp contract(off)
    const T den = (T)(extent - 1.0f);
    T g = k - T(0.5);
    g = g + T(0.5);
    g = g / den;
    g = g * T(2);
    g = g - T(1);
    return (float)g;
}

__device__ __forceinline__ f32x4 row4(const float* map, int w, int C, int y, int x, int c4) {
    return *reinterpret_cast<const f32x4*>(map + ((size_t)y * w + x) * C + 4 * c4);
}

// F.grid_sample(map, normalised keypoint, align_corners=True, zero padding) of one keypoint: channels 4 lane .. 4 lane + 3 of the
// channels-last map [h * w][C].  kp: the (x, y) of the keypoint in image pixels, f64 if kp_double, f32 otherwise; eh, ew: the image
// extents scale * (H, W) it is normalised by; nearest: the rounded cell, otherwise the four bilinear corners
__device__ __forceinline__ f32x4 sample_row(const float* map, int h, int w, int C, const void* kp, int kp_double, float eh, float ew,
                                            int nearest, int lane) {
#pragma clang fp contract(off)
    float gx, gy;
    if (kp_double) {
        const double* k = static_cast<const double*>(kp);
        gx = normalise<double>(k[0], ew);
        gy = normalise<double>(k[1], eh);
    } else {
        const float* k = static_cast<const float*>(kp);
        gx = normalise<float>(k[0], ew);
        gy = normalise<float>(k[1], eh);
    }
    // grid_sampler_unnormalize, align_corners: ((g + 1) / 2) * (size - 1)
    const float ix = ((gx + 1.f) / 2.f) * (float)(w - 1), iy = ((gy + 1.f) / 2.f) * (float)(h - 1);
    f32x4 o = {0.f, 0.f, 0.f, 0.f};
    if (nearest) {
        const float rx = rintf(ix), ry = rintf(iy);
        if (rx >= 0.f && rx <= (float)(w - 1) && ry >= 0.f && ry <= (float)(h - 1)) o = row4(map, w, C, (int)ry, (int)rx, lane);
    } else if (ix > -1.f && ix < (float)w && iy > -1.f && iy < (float)h) {
        // the four corners and weights of PyTorch's bilinear grid_sample, summed nw, ne, sw, se; corners outside the map add nothing
        const float fx = floorf(ix), fy = floorf(iy);
        const int x0 = (int)fx, y0 = (int)fy;
        const float x1f = fx + 1.f, y1f = fy + 1.f;
        const float wnw = (x1f - ix) * (y1f - iy), wne = (ix - fx) * (y1f - iy);
        const float wsw = (x1f - ix) * (iy - fy), wse = (ix - fx) * (iy - fy);
        const bool xin0 = x0 >= 0, xin1 = x0 + 1 < w, yin0 = y0 >= 0, yin1 = y0 + 1 < h;
        if (yin0 && xin0) { const f32x4 v = row4(map, w, C, y0, x0, lane); o = o + v * wnw; }
        if (yin0 && xin1) { const f32x4 v = row4(map, w, C, y0, x0 + 1, lane); o = o + v * wne; }
        if (yin1 && xin0) { const f32x4 v = row4(map, w, C, y0 + 1, x0, lane); o = o + v * wsw; }
        if (yin1 && xin1) { const f32x4 v = row4(map, w, C, y0 + 1, x0 + 1, lane); o = o + v * wse; }
    }
    return o;
}

}  // namespace sfmsample
