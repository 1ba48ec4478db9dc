// Device tracking, the crop (include/onepose_track.h): ophip_crop_resize_gray with the box read from device
// memory, so that the crop of frame t + 1 can be enqueued before frame t's pose is on the host.
//
// The result must equal crop_resize_kernel's (csrc/prep.hip) bit for bit: a grey level that sits on .5 moves with one rounding.  That
// kernel is compiled with contraction on, and which product of a sum of two products the compiler fuses is its choice: the same
// expressions under the same flags came out differently here (the sides are loaded and known to be positive, there they are opaque
// kernel arguments; measured in the ISA: u = mul + add unfused, then v fused the other way round).  So contraction is off in this file
// and the fused operations are written out as that kernel has them (its ISA, gfx950):
//     u = fma(0.5, wb, (X - 0.5 S) inv)     top    = fma(1 - a, p00, a p10)     val = fma(1 - b, top, b bottom)
//     v = fma(0.5, hb, (Y - 0.5 S) inv)     bottom = fma(1 - a, p01, a p11)
// (0.5 S is exact, so X - 0.5 S is the same fused or not).  tests/test_gpu_track_device.py compares the two kernels.
#include <hip/hip_runtime.h>
#include "onepose_track.h"
#include "capi_error.h"

#pragma clang fp contract(off)

namespace {

__global__ __launch_bounds__(256) void crop_box_kernel(const unsigned char* __restrict__ img, int H, int W, const int* __restrict__ box, int S,
                                                       float* __restrict__ out) {
    const int X = blockIdx.x * 32 + (threadIdx.x & 31), Y = blockIdx.y * 8 + (threadIdx.x >> 5);
    if (X >= S || Y >= S) return;
    const int x0 = box[0], y0 = box[1], x1 = box[2], y1 = box[3];
    // no box: an empty crop.  The unsigned differences are the true sides of a non-empty box, so the int ones below cannot overflow
    if (x1 <= x0 || y1 <= y0 || (unsigned)x1 - (unsigned)x0 > (unsigned)OPTRK_MAX_BOX_SIDE || (unsigned)y1 - (unsigned)y0 > (unsigned)OPTRK_MAX_BOX_SIDE) {
        out[(size_t)Y * S + X] = 0.f;
        return;
    }
    const int wb = x1 - x0, hb = y1 - y0;
    const float inv = (float)wb / (float)S;                    // 1 / scale of the second warp
    const float u = fmaf(0.5f, (float)wb, ((float)X - 0.5f * (float)S) * inv);
    const float v = fmaf(0.5f, (float)hb, ((float)Y - 0.5f * (float)S) * inv);
    const float fu = floorf(u), fv = floorf(v);
    const int i0 = (int)fu, j0 = (int)fv;
    const float a = u - fu, b = v - fv;
    auto px = [&](int i, int j) -> float {                     // the box crop with zeros outside it and outside the frame
        if (i < 0 || i >= wb || j < 0 || j >= hb) return 0.f;
        const int x = x0 + i, y = y0 + j;                      // below x1, y1: no overflow
        return (x >= 0 && x < W && y >= 0 && y < H) ? (float)img[(size_t)y * W + x] : 0.f;
    };
    const float top = fmaf(1.f - a, px(i0, j0), a * px(i0 + 1, j0)), bottom = fmaf(1.f - a, px(i0, j0 + 1), a * px(i0 + 1, j0 + 1));
    const float val = fmaf(1.f - b, top, b * bottom);
    out[(size_t)Y * S + X] = fminf(fmaxf(rintf(val), 0.f), 255.f) / 255.0f;      // cv2 writes uint8; astype(float32) / 255 is a true division
}

}  // namespace

extern "C" int optrk_crop(const unsigned char* image, int H, int W, const int* box, int S, float* out, void* stream) {
    if (!image || !box || !out) return capi::bad_arg(__func__, "null pointer");
    if (H < 1 || W < 1 || S < 1 || S > OPTRK_MAX_CROP) return capi::bad_arg(__func__, "bad sizes");
    crop_box_kernel<<<dim3((S + 31) / 32, (S + 7) / 8), dim3(256), 0, (hipStream_t)stream>>>(image, H, W, box, S, out);
    CAPI_CHECK_LAUNCH();
    return 0;
}
