// Device tracking, the crop (include/onepose_track.h): ophip_crop_resize_gray with the box read from device
// memory, so that the crop of frame t + 1 can be enqueued before frame t's pose is on the host; the pixel is crop_pixel.h's, as in
// crop_resize_kernel of prep.hip, so the two agree bit for bit.
#include <hip/hip_runtime.h>
#include "onepose_track.h"
#include "capi_error.h"
#include "crop_pixel.h"

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
    out[(size_t)Y * S + X] = crop_pixel(img, H, W, x0, y0, x1 - x0, y1 - y0, S, X, Y);
}

}  // namespace

extern "C" int optrk_crop(const unsigned char* image, int H, int W, const int* box, int S, float* out, void* stream) {
    if (!image || !box || !out) return capi::bad_arg(__func__, "null pointer");
    if (H < 1 || W < 1 || S < 1 || S > OPTRK_MAX_CROP) return capi::bad_arg(__func__, "bad sizes");
    crop_box_kernel<<<dim3((S + 31) / 32, (S + 7) / 8), dim3(256), 0, (hipStream_t)stream>>>(image, H, W, box, S, out);
    CAPI_CHECK_LAUNCH();
    return 0;
}
