// Device tracking, the box entries (include/onepose_track.h): the box of frame t + 1 from frame t's device pose
// (frameloop.project_bbox), and the crop intrinsics of a box (frameloop.crop_geometry), in float64 with every sum in the order the
// header writes it.  One workgroup of one wave per call:
//
//   box_from_pose_kernel   lanes 0-7 project one corner each into LDS; lane 0 forms the flag, reduces the corners in corner order and
//                          writes box and flag; lanes 0-8 write one entry of trans and K_crop each
//   box_set_kernel         lane 0 writes the given box and flag 0; lanes 0-8 the same geometry
//
// Every value is a fixed expression of the inputs, so the lane layout cannot change a bit.  Nothing is indexed by a device-side value:
// the status, the counts and the boxes only select between values.  Compiled with contraction off.
#include <hip/hip_runtime.h>
#include "onepose_pnp_device.h"
#include "onepose_track.h"
#include "capi_error.h"
#include "device_loop.h"

using devloop::fits_int32;
using devloop::geometry_entry;

#pragma clang fp contract(off)

namespace {

constexpr int kThreads = 64;                      // one wave

__global__ __launch_bounds__(kThreads) void box_set_kernel(int x0, int y0, int x1, int y1, const double* __restrict__ K, int S, int* __restrict__ box,
                                                           int* __restrict__ flag, double* __restrict__ K_crop, double* __restrict__ trans) {
    const int tid = threadIdx.x;
    const int b[4] = {x0, y0, x1, y1};
    if (tid == 0) {
        box[0] = x0; box[1] = y0; box[2] = x1; box[3] = y1;
        *flag = 0;
    }
    if (tid < 9) geometry_entry(b, K, S, tid, K_crop, trans);
}

__global__ __launch_bounds__(kThreads) void box_from_pose_kernel(const double* __restrict__ K, const double* __restrict__ pose,
                                                                 const int* __restrict__ n_inliers, const int* __restrict__ status,
                                                                 const double* __restrict__ bbox3d, const int* __restrict__ prev_box,
                                                                 const int* __restrict__ prev_flag, int min_inliers, int S, int* __restrict__ box,
                                                                 int* __restrict__ flag, double* __restrict__ K_crop, double* __restrict__ trans) {
    __shared__ double uv[8][2];
    __shared__ int sbox[4];
    const int tid = threadIdx.x;
    if (tid < 8) {
        const double X = bbox3d[3 * tid], Y = bbox3d[3 * tid + 1], Z = bbox3d[3 * tid + 2];
        const double c0 = ((pose[0] * X + pose[1] * Y) + pose[2] * Z) + pose[3];
        const double c1 = ((pose[4] * X + pose[5] * Y) + pose[6] * Z) + pose[7];
        const double c2 = ((pose[8] * X + pose[9] * Y) + pose[10] * Z) + pose[11];
        const double w0 = (K[0] * c0 + K[1] * c1) + K[2] * c2;
        const double w1 = (K[3] * c0 + K[4] * c1) + K[5] * c2;
        const double w2 = (K[6] * c0 + K[7] * c1) + K[8] * c2;
        uv[tid][0] = w0 / w2;
        uv[tid][1] = w1 / w2;
    }
    __syncthreads();
    if (tid == 0) {
        int f = 0;
        const int st = *status;
        if (*prev_flag != 0) f |= OPTRK_STALE;
        if ((st & OPPNPD_STATUS_NO_POSE) || *n_inliers < min_inliers) f |= OPTRK_LOST_POSE;
        if (st & OPPNPD_STATUS_NEEDS_MORE) f |= OPTRK_NEEDS_HOST;
        int b0 = prev_box[0], b1 = prev_box[1], b2 = prev_box[2], b3 = prev_box[3];
        if (f == 0) {
            bool ok = true;
            double lo_u = uv[0][0], lo_v = uv[0][1], hi_u = lo_u, hi_v = lo_v;
#pragma unroll
            for (int c = 0; c < 8; ++c) {
                const double u = uv[c][0], v = uv[c][1];
                ok = ok && fits_int32(u) && fits_int32(v);
                lo_u = u < lo_u ? u : lo_u; hi_u = u > hi_u ? u : hi_u;
                lo_v = v < lo_v ? v : lo_v; hi_v = v > hi_v ? v : hi_v;
            }
            int p0 = 0, p1 = 0, p2 = 0, p3 = 0;
            if (ok) {                                     // every coordinate fits, so the conversions are defined
                p0 = (int)lo_u; p1 = (int)lo_v; p2 = (int)hi_u; p3 = (int)hi_v;
                ok = p2 > p0 && p3 > p1;
            }
            if (ok) {
                b0 = p0; b1 = p1; b2 = p2; b3 = p3;
            } else {
                f |= OPTRK_LOST_BOX;
            }
        }
        sbox[0] = b0; sbox[1] = b1; sbox[2] = b2; sbox[3] = b3;
        box[0] = b0; box[1] = b1; box[2] = b2; box[3] = b3;
        *flag = f;
    }
    __syncthreads();
    if (tid < 9) geometry_entry(sbox, K, S, tid, K_crop, trans);
}

}  // namespace

extern "C" {

int optrk_abi_version(void) { return OPTRK_ABI_VERSION; }
const char* optrk_last_error(void) { return capi::g_error; }

int optrk_box_set(int x0, int y0, int x1, int y1, const double* K, int S, int* box, int* flag, double* K_crop, double* trans, void* stream) {
    if (!K || !box || !flag || !K_crop || !trans) return capi::bad_arg(__func__, "null pointer");
    if (S < 1 || S > OPTRK_MAX_CROP) return capi::bad_arg(__func__, "crop size S outside [1, OPTRK_MAX_CROP]");
    if (x1 <= x0 || y1 <= y0) return capi::bad_arg(__func__, "empty box (need x1 > x0, y1 > y0)");
    box_set_kernel<<<1, kThreads, 0, (hipStream_t)stream>>>(x0, y0, x1, y1, K, S, box, flag, K_crop, trans);
    CAPI_CHECK_LAUNCH();
    return 0;
}

int optrk_box_from_pose(const double* K, const double* pose, const int* n_inliers, const int* status, const double* bbox3d, const int* prev_box,
                        const int* prev_flag, int min_inliers, int S, int* box, int* flag, double* K_crop, double* trans, void* stream) {
    if (!K || !pose || !n_inliers || !status || !bbox3d || !prev_box || !prev_flag || !box || !flag || !K_crop || !trans)
        return capi::bad_arg(__func__, "null pointer");
    if (S < 1 || S > OPTRK_MAX_CROP) return capi::bad_arg(__func__, "crop size S outside [1, OPTRK_MAX_CROP]");
    if (min_inliers < 0) return capi::bad_arg(__func__, "min_inliers < 0");
    box_from_pose_kernel<<<1, kThreads, 0, (hipStream_t)stream>>>(K, pose, n_inliers, status, bbox3d, prev_box, prev_flag, min_inliers, S, box, flag,
                                                                  K_crop, trans);
    CAPI_CHECK_LAUNCH();
    return 0;
}

}  // extern "C"
