/* libonepose_track.so -- tracking within a sequence on the device (gfx950): the box of frame t + 1 from frame t's device pose, the crop
 * intrinsics of that box, and the crop itself with the box read from device memory.  C ABI; a library of its own, so that every other
 * library is built from exactly the sources it was built from before.  Opt-in (frameloop.SequenceRunner(track="device")): the host's
 * project_bbox / crop_geometry stay the default.
 *
 * The specification is DESIGN.md section 6m; tests/track_device_oracle.py restates the two box entries in numpy float64 with every sum
 * in one fixed order.
 *
 * Every entry returns 0, or -1 on invalid arguments (checked before any launch), or a positive HIP error code; optrk_last_error() says
 * which.  All pointers are device pointers; scalars are passed by value; `stream` is a hipStream_t.  Everything is enqueued on that
 * stream; nothing allocates or synchronises.  The outputs of an entry must not overlap its inputs.
 *
 * The track state of a frame: box int32[4] = [x0, y0, x1, y1], flag int32[1], K_crop float64[9], trans float64[9] (both row-major 3 x 3:
 * frameloop.crop_geometry's pair for that box).
 */
#ifndef ONEPOSE_TRACK_H
#define ONEPOSE_TRACK_H
#ifdef __cplusplus
extern "C" {
#endif

#define OPTRK_ABI_VERSION 1
/* flag bits of a track state (0: the box is the projection with the previous frame's pose, as the host loop would have computed it) */
/* the previous frame's status has OPPNPD_STATUS_NO_POSE, or its n_inliers < min_inliers: the host loop calls the detector */
#define OPTRK_LOST_POSE 1
/* the projected box has x1 <= x0 or y1 <= y0, or a projected coordinate is non-finite or truncates outside int32; tested only when no
 * other bit is set */
#define OPTRK_LOST_BOX 2
/* the previous state's flag was non-zero already: everything downstream of a lost frame is marked */
#define OPTRK_STALE 4
/* the previous frame's status has OPPNPD_STATUS_NEEDS_MORE: the host loop replaces that pose by the host solver's */
#define OPTRK_NEEDS_HOST 8
/* the crop writes zeros for a box wider or taller than this (and for an empty one) */
#define OPTRK_MAX_BOX_SIDE 1073741824
/* the largest crop size S an entry accepts */
#define OPTRK_MAX_CROP 16384

int optrk_abi_version(void);
const char* optrk_last_error(void);

/* A box the host chose (the detector's): box = [x0, y0, x1, y1], flag = 0, K_crop and trans of that box for crop size S and the
 * full-frame intrinsics K [9].  Refuses x1 <= x0, y1 <= y0 and S outside [1, OPTRK_MAX_CROP].  One workgroup. */
int optrk_box_set(int x0, int y0, int x1, int y1, const double* K, int S, int* box, int* flag, double* K_crop, double* trans, void* stream);

/* The box of the next frame.  pose [12] = [R | t] row-major, n_inliers [1], status [1]: one frame of the device PnP's output; bbox3d
 * [8][3]; prev_box [4], prev_flag [1]: the state the posed frame was cropped with.  flag = STALE (prev_flag != 0) | LOST_POSE | NEEDS_HOST
 * as defined above, then LOST_BOX when none of them is set and the projection is unusable.  flag == 0: box = the projection (per corner
 * cam_r = ((R_r0 X + R_r1 Y) + R_r2 Z) + t_r, uvw_r = (K_r0 cam_0 + K_r1 cam_1) + K_r2 cam_2, u = uvw_0 / uvw_2, v = uvw_1 / uvw_2 in
 * float64; minimum and maximum over the eight corners truncated toward zero).  flag != 0: box = prev_box.  K_crop and trans belong to the
 * box that was written: s = S / (x1 - x0), trans = [[s, 0, -s x0], [0, s, S / 2 - s (y0 + (y1 - y0) / 2)], [0, 0, 1]],
 * K_crop_ij = ((trans_i0 K_0j) + (trans_i1 K_1j)) + (trans_i2 K_2j).  Refuses S outside [1, OPTRK_MAX_CROP] and min_inliers < 0.  One workgroup. */
int optrk_box_from_pose(const double* K, const double* pose, const int* n_inliers, const int* status, const double* bbox3d, const int* prev_box,
                        const int* prev_flag, int min_inliers, int S, int* box, int* flag, double* K_crop, double* trans, void* stream);

/* ophip_crop_resize_gray with the box read from device memory: image uint8 [H][W] -> out float [S][S] in [0, 1].  A box with x1 <= x0 or
 * y1 <= y0, or a side above OPTRK_MAX_BOX_SIDE, writes zeros.  Refuses H < 1, W < 1 and S outside [1, OPTRK_MAX_CROP]. */
int optrk_crop(const unsigned char* image, int H, int W, const int* box, int S, float* out, void* stream);

#ifdef __cplusplus
}
#endif
#endif
