/* libonepose_pnp_device.so -- the pose of a frame from the matcher's device-side output, on the device (gfx950): P3P RANSAC with a fixed
 * number of trials, every root scored on every match, the winner refined by Levenberg-Marquardt, in float64.  C ABI; a library of its
 * own, so that every other library is built from exactly the sources it was built from before.  Opt-in: the host solver
 * (include/onepose_pnp.h) stays the default.
 *
 * The specification is the project's own (onepose_st_amd/pnp_device.py; tests/pnp_device_oracle.py restates it in
 * numpy): the host solver's P3P, inlier test and refinement, with a counter-based sampler in place of the host's sequential generator.
 *
 * Every entry returns 0, or -1 on invalid arguments, or a positive HIP error code; oppnpd_last_error() says which.  All pointers are
 * device pointers; `stream` is a hipStream_t; nothing is synchronised.  `count` (int32[1] on the device) is clamped to `cap`; rows at or
 * beyond it are never read.  `b_ids [cap]` ascending names the frame of every row (NULL: one frame); a row whose id lies outside
 * [0, F) belongs to no frame.  `K` is [F][9], or [1][9] with k_shared != 0.  Every kernel refuses to index outside its tables whatever
 * `count`, `b_ids` or the intermediate tables hold.
 */
#ifndef ONEPOSE_PNP_DEVICE_H
#define ONEPOSE_PNP_DEVICE_H
#include <stddef.h>
#ifdef __cplusplus
extern "C" {
#endif

#define OPPNPD_ABI_VERSION 1
#define OPPNPD_MAX_TRIALS 65536
#define OPPNPD_DEFAULT_TRIALS 10240
#define OPPNPD_MAX_ROWS 16777216
#define OPPNPD_MAX_FRAMES 4096
/* doubles per prepared row: X = scale * pts3d (3), the pixel (2), the ray K^-1 (u, v, 1) / w (2), one pad */
#define OPPNPD_ROW_DOUBLES 8
/* hypotheses a select workgroup reduces; rows of a frame the score kernel stages through LDS at a time */
#define OPPNPD_SELECT_BLOCK 1024
#define OPPNPD_SCORE_CHUNK 256
/* status bits */
#define OPPNPD_STATUS_NO_POSE 1
#define OPPNPD_STATUS_NEEDS_MORE 4
/* a pose must keep this many inliers (the sample and the point that picks the root); frames with fewer rows run no trials */
#define OPPNPD_MIN_INLIERS 4
/* what the confidence formula is clamped to (the host's reference policy: max_num_trials) */
#define OPPNPD_MAX_NEEDED 1000000
#define OPPNPD_LM_ITERS 20
#define OPPNPD_LM_TRIES 8
#define OPPNPD_LM_ROUNDS 2

int oppnpd_abi_version(void);
const char* oppnpd_last_error(void);

/* bytes of the workspace oppnpd_solve needs */
size_t oppnpd_workspace_bytes(int cap, int F, int trials);

/* Stage 1a: ranges [F][2] int32 = [begin, end) of every frame's rows, by binary search in b_ids[0 .. min(count, cap)). */
int oppnpd_ranges(const long long* b_ids, const int* count, int cap, int F, int* ranges, void* stream);

/* Stage 1b: rows [cap][OPPNPD_ROW_DOUBLES] of the rows below the count; a row of no frame is written as zeros. */
int oppnpd_prep(const float* pts2d, const float* pts3d, const int* count, int cap, const long long* b_ids, int F, const double* K,
                int k_shared, double scale, double* rows, void* stream);

/* Stage 2: samples [F][trials][3] int32, frame-local row numbers, three distinct ones per trial; -1 in a frame of fewer than
 * OPPNPD_MIN_INLIERS rows.  Trial t of frame f, pick k: h = mix(seed + G * (((f << 32 | t) * 4 + k) + 1)) with G = 0x9E3779B97F4A7C15
 * and mix the splitmix64 finaliser; index h % (n - k), stepped past the earlier picks in ascending order. */
int oppnpd_sample(const int* ranges, int F, int trials, unsigned long long seed, int* samples, void* stream);

/* Stage 3: hyps [F][4 * trials][12] = up to four poses [R | t] per trial, the valid roots first in the solver's root order; unused
 * slots are filled with NaN.  nsol [F][trials] int32 = the number of poses of every trial. */
int oppnpd_p3p(const double* rows, const int* ranges, const int* samples, int cap, int F, int trials, double* hyps, int* nsol,
               void* stream);

/* Stage 4: cnt [F][H] int32, cost [F][H] float64 of H hypotheses per frame on the frame's rows, in row order.  A hypothesis with a
 * non-finite entry: count 0, cost +inf. */
int oppnpd_score(const double* rows, const int* ranges, const double* K, int k_shared, const double* hyps, int cap, int F, int H,
                 double reproj_err_px, int* cnt, double* cost, void* stream);

/* Stage 5: best [F] int32 = the winner under (count descending, cost ascending, index ascending), -1 when H hypotheses hold none with a
 * count > 0; n_inliers [F] its count; status [F]: OPPNPD_STATUS_NO_POSE when the count is below OPPNPD_MIN_INLIERS,
 * OPPNPD_STATUS_NEEDS_MORE when the frame has at least OPPNPD_MIN_INLIERS rows and the confidence asks for more than `trials` trials;
 * inlier_mask [cap] = the winner's inliers on its frame's rows, 0 on every other row below the count.
 * partial: ceil(H / OPPNPD_SELECT_BLOCK) * F entries of 16 bytes. */
int oppnpd_select(const int* cnt, const double* cost, const double* rows, const int* ranges, const int* count, const double* K,
                  int k_shared, const double* hyps, int cap, int F, int H, double reproj_err_px, double confidence, int trials,
                  void* partial, int* best, int* n_inliers, int* status, unsigned char* inlier_mask, void* stream);

/* Stage 6: one workgroup per frame: LM on the masked rows, the inlier set re-evaluated, a second round unless it is unchanged.
 * pose [F][12] with t divided by scale; n_inliers, status and inlier_mask updated.  No pose: the identity, an empty mask. */
int oppnpd_refine(const double* rows, const int* ranges, const double* K, int k_shared, const double* hyps, const int* best, int cap,
                  int F, int H, double reproj_err_px, double scale, double* pose, int* n_inliers, int* status,
                  unsigned char* inlier_mask, void* stream);

/* All stages on one stream. */
int oppnpd_solve(const float* pts2d, const float* pts3d, const int* count, int cap, const long long* b_ids, int F, const double* K,
                 int k_shared, double scale, double reproj_err_px, double confidence, int trials, unsigned long long seed,
                 void* workspace, size_t workspace_bytes, double* pose, int* n_inliers, int* status, unsigned char* inlier_mask,
                 void* stream);

#ifdef __cplusplus
}
#endif
#endif
