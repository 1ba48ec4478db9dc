/* libonepose_detect.so -- the object detector's vote on the device (gfx950): one affine RANSAC per reference view on the LoFTR matcher's
 * device-side matches, the box every view votes, the winning view and the track state of its box.  C ABI; a library of its own, so that
 * every other library is built from exactly the sources it was built from before.  Opt-in (detector.LocalFeatureObjectDetector(vote=
 * "device"), frameloop.SequenceRunner(detect="device")): the host vote (oppnp_estimate_affine2d per view) stays the default.
 *
 * The specification is the project's own (tests/detect_device_oracle.py restates it in numpy float64): the host
 * estimator's model, inlier rule and fit (csrc_host/pnp.cpp: affine_from3, affine_inliers, the normal equations of
 * oppnp_estimate_affine2d), with its sequential generator and adaptive stop replaced by a fixed number of counter-based trials.  All
 * arithmetic is float64 from the float32 points, evaluated in the written order (contraction off).
 *
 *   ranges      [V][2] int32 = [begin, end) of every view's rows, by binary search in b_ids[0 .. min(count, cap)).
 *   sample      Trial t of view v, pick k = 0, 1, 2: h = mix(seed + G * (((v << 32 | t) * 4 + k) + 1)) with G = 0x9E3779B97F4A7C15 and mix
 *               the splitmix64 finaliser (arithmetic mod 2^64); index h % (n - k), stepped past the earlier picks in ascending order:
 *               three distinct view-local rows.  A view of fewer than max(min_matches, 3) rows runs no trials (samples -1, counts 0).
 *   hypothesis  affine_from3 on the three rows (x, y) -> (u, v): det = (x1 - x0) (y2 - y0) - (x2 - x0) (y1 - y0), scale = |x1 - x0| +
 *               |y1 - y0| + |x2 - x0| + |y2 - y0|; degenerate unless |det| > 1e-9 scale^2 and scale > 0; per output coordinate w (u, then v)
 *               a = ((w1 - w0) (y2 - y0) - (w2 - w0) (y1 - y0)) / det, b = ((x1 - x0) (w2 - w0) - (x2 - x0) (w1 - w0)) / det,
 *               c = w0 - a x0 - b y0.  A degenerate sample counts 0.
 *   score       A row is an inlier when ex^2 + ey^2 < thr^2 with ex = A0 x + A1 y + A2 - u, ey = A3 x + A4 y + A5 - v (left to right).  The
 *               count of a trial is the number of inliers among its view's rows: integers, so no order matters.
 *   select      The winning trial of a view: the highest count, the lowest trial among equals; none when every count is 0.  n_inliers =
 *               its count, inlier_mask = its inliers on the view's rows (0 on every other row below the count).  OPDET_STATUS_NO_MODEL when
 *               the view has fewer than min_matches rows or the count is below 3.  OPDET_STATUS_NEEDS_MORE (informational) when the view
 *               ran trials and the host's stop formula asks for more than ran: with w = count / n, 1 trial when w^3 > 1 - 1e-12,
 *               ceil(log(1 - confidence) / log(1 - w^3)) when w^3 > 1e-12, without bound otherwise.
 *   fit         The normal equations over p = [x, y, 1] on the winner's inliers: S_ab = sum p_a p_b, bu_a = sum p_a u, bv_a = sum p_a v.
 *               Order of every sum: thread l of 256 adds the view's rows l, l + 256, ... (view-local numbers, ascending, inliers only) to a
 *               partial that starts at 0, then the 256 partials are added in thread order 0, 1, ..., 255 to a sum that starts at 0.
 *               Singular when |det3(S)| < 1e-12 (det3 and inv3 as in csrc_host/pnp.cpp); affine_r = Si_r0 b_0 + Si_r1 b_1 + Si_r2 b_2 with
 *               b = bu for the first row, bv for the second.  The inlier set is not re-evaluated.
 *   box         The corners (0, 0), (W_v, 0), (0, H_v), (W_v, H_v) of the view through the affine (x' = A0 X + A1 Y + A2, y' = A3 X + A4 Y +
 *               A5, left to right), each coordinate truncated toward zero to int32, then minimum and maximum: [x0, y0, x1, y1].
 *   centre box  [W / 2 - 500, H / 2 - 500, W / 2 + 500, H / 2 + 500] of the query (integer division), with 0 inliers, an empty mask, the
 *               identity affine and OPDET_STATUS_NO_MODEL: a view of fewer than min_matches rows, a best count below 3, a singular system,
 *               a corner that is not finite or truncates outside int32.
 *   vote        winner = the view with the most inliers, the first among equals.  The track state (include/onepose_track.h) of its box:
 *               box, flag = 0, and K_crop / trans by the formula given there for optrk_box_from_pose, bit-equal to optrk_box_set of the
 *               same box.  A winning box with x1 <= x0 or y1 <= y0: the centre box is written to the state (boxes [winner] keeps the view's
 *               own) and OPDET_STATUS_DEGENERATE is set on the winner.
 *
 * Every entry returns 0, or -1 on invalid arguments (checked before any launch), or a positive HIP error code; opdet_last_error() says
 * which.  All pointers are device pointers; scalars are passed by value; `stream` is a hipStream_t.  Everything is enqueued on that
 * stream; nothing allocates or synchronises.  mk0 [cap][2] float32: points in the reference view; mk1 [cap][2] float32: points in the
 * query; b_ids [cap] int64 ascending: the view of every row (a row whose id lies outside [0, V) belongs to no view); `count` (int32[1] on
 * the device) is clamped to `cap`, NULL means all `cap` rows, rows at or beyond it are never read.  Every kernel refuses to index outside
 * its tables whatever `count`, `b_ids` or an intermediate table holds.  The outputs of an entry must not overlap its inputs.
 */
#ifndef ONEPOSE_DETECT_H
#define ONEPOSE_DETECT_H
#include <stddef.h>
#ifdef __cplusplus
extern "C" {
#endif

#define OPDET_ABI_VERSION 1
#define OPDET_MAX_VIEWS 256
#define OPDET_MAX_TRIALS 65536
/* OpenCV's 2000 (the host estimator's default) rounded up to a multiple of the 256 trials a workgroup scores */
#define OPDET_DEFAULT_TRIALS 2048
#define OPDET_MAX_ROWS 16777216
/* the largest query height and width an entry accepts */
#define OPDET_MAX_SIDE 1073741824
/* rows of a view the score kernel stages through LDS at a time (16 bytes each) */
#define OPDET_SCORE_CHUNK 256
/* status bits of a view */
#define OPDET_STATUS_NO_MODEL 1
#define OPDET_STATUS_DEGENERATE 2
#define OPDET_STATUS_NEEDS_MORE 4

int opdet_abi_version(void);
const char* opdet_last_error(void);

/* bytes of the workspace opdet_detect needs; 0 on sizes an entry would refuse */
size_t opdet_workspace_bytes(int cap, int V, int trials);

/* Stage 1: ranges [V][2]. */
int opdet_ranges(const long long* b_ids, const int* count, int cap, int V, int* ranges, void* stream);

/* Stages 2-4 in one kernel: samples [V][trials][3] int32 and cnt [V][trials] int32.  One workgroup of 256 threads per (view, 256 trials). */
int opdet_score(const float* mk0, const float* mk1, const int* ranges, int cap, int V, int trials, int min_matches, double reproj_thr,
                unsigned long long seed, int* samples, int* cnt, void* stream);

/* Stage 5: best [V] int32 (the winning trial, -1: none), n_inliers [V], status [V], inlier_mask [cap].  One workgroup per view.  A sample
 * that does not name three rows of its view gives an empty mask. */
int opdet_select(const float* mk0, const float* mk1, const int* ranges, const int* count, const int* samples, const int* cnt, int cap, int V,
                 int trials, int min_matches, double reproj_thr, double confidence, int* best, int* n_inliers, int* status,
                 unsigned char* inlier_mask, void* stream);

/* Stages 6-7: affine [V][6] float64 and boxes [V][4] int32 from the masked rows; view_hw [V][2] int32 = (H_v, W_v); H, W: the query's.
 * n_inliers, status and inlier_mask are updated where a view votes the centre box.  One workgroup per view. */
int opdet_fit_box(const float* mk0, const float* mk1, const int* ranges, const int* view_hw, int cap, int V, int H, int W, int* n_inliers,
                  int* status, unsigned char* inlier_mask, double* affine, int* boxes, void* stream);

/* Stage 8: winner [1] and the track state; K [9] float64: the full-frame intrinsics, S: the crop size in [1, OPTRK_MAX_CROP].  status
 * [V] gains OPDET_STATUS_DEGENERATE on the winner.  One workgroup. */
int opdet_vote(const int* boxes, const int* n_inliers, int* status, int V, int H, int W, const double* K, int S, int* winner, int* box,
               int* flag, double* K_crop, double* trans, void* stream);

/* All stages on one stream.  The workspace starts with the ranges table. */
int opdet_detect(const float* mk0, const float* mk1, const long long* b_ids, const int* count, int cap, int V, const int* view_hw, int H, int W,
                 const double* K, int S, int min_matches, double reproj_thr, double confidence, int trials, unsigned long long seed,
                 void* workspace, size_t workspace_bytes, int* boxes, int* n_inliers, double* affine, int* status, unsigned char* inlier_mask,
                 int* winner, int* box, int* flag, double* K_crop, double* trans, void* stream);

#ifdef __cplusplus
}
#endif
#endif
