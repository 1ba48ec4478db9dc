/* libonepose_pose_eval.so -- pose evaluation on the device (gfx950): the cm-degree errors, ADD, ADD-S and the 2D projection error of a
 * whole sequence of poses against their ground truth.  C ABI; its own library (a row of
 * cabi.LIBRARIES: DESIGN.md section 1b).
 *
 * This header is the specification; tests/pose_eval_oracle.py restates it in numpy, one function per stage.  All arithmetic is float64,
 * every expression evaluated in the written order with contraction off; the operations are + - * /, sqrt and comparisons, so the device
 * equals numpy bit for bit.  The arc cosine is NOT taken here: the host computes rad2deg(arccos(rot_cos)) on the F scalars it reads back.
 *
 * Every entry returns 0, or -1 on invalid arguments (checked before any launch), or a positive HIP error code; opevl_last_error() says
 * which.  Pointers are device pointers; `stream` is a hipStream_t; nothing is synchronised and nothing is read on the host.
 *
 * A pose table is `frames` row-major matrices [R | t], `stride` doubles apart: 12 ([F][3][4]) or 16 ([F][4][4], the fourth row is never
 * read).  A model is verts [V][3] float32, widened to float64.  A model vertex x under a pose:
 *     X'_k = ((R[k][0] * x0 + R[k][1] * x1) + R[k][2] * x2) + t_k.
 */
#ifndef ONEPOSE_POSE_EVAL_H
#define ONEPOSE_POSE_EVAL_H
#ifdef __cplusplus
extern "C" {
#endif

#define OPEVL_ABI_VERSION 1
#define OPEVL_MAX_FRAMES 1048576
#define OPEVL_MAX_VERTICES 262144
/* the summation block and the LDS tile of the nearest-neighbour search */
#define OPEVL_BLOCK 256
/* the most vertex pairs one opevl_adds launch evaluates (DESIGN.md section 6p says where the figure comes from) */
#define OPEVL_MAX_PAIRS_PER_LAUNCH 4294967296
/* flags [F]: a frame with either bit has rot_cos = NaN and every other output +inf */
#define OPEVL_NO_POSE 1
#define OPEVL_BAD_INPUT 2

int opevl_abi_version(void);
const char* opevl_last_error(void);

/* 1. One lane per frame.  flags[f] = OPEVL_NO_POSE when status is not NULL and status[f] & status_mask, | OPEVL_BAD_INPUT when one of the
 * 12 entries of either pose is not finite.  A frame with flags 0:
 *     trace = sum_i sum_j Rp[i][j] * Rg[i][j]     (i outer, j inner, accumulated left to right from 0.0)
 *     rot_cos = ((trace <= 3 ? trace : 3) - 1) / 2          (the upper clamp only; below -1 the host's arc cosine gives NaN)
 *     t_err = unit_scale * sqrt((dx * dx + dy * dy) + dz * dz),   d = tp - tg
 * unit_scale: finite and > 0 (100 for poses in metres, 1 for centimetres, 0.1 for millimetres: t_err is in centimetres). */
int opevl_errors(const double* pose_pred, int pred_stride, const double* pose_gt, int gt_stride, const int* status, int status_mask,
                 int frames, double unit_scale, double* rot_cos, double* t_err, int* flags, void* stream);

/* Every mean below is summed in one fixed order: blocks of OPEVL_BLOCK consecutive vertices; in a block lane l holds term l (0 beyond the
 * last vertex); for stride = 128, 64, .., 1: s[l] += s[l + stride] for l < stride; s[0] is the block's partial.  partials is
 * [frames][ceil(V / OPEVL_BLOCK)] doubles of workspace; a finish launch adds a frame's partials in ascending block order from 0.0 and
 * divides by V.  flags [F] as opevl_errors left them (NULL: every frame is evaluated): a flagged frame's result is +inf and none of its
 * partials is written.
 *
 * 2. add_dist[f] = mean over v of sqrt((dx * dx + dy * dy) + dz * dz), d = X'(pose_pred) - X'(pose_gt).  Grid (blocks, frames). */
int opevl_add(const float* verts, int V, const double* pose_pred, int pred_stride, const double* pose_gt, int gt_stride, const int* flags,
              int frames, double* partials, double* add_dist, void* stream);

/* 3. The symmetric form, exact: adds_dist[f] = mean over the TARGET vertices j (under pose_gt) of sqrt(m_j), m_j the minimum over ALL
 * predicted vertices i (under pose_pred, ascending i) of d2 = (dx * dx + dy * dy) + dz * dz, d = X'_i(pose_pred) - X'_j(pose_gt), taken
 * as m = +inf; if (d2 < m) m = d2.  Each lane keeps its target in registers; the predicted vertices go through LDS in tiles of OPEVL_BLOCK,
 * the last tile masked by index.  The launches are chunked so that none evaluates more than pair_budget pairs (0: OPEVL_MAX_PAIRS_PER_LAUNCH):
 * whole frames, V * V pairs each, while one frame fits; else the blocks of one frame, OPEVL_BLOCK * V pairs each.  pair_budget outside
 * [min(V, OPEVL_BLOCK) * V, OPEVL_MAX_PAIRS_PER_LAUNCH] is rejected.  The chunking changes no result. */
int opevl_adds(const float* verts, int V, const double* pose_pred, int pred_stride, const double* pose_gt, int gt_stride, const int* flags,
               int frames, long long pair_budget, double* partials, double* adds_dist, void* stream);

/* 4. With K [3][3] (k_shared != 0) or [F][3][3]: u_k = ((K[k][0] * X'_0 + K[k][1] * X'_1) + K[k][2] * X'_2), xy = (u_0 / u_2, u_1 / u_2)
 * under both poses; proj2d[f] = mean over v of sqrt(dx * dx + dy * dy), d = xy(pose_pred) - xy(pose_gt). */
int opevl_proj2d(const float* verts, int V, const double* pose_pred, int pred_stride, const double* pose_gt, int gt_stride, const double* K,
                 int k_shared, const int* flags, int frames, double* partials, double* proj2d, void* stream);

#ifdef __cplusplus
}
#endif
#endif
