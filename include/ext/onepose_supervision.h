/* libonepose_supervision.so -- the supervised signals of training and validation on the device (gfx950), forward only: the sparse
 * ground-truth assignment of a labelled frame, the fine-level targets of the coarse matches, the focal loss over conf_matrix and the
 * std-weighted L2 fine loss.  C ABI; its own library (the row of cabi.ADDONS: DESIGN.md section 1b).
 *
 * This header is the specification; tests/supervision_oracle.py restates it in numpy, one function per entry.  float32 steps are float32
 * and float64 steps float64, every expression evaluated in the written order with contraction off.  Entries 1 and 2 use + - * /, rint and
 * comparisons only, so the device equals numpy bit for bit; entries 3 and 4 also call the float64 log and pow of the device's math library.
 *
 * Every entry returns 0, or -1 on invalid arguments (checked before any launch), or a positive HIP error code; opsup_last_error() says
 * which.  Pointers are device pointers; `stream` is a hipStream_t; nothing is synchronised and no count is read on the host.  A count is a
 * device int clamped into [0, capacity]; rows at or past it are never read and their outputs never written.  No workgroup waits for
 * another; there are no float atomics; the integer atomics (a minimum and a counter) give results that do not depend on their order, so
 * two runs give identical bytes.
 */
#ifndef ONEPOSE_SUPERVISION_H
#define ONEPOSE_SUPERVISION_H
#ifdef __cplusplus
extern "C" {
#endif

#define OPSUP_ABI_VERSION 1
/* the workgroup of every sum: thread k of OPSUP_BLOCK takes the elements k, k + OPSUP_BLOCK, ... in ascending order, from 0.0; then the
 * tree s[k] = s[k] + s[k + stride] for k < stride, stride = 128, 64, .. 1 */
#define OPSUP_BLOCK 256
#define OPSUP_MAX_BATCH 65535
#define OPSUP_MAX_ROWS 16777216
/* status of opsup_fine_loss */
#define OPSUP_OK 0
#define OPSUP_NONE 1
#define OPSUP_FORCED 2
#define OPSUP_EMPTY 3

int opsup_abi_version(void);
const char* opsup_last_error(void);

/* 1. The sparse ground truth of B frames (the reference's read_anno, train split, and build_assignmatrix, at query_image_scale 1).
 * keypoints3d [N][3] float32 per frame, kp_bstride floats apart (0: one object for every frame); point_ids [B][A]: the 3D index of every
 * annotated 2D keypoint in annotation order; counts [B] (NULL: A rows each); pose_gt [B][4][4] and K ([3][3] with k_shared != 0, else
 * [B][3][3]) float32; the image is H x W, the coarse grid w_c = W / stride wide and M = (H / stride) * w_c cells (integer divisions).
 * Row r < counts[b] of frame b, everything float32:
 *     i = point_ids[b][r]; dropped unless 0 <= i < N         (the reference's gather would raise)
 *     Xc_k = ((R[k][0] * X + R[k][1] * Y) + R[k][2] * Z) + t_k;    q_k = (K[k][0] * Xc_0 + K[k][1] * Xc_1) + K[k][2] * Xc_2
 *     p = (q_0 / (q_2 + 1e-6f), q_1 / (q_2 + 1e-6f))           NO depth test: a point behind the camera that lands inside is ground truth
 *     pr = rint(p / stride) * stride                           (half to even)
 *     dropped unless pr_x >= 0 && pr_x <= W - 1 && pr_y >= 0 && pr_y <= H - 1      (so a NaN is dropped: the reference's index is undefined)
 *     j = (long long)((pr_y / stride) * w_c + pr_x / stride); dropped when j >= M      (the reference tests j > M and would fault at
 *                                                                j == M; neither happens when H and W are multiples of stride)
 * Of the surviving rows of one cell j the FIRST in annotation order stays: owner [B][M] int32 workspace takes the minimum r (an integer
 * atomic), a second launch keeps row r iff owner[b][j] == r.  Two rows with one i project alike, so a point keeps at most one cell.
 * gt_j [B][N] (-1: none), gt_xy [B][N][2] = p ((-50, -50): none), gt_i [B][M] (-1: none), n_gt [B]: the kept rows.  Three launches. */
int opsup_ground_truth(const float* keypoints3d, long long kp_bstride, const long long* point_ids, const int* counts, const float* pose_gt,
                       const float* K, int k_shared, int B, int N, int A, int H, int W, int stride, int* owner, long long* gt_j,
                       float* gt_xy, long long* gt_i, int* n_gt, void* stream);

/* 2. The fine-level target of every coarse match (the reference's fine_supervision).  b_ids, i_ids, j_ids [cap] with the device count
 * (NULL: cap).  Row k < count, float32:
 *     loc = (0 <= b < B && 0 <= i < N && gt_j[b][i] == j) ? gt_xy[b][i] : (-50, -50)
 *     scale == NULL:  cs = fs = (float)fine_res       (the reference's line 18 ends in `else fine_scale`: its coarse scale without an image
 *                                                     scale IS the fine one, a bug kept literally; coarse_res is then unused)
 *                     g = (float)((j mod w_c) * fine_res), (float)((j div w_c) * fine_res)          (integers; floor division)
 *     scale [B][2]:   cs = coarse_res * scale[b][1 - a], fs = fine_res * scale[b][1 - a] for axis a = 0 (x), 1 (y)
 *                     g = (float)(j mod w_c) * cs_x, (float)(j div w_c) * cs_y                        (b outside [0, B): scale 1)
 *     expec_f_gt[k][a] = ((loc_a - g_a) / fs_a) / (float)radius */
int opsup_fine_targets(const long long* b_ids, const long long* i_ids, const long long* j_ids, const int* count, int cap,
                       const long long* gt_j, const float* gt_xy, int B, int N, int w_c, int coarse_res, int fine_res, int radius,
                       const float* scale, float* expec_f_gt, void* stream);

/* 3. The focal loss over conf [B][N][M] float32 (batches conf_bstride, rows conf_rstride floats apart, elements contiguous) with gt_j
 * [B][N].  Element (b, i, j), x = (double)conf, float64:
 *     c = x < 1e-6 ? 1e-6 : (x > 1 - 1e-6 ? 1 - 1e-6 : x)              (NaN stays NaN)
 *     positive (gt_j[b][i] == j):  term = ((-alpha) * P(1 - c)) * log(c)
 *     every other element:         term = ((-(1 - alpha)) * P(c)) * log(1 - c)
 *     P(v) = v * v when gamma == 2, else pow(v, gamma)
 * One workgroup per row sums its negatives in the order of OPSUP_BLOCK; the row's positive term (at most one) needs no sum.  partials
 * [B * N + 1][2] doubles of workspace: row (b, i) at b * N + i holds (positive term or 0.0, negative sum); the last pair is written first,
 * by one lane: the negative term at c = 1e-6, which the rows add for every x <= 1e-6 instead of evaluating it -- the same value, so the
 * sum is the specified one.  A last launch of one workgroup sums the rows' pairs in the order of OPSUP_BLOCK over b * N + i and writes
 *     sums[0] = pos_sum, sums[1] = neg_sum, counts[0] = n_pos (rows with 0 <= gt_j < M), counts[1] = n_neg = B * N * M - n_pos,
 *     sums[2] = loss_c = n_pos == 0 ? neg_weight * (neg_sum / n_neg) : n_neg == 0 ? pos_weight * (pos_sum / n_pos)
 *                                   : pos_weight * (pos_sum / n_pos) + neg_weight * (neg_sum / n_neg)
 * the means of the reference: over the whole batch flattened.  Three launches. */
int opsup_coarse_loss(const float* conf, long long conf_bstride, long long conf_rstride, const long long* gt_j, int B, int N, int M,
                      double alpha, double gamma, double pos_weight, double neg_weight, double* partials, double* sums,
                      long long* counts, void* stream);

/* 4. The std-weighted L2 fine loss over expec_f [cap][3] (x, y, std) and expec_f_gt [cap][2] float32 with the device count n (NULL: cap);
 * one workgroup, float64 from the float32 values, every sum in the order of OPSUP_BLOCK over the rows k < n:
 *     inv_k = 1 / (std_k < 1e-10 ? 1e-10 : std_k)  (NaN stays);   mean_inv = (sum inv_k) / n;   w_k = inv_k / mean_inv
 *     correct_k = max(|gt_x|, |gt_y|) < correct_thr               (false for NaN)
 *     d_k = (dx * dx + dy * dy) * w_k, d = expec_f_gt[k] - expec_f[k][:2]
 *     n_correct > 0:                       loss_f = (sum over correct of d_k) / n_correct, status OPSUP_OK
 *     n_correct == 0, training == 0:       loss_f = NaN, status OPSUP_NONE
 *     n_correct == 0, training, n > 0:     loss_f = (dx * dx + dy * dy of row 0) * 1e-6, n_correct = 1, status OPSUP_FORCED
 *     n_correct == 0, training, n == 0:    loss_f = NaN, status OPSUP_EMPTY     (the reference indexes row 0 of nothing and raises) */
int opsup_fine_loss(const float* expec_f, const float* expec_f_gt, const int* count, int cap, double correct_thr, int training,
                    double* loss_f, int* n_correct, int* status, void* stream);

#ifdef __cplusplus
}
#endif
#endif
