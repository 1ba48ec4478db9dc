/* libonepose_loss_backward.so -- the backward of the training loss on the device (gfx950), down to the matcher's feature boundaries: the
 * gradient of the focal loss through the N x M dual softmax into the two coarse feature tables, and the gradient of the std-weighted L2
 * fine loss through the window softmax into the fine features.  C ABI; its own library (the row of cabi.BACKWARD:
 * DESIGN.md section 1b).
 *
 * This header is the specification; tests/loss_backward_oracle.py restates it in numpy float64, one function per entry.  The forward it
 * differentiates is onepose_supervision.h's (opsup_coarse_loss over the dual-softmax conf_matrix, opsup_fine_loss); the backward of the
 * transformers, of the window gather and of the backbone are not here: they consume the four tensors these entries write.
 *
 * Every entry returns 0, or -1 on invalid arguments (checked before any launch), or a positive HIP error code; opbwd_last_error() says
 * which.  Pointers are device pointers; `stream` is a hipStream_t; nothing is synchronised and nothing is read on the host.  A count is a
 * device int clamped into [0, capacity]; rows at or past it are never read and their outputs never written.  No workgroup waits for
 * another; there are no float atomics and no sum whose order depends on the schedule: every sum is taken by one lane, one wave or one
 * workgroup in a fixed order, so two runs give identical bytes.
 */
#ifndef ONEPOSE_LOSS_BACKWARD_H
#define ONEPOSE_LOSS_BACKWARD_H
#include <stddef.h>
#ifdef __cplusplus
extern "C" {
#endif

#define OPBWD_ABI_VERSION 1
/* the workgroup of the fine entry's sums over rows: opsup_fine_loss's (OPSUP_BLOCK): thread k takes the rows k, k + 256, ... in ascending
 * order from 0.0, then the tree s[k] = s[k] + s[k + stride], stride = 128 .. 1 */
#define OPBWD_BLOCK 256
/* the coarse kernel: a workgroup OWNS OPBWD_OWNED_ROWS rows of one side (four waves of 32) and sweeps the other side in tiles of
 * OPBWD_SWEPT_ROWS rows */
#define OPBWD_OWNED_ROWS 128
#define OPBWD_SWEPT_ROWS 32
#define OPBWD_CHANNELS 256
#define OPBWD_FINE_CHANNELS 128
#define OPBWD_MAX_BATCH 65535
#define OPBWD_MAX_ROWS 1048576
/* status of opbwd_fine_grads: opsup_fine_loss's values */
#define OPBWD_OK 0
#define OPBWD_NONE 1
#define OPBWD_FORCED 2
#define OPBWD_EMPTY 3

int opbwd_abi_version(void);
const char* opbwd_last_error(void);

/* 1. The coarse gradient.  feat0 [B][N][256] and feat1 [B][M][256] float32, contiguous: the coarse transformer's outputs.  gt_j [B][N]
 * (the cell of a 3D point, outside [0, M): none) and gt_i [B][M] (the point of a cell, outside [0, N): none): GroundTruth's two tables, each
 * the inverse of the other.  The specification is float64:
 *     a_i = feat0[b][i] / 16, b_j = feat1[b][j] / 16          (1 / sqrt(256): an exact power of two)
 *     t = (float)(temperature + 1e-4)                         (the forward's temperature argument, as it is formed there)
 *     S_ij = (a_i . b_j) / t;   lr_i = logsumexp_j S_ij;   lc_j = logsumexp_i S_ij
 *     Pr_ij = exp(S_ij - lr_i);   Pc_ij = exp(S_ij - lc_j);   conf_ij = Pc_ij * Pr_ij
 * the derivative of opsup_coarse_loss with respect to conf:
 *     c = conf < 1e-6 ? 1e-6 : (conf > 1 - 1e-6 ? 1 - 1e-6 : conf);   inside = 1e-6 <= conf && conf <= 1 - 1e-6    (torch.clamp's backward)
 *     positive (gt_j[b][i] == j):  g = wpos * (alpha * gamma * Q(1 - c) * log(c) - alpha * P(1 - c) / c)
 *     every other element:         g = wneg * (-(1 - alpha) * (gamma * Q(c) * log(1 - c) - P(c) / (1 - c)))
 *     g = 0 where inside is false
 *     P(v) = v * v and Q(v) = v when gamma == 2, else P(v) = pow(v, gamma) and Q(v) = pow(v, gamma - 1)      (opsup_coarse_loss's rule)
 *     n_pos = the rows of the WHOLE BATCH with 0 <= gt_j < M, n_neg = B * N * M - n_pos           (counted on the device, as entry 3 of
 *     wpos = n_pos > 0 ? pos_weight / n_pos : 0;   wneg = n_neg > 0 ? neg_weight / n_neg : 0       onepose_supervision.h counts them)
 * A quirk of the reference, kept: a positive whose confidence is still below 1e-6 -- at the start of training, most of them -- gets NO
 * direct gradient, because the clamp's backward is zero outside its bounds.  Through the dual softmax (`scale`: coarse_weight times the
 * caller's upstream factor):
 *     u_ij = scale * conf_ij * g_ij;   r_i = sum_j u_ij;   c_j = sum_i u_ij
 *     dS_ij = 2 * u_ij - Pr_ij * r_i - Pc_ij * c_j
 *     grad0[b][i] = (1 / (16 t)) * sum_j dS_ij * b_j;   grad1[b][j] = (1 / (16 t)) * sum_i dS_ij * a_i
 * dS is dense although g is zero on most elements.  grad0 [B][N][256], grad1 [B][M][256] float32, contiguous, every row written.
 *
 * The device works in float32 around split-bf16 matrix products (x = hi + lo, hi = bf16(x), lo = bf16(x - hi); a . b taken as
 * a_hi . b_hi + a_hi . b_lo + a_lo . b_hi on v_mfma_f32_32x32x16_bf16, f32 accumulate).  The operand points are feat / 16 (for S and as the
 * swept operand of the gradient products) and dS.  For S the three sums over the channels are kept apart and joined as
 * (a_lo . b_hi + a_hi . b_lo) + a_hi . b_hi, so that S_ij has the same bits whichever side owns it and S_ij - lr_i, S_ij - lc_j cancel in
 * every pass as they did where lr and lc were formed.  Nothing N x M is stored or read; S is recomputed in every pass.  Launches:
 *     count      one workgroup of 256: n_pos by an integer tree; wpos * scale and wneg * scale (float64, rounded once to float32)
 *     planes     both sides to (hi, lo) bf16 planes of feat / 16 in two layouts, rows zero-padded to a multiple of 32: the S layout is the
 *                forward's (frag_planes_kernel: for 32-row tile T and k-step s the 1 KiB block ((T * 16 + s) * 2 + plane) holds lane l's
 *                8 values, row 32 T + (l & 31), channels 16 s + 8 (l >> 5) ..); the transposed layout feeds the gradient product: block
 *                (((T * 2 + s) * 8 + ct) * 2 + plane) holds for lane l channel 32 ct + (l & 31), element e: row
 *                32 T + 16 s + 8 (e >> 2) + 4 (l >> 5) + (e & 3), the order in which an accumulator's registers are the next operand
 *     sweep x 3  ONE kernel in two roles per launch (grid x: the blocks that own rows of feat0, then those that own rows of feat1; y: b).
 *                A wave owns 32 rows and keeps their S-layout fragments in registers; the workgroup streams the other side's tiles of
 *                OPBWD_SWEPT_ROWS rows through two LDS buffers.  Per tile the wave computes the TRANSPOSED tile S^T[swept][owned] (16
 *                k-steps), so a lane holds one owned row and 16 swept rows (rows (reg & 3) + 8 (reg >> 2) + 4 (lane >> 5)).
 *         pass 1 lr (rows of feat0) and lc (rows of feat1): per lane an online (max, sum exp) over the tiles in ascending order, registers
 *                in ascending order inside a tile; the two lanes of an owned row are combined as (lane < 32) op (lane + 32); m + log(sum)
 *         pass 2 r and c: u from lr, lc and the ground truth; per lane the float32 sum in the same order, the two lanes combined alike
 *         pass 3 dS in registers, split, and as the A operand of the second product against the swept side's transposed planes into eight
 *                32 x 32 accumulators (the wave's 32 rows x 256 channels), in ascending tile order; times 1 / (16 t); stored
 * Both roles find the positive from gt_j alone (the feat1-owning role reads the swept rows' gt_j); gt_i is accepted for callers that hold
 * both tables and is not read.
 * workspace: opbwd_coarse_workspace_bytes(B, N, M) bytes, 256-byte aligned: the planes (2 KiB per padded row) and 12 bytes of statistics per
 * padded row; O(B * (N + M)). */
size_t opbwd_coarse_workspace_bytes(int B, int N, int M);
int opbwd_coarse_grads(const float* feat0, const float* feat1, const long long* gt_j, const long long* gt_i, int B, int N, int M,
                       double temperature, double alpha, double gamma, double pos_weight, double neg_weight, double scale, void* workspace,
                       size_t workspace_bytes, float* grad0, float* grad1, void* stream);

/* 2. The fine gradient.  feat_f0 [cap][128] and feat_f1 [cap][W * W][128] float32: the fine transformer's outputs (the centre feature of
 * the 3D point and the window of the query image); expec_f [cap][3] and expec_f_gt [cap][2] as opsup_fine_loss takes them; the device
 * count n (NULL: cap); W odd, 3 <= W <= 11.  float64 from the float32 values; one workgroup of OPBWD_BLOCK threads per four rows, one wave
 * per row.  The bookkeeping is opsup_fine_loss's, recomputed by every workgroup in that entry's order:
 *     inv_k = 1 / (std_k < 1e-10 ? 1e-10 : std_k), std_k = expec_f[k][2];   mean_inv = (sum inv_k) / n;   w_k = inv_k / mean_inv
 *     correct_k = max(|gt_x|, |gt_y|) < correct_thr (false for NaN), gt = expec_f_gt[k];   n_correct: their number
 *     status: OPBWD_OK (n_correct > 0); OPBWD_NONE (none, training == 0); OPBWD_FORCED (none, training, n > 0: row 0 ALONE counts, with
 *     w_0 = 1e-6 and n_correct = 1); OPBWD_EMPTY (none, training, n == 0).  The weight is detached: nothing flows through std.
 * Row k < n that counts (lane l of the wave holds window rows l and l + 64; sum_lanes(x): x += x of lane ^ 32, 16, .. 1; max alike):
 *     sim_r = sum_c f0[c] * f1[r][c], c ascending from 0.0;   x_r = sim_r * (1 / sqrt(128.0))
 *     m = max_r x_r;   e_r = exp(x_r - m);   Z = sum_lanes(e_l + e_(l + 64));   p_r = e_r / Z                  (rows past W * W: 0)
 *     grid_r = (-1 + 2 * (r mod W) / (W - 1), -1 + 2 * (r div W) / (W - 1))
 *     co = sum_lanes(p_l * grid_l + p_(l + 64) * grid_(l + 64))                                                    (per axis)
 *     dco = ((scale * -2) * (gt - co)) * w_k / n_correct                                                          (per axis)
 *     ds_r = p_r * ((grid_r.x * dco.x + grid_r.y * dco.y) - (co.x * dco.x + co.y * dco.y))
 *     grad_f0[k][c] = (1 / sqrt(128.0)) * sum_r ds_r * f1[r][c], r ascending from 0.0;   grad_f1[k][r][c] = ((1 / sqrt(128.0)) * ds_r) * f0[c]
 * rounded once to float32.  Every other row k < n is written with zeros; so is every written row with OPBWD_NONE or OPBWD_EMPTY.
 * n_correct and status: device ints, written by the first workgroup.  One launch. */
int opbwd_fine_grads(const float* feat_f0, const float* feat_f1, const float* expec_f, const float* expec_f_gt, const int* count, int cap,
                     int W, double correct_thr, int training, double scale, float* grad_f0, float* grad_f1, int* n_correct, int* status,
                     void* stream);

#ifdef __cplusplus
}
#endif
#endif
