/* libonepose_train_forward.so -- the one step in which the training-mode forward differs from the eval forward, on the device (gfx950): the
 * coarse match list cut to a random part of the predicted matches and padded with random ground-truth matches of confidence 0 (the
 * reference's CoarseMatching.get_coarse_match, coarse_matching.py:174-240), from the SPARSE ground truth gt_j [B][N] of
 * onepose_supervision.h instead of a dense conf_matrix_gt [B][N][M].  C ABI; its own library (the row of
 * cabi.TRAINING: DESIGN.md section 1b).
 *
 * This header is the specification; tests/train_forward_oracle.py restates it in numpy, one function per entry, sampler included.  Every
 * expression is evaluated in the written order with contraction off; integers are exact; the two float32 products of entry 2 are float32.
 *
 * Every entry returns 0, or -1 on invalid arguments (checked before any launch), or a positive HIP error code; optrn_last_error() says
 * which.  Pointers are device pointers; `stream` is a hipStream_t; nothing is synchronised and no count is read on the host: a count is a
 * device int.  No workgroup waits for another; there are no atomics of any kind, so two runs give identical bytes.
 *
 * The padded list always has exactly T rows (T = int(B * min(N, M) * train_coarse_percent), a host constant): with P predicted rows and
 * G = train_pad_num_gt_min, P <= T - G keeps all P rows and pads T - P; otherwise T - G rows are picked and G are padded.  So the capacity
 * of every buffer behind this step is T, and the split n_keep = min(P, T - G) is one device int.
 */
#ifndef ONEPOSE_TRAIN_FORWARD_H
#define ONEPOSE_TRAIN_FORWARD_H
#include <stddef.h>
#ifdef __cplusplus
extern "C" {
#endif

#define OPTRN_ABI_VERSION 1
/* the workgroup of entry 1: OPTRN_BLOCK consecutive rows r per workgroup */
#define OPTRN_BLOCK 256
#define OPTRN_MAX_BATCH 65535
/* B * N, N, M and the capacity of a predicted list: at most this */
#define OPTRN_MAX_ROWS 16777216
/* step: below this */
#define OPTRN_MAX_STEP 1073741824
/* status of optrn_pad_matches */
#define OPTRN_OK 0
#define OPTRN_NO_GT 1

int optrn_abi_version(void);
const char* optrn_last_error(void);

/* 1. The reference's torch.where(conf_matrix_gt), in its order.  Row r = b * N + i (r < B * N <= OPTRN_MAX_ROWS) is a ground-truth row iff
 * 0 <= gt_j[b][i] < M.  gt_rows[k] is the k-th such r in ascending order -- ascending (b, i, j), since a point has at most one cell --
 * for k < n_gt_total[0], the number of such rows; gt_rows [B * N] int32, the entries at or past n_gt_total are not written.
 * An exclusive prefix sum over the B * N flags: (a) one workgroup per OPTRN_BLOCK rows counts its flags into workspace[block];
 * (b) ONE workgroup turns the block counts into their exclusive prefix sum in place, OPTRN_BLOCK counts at a time with a running carry (it
 * loops when there are more than OPTRN_BLOCK blocks), and writes n_gt_total; (c) the workgroups of (a) scan their own flags and scatter.
 * workspace: optrn_gt_list_bytes(B, N) bytes (one int per workgroup of (a), rounded up to 256 bytes).  Three launches. */
size_t optrn_gt_list_bytes(int B, int N);
int optrn_gt_list(const long long* gt_j, int B, int N, int M, void* workspace, size_t workspace_bytes, int* gt_rows, int* n_gt_total,
                  void* stream);

/* 2. The T rows of the training list, one thread per output row.  The predicted list (the eval forward's): b_ids, i_ids, j_ids [cap]
 * int64, mconf [cap], mkpts_3d [cap][3], mkpts_c [cap][2] float32 with the device count `count` (NULL: cap); P = count clamped into
 * [0, cap].  gt_rows / n_gt_total: entry 1's (n_gt_total clamped into [0, B * N]); keypoints3d [N][3] float32 per frame, kp_bstride floats
 * apart (0: one object for every frame).  n_keep = min(P, T - G).
 *
 * The sampler: h(c, s) = mix(seed + 0x9E3779B97F4A7C15 * ((((step * 2 + c) << 32) | s) + 1)), arithmetic modulo 2^64, mix the splitmix64
 * finaliser of onepose_pnp_device.h and onepose_detect.h; step < OPTRN_MAX_STEP is the caller's call counter, c = 0 for the predicted
 * picks and 1 for the ground-truth picks.  Picks are with replacement, as torch.randint's are.  A pick is h % n: the modulo bias of a
 * 64-bit draw is below n / 2^64 < 2^-40 at n <= OPTRN_MAX_ROWS and is ignored.  The draws are this project's own specification: they
 * cannot equal torch.randint's stream.  Everything else is the reference's.
 *
 * Row s < n_keep: the source is predicted row s when P <= T - G, else predicted row h(0, s) % P; b, i, j, mconf, mkpts_3d and mkpts_c are
 * copied from that row.
 * Row s >= n_keep, u = s - n_keep: r = gt_rows[h(1, u) % n_gt_total] (forced into [0, B * N): entry 1 writes nothing else);
 *     b = r / N, i = r % N, j = gt_j[b][i], mconf = 0,
 *     mkpts_3d = keypoints3d[b][i]
 *     mkpts_c  = (float)(j % w_c) * sx, (float)(j / w_c) * sy      sx = sy = scale with query_scale == NULL, else (query_scale [B][2])
 *                                                                  sx = scale * query_scale[b][1], sy = scale * query_scale[b][0]
 * Both kinds: gt_mask[s] = (mconf == 0).  Also written, by the thread of row 0: out_count[0] = T, n_keep[0], status[0] = OPTRN_OK.
 * n_gt_total == 0: status[0] = OPTRN_NO_GT, out_count[0] = 0, n_keep[0] as above, and NO row is written (the reference asserts there).
 * The outputs hold at least T rows; rows at or past T are never written.
 * -1 unless 0 < G < T (the reference's assert), T <= B * N, 1 <= B <= OPTRN_MAX_BATCH, 1 <= N, M, cap <= OPTRN_MAX_ROWS,
 * B * N <= OPTRN_MAX_ROWS, w_c >= 1, 0 <= step < OPTRN_MAX_STEP, kp_bstride == 0 or >= 3 * N.  One launch. */
int optrn_pad_matches(const long long* b_ids, const long long* i_ids, const long long* j_ids, const float* mconf, const float* mkpts_3d,
                      const float* mkpts_c, const int* count, int cap, const int* gt_rows, const int* n_gt_total, const long long* gt_j,
                      const float* keypoints3d, long long kp_bstride, int B, int N, int M, int w_c, int T, int G,
                      unsigned long long seed, int step, float scale, const float* query_scale, long long* out_b_ids,
                      long long* out_i_ids, long long* out_j_ids, float* out_mconf, float* out_mkpts_3d, float* out_mkpts_c,
                      unsigned char* out_gt_mask, int* out_count, int* n_keep, int* status, void* stream);

#ifdef __cplusplus
}
#endif
#endif
