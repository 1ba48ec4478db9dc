/* libonepose_postopt_lm.so -- the second-order (Levenberg-Marquardt) solver of the keypoint-free SfM depth refinement, on the device
 * (gfx950).  C ABI; its own library (a row of cabi.LIBRARIES: DESIGN.md section 1b), so that libonepose_hip.so keeps its
 * symbol set.
 *
 * The problem is the one ophip_postopt_refine (onepose_hip.h) solves with Adam: every residual row folds to h(d) = d * a + b, every
 * track owns one depth, so the normal equations are diagonal and a Levenberg-Marquardt solve is P independent scalar problems.  One
 * launch runs every iteration of every track (one wave per track); a second, one-workgroup launch sums the per-track costs in index
 * order.  The algorithm is written out in DESIGN.md section 6e and restated in tests/postopt_lm_oracle.py.
 *
 * Every entry returns 0, or -1 on invalid arguments, or a positive HIP error code; oplm_last_error() says which.  All pointers are
 * device pointers; `stream` is a hipStream_t.
 */
#ifndef ONEPOSE_POSTOPT_LM_H
#define ONEPOSE_POSTOPT_LM_H
#include <stddef.h>
#ifdef __cplusplus
extern "C" {
#endif

#define OPLM_ABI_VERSION 1
/* status [P]: the step fell below step_tol; max_iters evaluations were spent; lambda passed lam_max; the start has a non-finite cost or
 * no curvature (H > 0 fails) and the depth is left as it came */
#define OPLM_CONVERGED 0
#define OPLM_MAX_ITERS 1
#define OPLM_STALLED 2
#define OPLM_DEGENERATE 3

int oplm_abi_version(void);
const char* oplm_last_error(void);

/* bytes of the workspace of oplm_refine for L rows in P tracks (the folded rows of tracks longer than one wave); 0 on bad sizes */
size_t oplm_workspace_bytes(long long L, int P);

/* In:  depth [P] start; track_offsets [P + 1] first row of every track (rows track after track, track_offsets[P] = L);
 *      intrinsic0 / intrinsic1 [L][3][3], mkpts0_c / mkpts1_f [L][2], left_idx / right_idx [L] into angle_axis [F][6];
 *      lam0, up, down, lam_min, lam_max, step_tol, max_iters: the damping schedule, the step tolerance and the evaluation budget.
 * Out: depth [P]; iterations / rejects / status [P] int; lambda / initial_cost / final_cost [P];
 *      initial_residual / final_residual [1]: the per-track costs summed in a fixed order; residuals [L][2] at the returned depths,
 *      or NULL.  workspace: 256-byte aligned, oplm_workspace_bytes(L, P) bytes. */
int oplm_refine(double* depth, const long long* track_offsets, int P, long long L, const double* intrinsic0, const double* intrinsic1,
                const double* mkpts0_c, const double* mkpts1_f, const long long* left_idx, const long long* right_idx,
                const double* angle_axis, int F, double lam0, double up, double down, double lam_min, double lam_max, double step_tol,
                int max_iters, int* iterations, int* rejects, int* status, double* lambda, double* initial_cost, double* final_cost,
                double* initial_residual, double* final_residual, double* residuals, void* workspace, size_t workspace_bytes,
                void* stream);

#ifdef __cplusplus
}
#endif
#endif
