/* libonepose_sfm.so -- the keypoint-free SfM's last two steps on the device (gfx950): feature aggregation over tracks, point
 * selection (box, track length, merge of close points) and the per-point descriptor mean.  C ABI; its own library, so that
 * libonepose_hip.so (the frame path) is built from exactly the sources it was built from before.
 *
 * The reference: src/KeypointFreeSfM/post_optimization/feature_aggregation.py:10-180 and run.py:295-390 (filter_points.py,
 * filter_tkl.py, feature_process.py).  The contract of every stage is in onepose_st_amd/sfm_objectblock.py and DESIGN.md section 6h.
 *
 * Every entry returns 0, or -1 on invalid arguments, or a positive HIP error code; opsfm_last_error() says which.  All pointers are
 * device pointers unless said otherwise; `stream` is a hipStream_t; the workspace is caller-allocated, 256-byte aligned, at least
 * opsfm_workspace_bytes(n_slots, n_points) bytes.  Index tables are validated by the caller before any launch; the kernels also
 * refuse to write outside their outputs.
 */
#ifndef ONEPOSE_SFM_H
#define ONEPOSE_SFM_H
#include <stddef.h>
#ifdef __cplusplus
extern "C" {
#endif

#define OPSFM_ABI_VERSION 1
#define OPSFM_MAX_ITEMS 1073741823
#define OPSFM_PAIR_BLOCK 1024
#define OPSFM_PAIR_TILE 256
#define OPSFM_PAIR_MAX_CHUNKS 64

int opsfm_abi_version(void);
const char* opsfm_last_error(void);

/* n_slots: 2D keypoints of all images (stage A's winner table, 4 bytes each); n_points: points that enter the merge (1 byte each) */
size_t opsfm_workspace_bytes(long long n_slots, long long n_points);

/* Stage A.  P tracks, track p owning rows row_offsets[p] .. row_offsets[p + 1]; R rows; I images; U = kpt_offsets[I] slots.
 * desc_coarse [U][dim_c], desc_fine [U][dim_f] float32 and written / scores_cleared [U] bytes are fully written (0 where nothing lands). */
int opsfm_aggregate(const long long* assigned_image, const long long* assigned_kpt, const long long* row_offsets,
                    const long long* ref_image, const long long* ref_kpt, const float* feature_c0, const float* feature_c1,
                    const float* feature0, const float* feature1, const long long* kpt_offsets, int P, long long R, int I, long long U,
                    int dim_c, int dim_f, void* workspace, size_t workspace_bytes, float* desc_coarse, float* desc_fine,
                    unsigned char* written, unsigned char* scores_cleared, void* stream);

/* Stage B, step 1.  xyz [Q][3], corners [8][3] float64; keep [Q] bytes = 0 < (p - c4).v < v.v for v45, v40, v47, strictly. */
int opsfm_box_test(const double* xyz, long long Q, const double* corners, unsigned char* keep, void* stream);

/* Stage B, step 4: the pair test sqrt((dx^2 + dy^2) + dz^2) < dist_threshold over N points, never as a matrix.  The points j are cut in
 * blocks of OPSFM_PAIR_BLOCK, the partners i in n_chunks chunks of chunk_len (a multiple of OPSFM_PAIR_TILE); counts [N][n_chunks] int64
 * receives how many partners of j (itself included) chunk c holds.  After an exclusive scan of the flattened counts into
 * positions [N * n_chunks + 1], opsfm_pair_emit writes the partner indices, ascending per point, into neighbours [E] (int32). */
int opsfm_pair_count(const double* xyz, int N, double dist_threshold, int chunk_len, int n_chunks, long long* counts, void* stream);
int opsfm_pair_emit(const double* xyz, int N, double dist_threshold, int chunk_len, int n_chunks, const long long* positions,
                    int* neighbours, long long E, void* stream);

/* The reference's sequential rule over the M points that have a partner besides themselves (multi [M], ascending): one workgroup walks
 * them in order; accepted [N] bytes must hold 1 for every point that is alone and 0 elsewhere, and receives 1 for every accepted point. */
int opsfm_merge_resolve(const long long* positions, int n_chunks, const int* neighbours, const long long* multi, int M, int N,
                        void* workspace, size_t workspace_bytes, unsigned char* accepted, void* stream);

/* New point g = accepted_idx[g]: keypoints3d [G][3] = float64 mean of its partners' xyz in ascending index order, group_members
 * [group_offsets[g] ..] = their ids in that order. */
int opsfm_group_emit(const double* xyz, const long long* ids, const long long* accepted_idx, const long long* positions, int n_chunks,
                     const int* neighbours, const long long* group_offsets, int G, int N, double* keypoints3d, long long* group_members,
                     long long members_total, void* stream);

/* Stage C.  table [U][dim] float32; point g owns observations obs[run_offsets[g] .. run_offsets[g + 1]) (rows of the table, already in
 * the summation order); out [G][dim] float64 = running float64 sum in that order, then one division by the count. */
int opsfm_point_mean(const float* table, long long U, int dim, const long long* obs, const long long* run_offsets, int G, double* out,
                     void* stream);

#ifdef __cplusplus
}
#endif
#endif
