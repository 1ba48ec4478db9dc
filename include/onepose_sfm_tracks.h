/* libonepose_sfm_tracks.so -- the step of the keypoint-free SfM between the triangulated model and the fine matcher / the optimiser,
 * on the device (gfx950): greedy keyframe selection with the feature-track assignment, the fine matcher's pair rows, and the per-track
 * rows of the optimiser and the feature aggregation.  C ABI; its own library, so that libonepose_hip.so (the frame path) and
 * libonepose_sfm.so are built from exactly the sources they were built from before.
 *
 * The reference: src/KeypointFreeSfM/dataset/coarse_colmap_dataset.py (get_keyframes_greedy, build_initial_depth_pose,
 * extract_corresponding_frames), post_optimization/data_construct/construct_matching_data.py and construct_optimization_data.py.
 * The contract of every entry is in onepose_st_amd/sfm_tracks.py and DESIGN.md section 6i.
 *
 * Every entry returns 0, or -1 on invalid arguments, or a positive HIP error code; opsft_last_error() says which.  All pointers are
 * device pointers; `stream` is a hipStream_t.  Images are 0 .. I - 1, the 2D keypoints of all images form one table of U slots
 * (kpt_offsets [I + 1]), points are 0 .. Q - 1 and own the track elements track_offsets[q] .. track_offsets[q + 1] of E.  The tables
 * are validated by the caller before any launch; the kernels also refuse to write outside their outputs.
 *
 * Slot states (int): -1 unregistered, -2 unoccupied, -3 robbed, >= 0 the index of the point the slot owns.
 */
#ifndef ONEPOSE_SFM_TRACKS_H
#define ONEPOSE_SFM_TRACKS_H
#include <stddef.h>
#ifdef __cplusplus
extern "C" {
#endif

#define OPSFT_ABI_VERSION 1
/* the per-round ordering of the remaining images lives in one workgroup (one image per thread): I above this is refused */
#define OPSFT_MAX_IMAGES 1024
#define OPSFT_MAX_ITEMS 1073741823
/* ctrl [OPSFT_CTRL_INTS] int: 0 done flag, 1 images still in the order, 2 keyframes selected, 3 the current keyframe */
#define OPSFT_CTRL_INTS 4

int opsft_abi_version(void);
const char* opsft_last_error(void);

/* The greedy rounds: I times (select, take) enqueued back to back; every launch reads ctrl[0] first and returns once it is set.
 * In:  slot_point [U] (point index or -1), elem_image / elem_slot [E] (image and slot of every track element), max_slots (the largest
 *      image, sizes the grid).
 * In/out, initialised by the caller: state [U] (-1 / -2), count [I] (-2 slots per image), order [I] = 0 .. I - 1,
 *      assigned_image / assigned_kpt [Q] = -1, keyframes [I], ctrl = {0, I, 0, -1}.
 * Out: state, assigned_image / assigned_kpt (the later keypoint wins when a keyframe sees a point twice), keyframes [ctrl[2]] in
 *      selection order. */
int opsft_assign(const long long* kpt_offsets, const long long* slot_point, const long long* track_offsets, const long long* elem_image,
                 const long long* elem_slot, int I, long long U, int Q, long long E, int max_slots, int* state, int* count, int* order,
                 int* assigned_image, int* assigned_kpt, int* keyframes, int* ctrl, void* stream);

/* state_ids [U] = the owned point's id (point_ids) or the negative state; initial_depth [U] = z of K (R X + t) in float64 on occupied
 * slots (all of them lie in keyframes), -1 elsewhere.  K, R [I][3][3], t [I][3], xyz [Q][3]. */
int opsft_finish(const int* state, const long long* slot_image, const long long* point_ids, const double* xyz, const double* K,
                 const double* R, const double* t, int I, long long U, int Q, long long* state_ids, double* initial_depth, void* stream);

/* Per track element e of point elem_point[e]: other [E] bytes = 1 where e is the first element of its image in the track and that
 * image is not the point's assigned one (the rows of the optimiser, in order); match_kpt [E] = the keypoint of that first occurrence
 * (the pair rows' mkpts1_c), ref_kpt [E] = the keypoint of the image's last occurrence (the optimiser rows' pairs_dict value).
 * Both are written where e is a first occurrence, -1 elsewhere. */
int opsft_track_rows(const long long* track_offsets, const long long* elem_point, const long long* elem_image, const long long* track_kpt,
                     const int* assigned_image, int Q, long long E, unsigned char* other, long long* match_kpt, long long* ref_kpt,
                     void* stream);

/* Pair row m = (owner_slot[m], element row_elem[m]): keys [M] = ((left * I + id_rank[right]) * key_stride + left keypoint), the order of
 * the fine matcher's work list (left images by index, right images by ascending id, rows by left keypoint). */
int opsft_pair_keys(const long long* owner_slot, const long long* row_elem, const long long* slot_image, const long long* kpt_offsets,
                    const long long* elem_image, const long long* id_rank, int I, long long U, long long E, long long M,
                    long long key_stride, long long* keys, void* stream);

/* Sorted position r takes pair row perm[r]: mkpts0_c / mkpts1_c [M][2] are copies of xys [U][2], mkpts0_idx [M] the left keypoint,
 * row_left / row_right [M] the images. */
int opsft_pair_emit(const long long* perm, const long long* owner_slot, const long long* row_elem, const long long* slot_image,
                    const long long* kpt_offsets, const long long* elem_image, const long long* match_kpt, const double* xys, int I,
                    long long U, long long E, long long M, double* mkpts0_c, double* mkpts1_c, long long* mkpts0_idx,
                    long long* row_left, long long* row_right, void* stream);

/* Optimiser row j of point row_point[j] with reference image ref_image[j]: fine_row [R] = the one pair row with
 * (left, right) = (assigned_image, ref_image) and mkpts0_idx == assigned_kpt, by binary search in the pair list (sorted as
 * opsft_pair_keys orders it); -1 and error_flag[0] |= 1 unless exactly one such row exists. */
int opsft_fine_rows(const long long* row_point, const long long* ref_image, const int* assigned_image, const int* assigned_kpt,
                    const long long* image_ids, const long long* pair_left, const long long* pair_right, const long long* pair_offsets,
                    const long long* mkpts0_idx, int I, int Q, long long R, long long Np, long long M, long long* fine_row,
                    int* error_flag, void* stream);

#ifdef __cplusplus
}
#endif
#endif
