/* libonepose_sfm_fine.so -- the fine half of the keypoint-free SfM's matcher over a whole pair list, on the device (gfx950): the
 * per-row forms of ophip_loftr_coarse_ids and ophip_sample_features, which read every row's own image through device tables instead
 * of taking one image pair per call.  C ABI; its own library, so that libonepose_hip.so and the other SfM libraries are built from
 * exactly the sources they were built from before.
 *
 * The reference: src/KeypointFreeSfM/loftr_for_sfm/loftr.py:79-167 (the fine-only branch and the feature extraction), called once per
 * pair by post_optimization/matcher_model/fine_match_worker.py.  The contract of every entry is in onepose_st_amd/sfm_fine.py and
 * DESIGN.md section 6k.
 *
 * Every entry returns 0, or -1 on invalid arguments, or a positive HIP error code; opsff_last_error() says which.  All pointers are
 * device pointers; `stream` is a hipStream_t.  Images are 0 .. I - 1; image_hw [I][2] int holds (H, W), image_scale [I][2] float the
 * reference's (h factor, w factor).  Pair rows are 0 .. M - 1; row_left / row_right [M] name the two images of a row.  Both kernels
 * refuse to read outside the tables they are given: a row whose image index lies outside [0, I) is counted as a bad id / sampled as
 * zeros.
 */
#ifndef ONEPOSE_SFM_FINE_H
#define ONEPOSE_SFM_FINE_H
#include <stddef.h>
#ifdef __cplusplus
extern "C" {
#endif

#define OPSFF_ABI_VERSION 1
#define OPSFF_MAX_ROWS 1073741823
/* ctrl [OPSFF_CTRL_INTS] int: 0 the number of ids outside their grid (both sides counted), 1 the smallest row with such an id
 * (OPSFF_NO_ROW when there is none) */
#define OPSFF_CTRL_INTS 2
#define OPSFF_NO_ROW 2147483647

int opsff_abi_version(void);
const char* opsff_last_error(void);

/* The per-row form of ophip_loftr_coarse_ids, the same arithmetic in the same order without FMA: per row and side the keypoint
 * (mkpts* [M][2] (x, y), float, or double when mk*_double != 0; read only) is clipped to [0, W - 2] x [0, H - 2] of the row's own image
 * into mkpts*_out (same dtype), divided by coarse_scale * image_scale[image][[1, 0]], rounded half to even, and id = y * (W / 8) + x
 * truncated to int64 -> i_ids / j_ids [M].  Ids outside [0, (H / 8) * (W / 8)) (NaN keypoints and image indices outside [0, I) too)
 * are counted into ctrl[0], the smallest such row goes to ctrl[1]; the call initialises ctrl. */
int opsff_row_ids(const void* mkpts0, int mk0_double, const void* mkpts1, int mk1_double, const long long* row_left,
                  const long long* row_right, const int* image_hw, const float* image_scale, int I, long long M, float coarse_scale,
                  void* mkpts0_out, void* mkpts1_out, long long* i_ids, long long* j_ids, int* ctrl, void* stream);

/* The per-row form of ophip_sample_features, the same arithmetic in the same order: all four feature tables of n pair rows in one
 * launch, one wave per row and table.  The rows are rows[0 .. n) (rows NULL: row0 .. row0 + n) of tables with M rows.  All left images
 * of these rows lie in one group of n_group0 equally sized images (H0 x W0): coarse0 [n_group0][(H0 / 8) * (W0 / 8)][256] and
 * fine0 [n_group0][(H0 / 2) * (W0 / 2)][128], channels last, *_bstride floats between images; the right images likewise.  A row reads
 * the maps of image_index[row_left[r]] / image_index[row_right[r]] (the index within the group).  Keypoints mkpts0 / mkpts1 [M][2] are
 * normalised by image_scale[image] * (H, W) as the reference does; coarse rows are sampled nearest (half to even), fine rows bilinear,
 * zero padding, align_corners -> feature_c0 / feature_c1 [M][256], feature0 / feature1 [M][128] float, written at row r.  Maps and
 * outputs 16-byte aligned. */
int opsff_sample_rows(const float* coarse0, long long coarse0_bstride, const float* fine0, long long fine0_bstride, int n_group0, int H0,
                      int W0, const float* coarse1, long long coarse1_bstride, const float* fine1, long long fine1_bstride, int n_group1,
                      int H1, int W1, const void* mkpts0, int mk0_double, const void* mkpts1, int mk1_double, const long long* row_left,
                      const long long* row_right, const long long* image_index, const float* image_scale, int I, const long long* rows,
                      long long row0, int n, long long M, float* feature_c0, float* feature_c1, float* feature0, float* feature1,
                      void* stream);

#ifdef __cplusplus
}
#endif
#endif
