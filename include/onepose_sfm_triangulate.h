/* libonepose_sfm_triangulate.so -- the step of the keypoint-free SfM between the merged coarse matches (sfm_coarse) and the track model
 * (sfm_tracks), on the device (gfx950): match rows become components (union-find), every component is triangulated from two-view
 * hypotheses scored against all its observations, refit, refined and filtered, in float64.  C ABI; its own library, so that
 * libonepose_hip.so, libonepose_sfm.so and libonepose_sfm_tracks.so are built from exactly the sources they were built from before.
 *
 * The reference shells out to COLMAP's point_triangulator (src/sfm_utils/triangulation.py:195-250); the arithmetic here is this
 * project's own specification: onepose_st_amd/sfm_triangulate.py and DESIGN.md section 6j.
 *
 * Every entry returns 0, or -1 on invalid arguments, or a positive HIP error code; opstr_last_error() says which.  All pointers are
 * device pointers; `stream` is a hipStream_t.  Images are 0 .. I - 1, the 2D keypoints of all images form one table of U slots.  The
 * tables are validated by the caller before any launch; the kernels also refuse to read or write outside their tables.
 */
#ifndef ONEPOSE_SFM_TRIANGULATE_H
#define ONEPOSE_SFM_TRIANGULATE_H
#include <stddef.h>
#ifdef __cplusplus
extern "C" {
#endif

#define OPSTR_ABI_VERSION 1
#define OPSTR_MAX_ITEMS 1073741823
/* a component of at most this many candidates is one wavefront's (its rays and camera rows in LDS); a longer one is a workgroup's */
#define OPSTR_SHORT_TRACK 64
#define OPSTR_MAX_HYPOTHESES 65536
#define OPSTR_MAX_REFINE_STEPS 64
#define OPSTR_MAX_ROUNDS 255
/* doubles per image in the camera table: P = K [R | t] row-major [3][4], then the centre -R^T t, one pad */
#define OPSTR_CAMERA_DOUBLES 16
/* a squared reprojection cost below n * OPSTR_COST_FLOOR (n observations, px^2) is rounding noise and counts as 0 in the refine guard */
#define OPSTR_COST_FLOOR 1e-18
#define OPSTR_PARALLEL_SIN 1e-12

int opstr_abi_version(void);
const char* opstr_last_error(void);

/* bytes of the workspace opstr_round needs for n_elems candidate elements (the unit directions and inlier marks of long components) */
size_t opstr_workspace_bytes(long long n_elems);

/* Components of the graph with nodes 0 .. U - 1 and edges (slot0[t], slot1[t]): labels [U] = the smallest node of each node's
 * component.  parent [U] int is scratch.  Lock-free union-find: hook the larger root under the smaller with one compare-and-swap, then
 * flatten; no workgroup waits for another. */
int opstr_components(const long long* slot0, const long long* slot1, long long T, long long U, int* parent, long long* labels,
                     void* stream);

/* cameras [I][OPSTR_CAMERA_DOUBLES] from K, R [I][3][3], t [I][3]; dirs [U][3] = the unit ray of every slot in world coordinates,
 * R^T K^-1 (x, y, 1) normalised, with K = [[fx, s, cx], [0, fy, cy], [0, 0, 1]]. */
int opstr_prepare(const double* K, const double* R, const double* t, const double* xys, const long long* slot_image, int I, long long U,
                  double* cameras, double* dirs, void* stream);

/* One round over C components.  Component c owns the candidates elem_slot[comp_offsets[c] .. comp_offsets[c + 1]) (ascending slots) and
 * has the label comp_label[c].  Launch 1 takes every component of at most OPSTR_SHORT_TRACK candidates, one wavefront each; launch 2
 * takes long_comps [n_long] (the indices of the longer ones), one workgroup each.
 * Out: ok [C] (1: a point), xyz [C][3], point_error [C], min_slot [C] (the point's smallest slot), and assigned[slot] = point_base + c on
 * the inliers of a kept point (other entries are left as they are). */
int opstr_round(const long long* comp_offsets, const long long* comp_label, const long long* elem_slot, const long long* long_comps,
                long long C, long long n_long, long long n_elems, const long long* slot_image, const double* xys, const double* cameras,
                const double* dirs, int I, long long U, int round, double max_reproj_error, double cos_min_tri_angle,
                int max_hypotheses, int refine_steps, long long point_base, void* workspace, size_t workspace_bytes, int* ok, double* xyz,
                double* point_error, long long* min_slot, long long* assigned, void* stream);

#ifdef __cplusplus
}
#endif
#endif
