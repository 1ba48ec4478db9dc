/* libonepose_temporal.so -- the temporal pose refinement on the device (gfx950): a pyramidal, translation-only Lucas-Kanade tracker
 * with a forward-backward check, and the glue that carries a frame's 2D-3D matches into a later frame's match table in front of a second
 * PnP.  C ABI; its own library (a row of cabi.LIBRARIES: DESIGN.md section 1b).
 *
 * This header is the specification; tests/temporal_oracle.py restates it in numpy, one function per entry.  All per-point arithmetic is
 * float64, every expression evaluated in the written order with contraction off; the operations are + - * /, sqrt, floor and
 * comparisons, so the device equals numpy bit for bit.
 *
 * Every entry returns 0, or -1 on invalid arguments (checked before any launch), or a positive HIP error code; optmp_last_error() says
 * which.  Pointers are device pointers unless said otherwise; `stream` is a hipStream_t.  Every count is a device int clamped to its
 * capacity (NULL: the capacity); rows at or past the count are never read and their outputs never written; every launch is sized by the
 * capacity; nothing is synchronised and no count is read on the host.
 */
#ifndef ONEPOSE_TEMPORAL_H
#define ONEPOSE_TEMPORAL_H
#include <stddef.h>
#ifdef __cplusplus
extern "C" {
#endif

#define OPTMP_ABI_VERSION 1
#define OPTMP_MAX_LEVELS 6
#define OPTMP_MIN_WINDOW 3
#define OPTMP_MAX_WINDOW 31
#define OPTMP_MAX_ITERS 1000
#define OPTMP_MAX_SIDE 16384
#define OPTMP_MAX_ROWS 1048576
#define OPTMP_MAX_SOURCES 8
/* flags [cap]: the first four mean the track is lost (OPTMP_LOST is their union); OPTMP_FLAG_MAX_ITERS is informational */
#define OPTMP_DEGENERATE 1
#define OPTMP_OUT_OF_IMAGE 2
#define OPTMP_FB_FAIL 4
#define OPTMP_BAD_INPUT 8
#define OPTMP_FLAG_MAX_ITERS 16
#define OPTMP_LOST 15

int optmp_abi_version(void);
const char* optmp_last_error(void);

/* 1. The pyramid of an H x W frame with `levels` levels, one allocation.  Level 0 is the frame as float32, H x W; level l + 1 has
 * ceil(h / 2) x ceil(w / 2) elements of level l (h x w).  Level l starts at byte offset o_l: o_0 = 0, o_{l+1} = o_l + h_l * w_l * 4
 * rounded up to a multiple of 256; the size is o_levels.  optmp_pyramid_bytes is 0 unless 1 <= levels <= OPTMP_MAX_LEVELS, H and W are
 * in [2, OPTMP_MAX_SIDE] and the smallest level is at least 2 x 2.
 *
 * Level l + 1 = a 5-tap binomial blur of level l, the vertical pass first, then the horizontal pass over its result, of which the even
 * rows and columns are kept: out(y, x) = h5(v5(in))(2 y, 2 x).  A pass reads a[-2] .. a[2] around its element along its axis, indices
 * clamped to the image (border replicated), and computes in float32
 *     (((a[-2] + a[2]) + 4 * (a[-1] + a[1])) + 6 * a[0]) * (1 / 16).
 * One launch per level: both passes go through an LDS tile with its halo. */
size_t optmp_pyramid_bytes(int H, int W, int levels);
int optmp_pyramid(const unsigned char* frame, int H, int W, int levels, void* pyramid, size_t pyramid_bytes, void* stream);

/* 2-6. Track `count` points pts [cap][2] (x, y; level-0 pixels) from the pyramid src into the pyramid dst, both of H x W x levels.
 *
 * sample(I, x, y), I of h x w float32 widened to float64: x0 = floor(x), fx = x - x0, y0 = floor(y), fy = y - y0; the indices x0, x0 + 1,
 * y0, y0 + 1 are clamped to the image (a NaN index clamps to 0); a = I[y0][x0], b = I[y0][x0 + 1], c = I[y0 + 1][x0], d = I[y0 + 1][x0 + 1];
 * top = a + fx * (b - a), bot = c + fx * (d - c), result top + fy * (bot - top).
 *
 * Guess g of a row: with pts_3d, pose and K (all three or none): X = scale * pts_3d[row], cam_i = ((R_i0 * X_0 + R_i1 * X_1) + R_i2 * X_2)
 * + scale * t_i for pose = [R | t] ([3][4], row major), u_i = ((K_i0 * cam_0 + K_i1 * cam_1) + K_i2 * cam_2), g = (u_0 / u_2, u_1 / u_2),
 * used when cam_2 > 1e-12 and g is finite and inside [0, W - 1] x [0, H - 1].  Otherwise guess[row] when guess is not NULL, else p.
 *
 * track(S, D, p, g): p or g not finite, or p outside [0, W - 1] x [0, H - 1]: OPTMP_BAD_INPUT, nothing is sampled.  Else
 * d = (g - p) / 2^(levels - 1), and for l = levels - 1 .. 0, with p_l = p / 2^l and the window offsets o = (ox, oy), ox, oy in
 * [-(window / 2), window / 2], element k = (oy + window / 2) * window + (ox + window / 2):
 *   T_k = sample(S_l, p_l + o), gx_k = 0.5 * (sample(S_l, p_l + o + (1, 0)) - sample(S_l, p_l + o - (1, 0))), gy_k likewise along y;
 *   Gxx = sum gx_k * gx_k, Gxy = sum gx_k * gy_k, Gyy = sum gy_k * gy_k, det = Gxx * Gyy - Gxy * Gxy,
 *   min_eig = ((Gxx + Gyy) - sqrt((Gxx - Gyy) * (Gxx - Gyy) + 4 * (Gxy * Gxy))) / (2 * window^2);
 *   det <= 0 or min_eig < min_eig_threshold (or either is NaN): OPTMP_DEGENERATE, stop.
 *   At most max_iters times: e_k = T_k - sample(D_l, (p_l + d) + o), bx = sum e_k * gx_k, by = sum e_k * gy_k,
 *   delta = ((Gyy * bx - Gxy * by) / det, (Gxx * by - Gxy * bx) / det), d = d + delta, the iteration count goes up by one, and the level
 *   ends once delta.x * delta.x + delta.y * delta.y < eps * eps.  Level 0 ending without that: OPTMP_FLAG_MAX_ITERS (the track counts).
 *   p + 2^l * d outside [0, W - 1] x [0, H - 1] (or NaN): OPTMP_OUT_OF_IMAGE, stop.  Then, for l > 0, d = 2 * d.
 * Result q = p + d.
 *
 * Sums: one wave of 64 lanes per point; element k belongs to lane k % 64; a lane adds its elements in ascending k starting from 0; the 64
 * partials x go through the butterfly x = x + x[lane ^ off] for off = 32, 16, 8, 4, 2, 1, after which every lane holds the same sum.
 *
 * Forward-backward check, when fb_threshold >= 0: the same wave runs track(D, S, q, q - (g - p)) -> back;
 * fb_error = sqrt((back - p).x^2 + (back - p).y^2); a lost backward track (fb_error NaN then) or fb_error > fb_threshold: OPTMP_FB_FAIL.
 *
 * Out, rows below the count only: out_pts [cap][2] = q (NaN, NaN when DEGENERATE, OUT_OF_IMAGE or BAD_INPUT), flags [cap], iterations
 * [cap] (forward iterations over all levels), fb_error [cap] (NaN when not computed).
 * window odd in [3, 31]; max_iters in [1, OPTMP_MAX_ITERS]; eps > 0; min_eig_threshold >= 0; scale > 0; fb_threshold < 0: no check. */
int optmp_track(const void* src, const void* dst, int H, int W, int levels, const double* pts, const int* count, int cap,
                const double* guess, const float* pts_3d, const double* pose, const double* K, double scale, int window, int max_iters,
                double eps, double min_eig_threshold, double fb_threshold, double* out_pts, int* flags, int* iterations, double* fb_error,
                void* stream);

/* 7. The selected rows of one frame's match table (pts_2d [cap][2] crop pixels, pts_3d [cap][3]; row < count and, with mask [cap] not
 * NULL, mask[row] != 0), compacted in ascending row order by one workgroup's scan, and mapped to the original image with the inverse of
 * trans [3][3] (m_ij, row major): c0 = m11 * m22 - m12 * m21, c1 = m12 * m20 - m10 * m22, c2 = m10 * m21 - m11 * m20,
 * det = (m00 * c0 + m01 * c1) + m02 * c2, inverse rows
 *     (c0, m02 * m21 - m01 * m22, m01 * m12 - m02 * m11) / det,  (c1, m00 * m22 - m02 * m20, m02 * m10 - m00 * m12) / det,
 *     (c2, m01 * m20 - m00 * m21, m00 * m11 - m01 * m10) / det   (every entry divided by det on its own),
 * and with it h_i = (n_i0 * x + n_i1 * y) + n_i2, pts_orig = (h_0 / h_2, h_1 / h_2), (x, y) widened from float32.
 * Out: pts_orig [cap][2], out_3d [cap][3] (copies), out_count [1]. */
int optmp_collect(const float* pts_2d, const float* pts_3d, const int* count, int cap, const unsigned char* mask, const double* trans,
                  double* pts_orig, float* out_3d, int* out_count, void* stream);

/* 8. The injected table of a frame: rows [0, own_count) are own_2d / own_3d unchanged; then per source s = 0 .. n_sources - 1 (oldest
 * first) the rows below src_count[s] whose src_flags[s] carry no bit of OPTMP_LOST, in ascending row order: src_pts[s] (float64 [cap_s][2],
 * original image) mapped to the crop by trans (h_i = (m_i0 * x + m_i1 * y) + m_i2, (h_0 / h_2, h_1 / h_2)) and rounded to float32 once,
 * with src_3d[s]'s row.  One launch copies the own rows and leaves their count in out_count; one launch of one workgroup per source
 * appends behind the count the launch before it left, its scan deciding every position.  Rows that do not fit into cap_total are
 * dropped; out_count [1] is the number written.  src_pts / src_3d / src_flags / src_count / src_cap: HOST arrays of n_sources device
 * pointers (src_count[s] NULL: the capacity) and capacities. */
int optmp_inject(const float* own_2d, const float* own_3d, const int* own_count, int cap_own, const void** src_pts, const void** src_3d,
                 const void** src_flags, const void** src_count, const int* src_cap, int n_sources, const double* trans, float* out_2d,
                 float* out_3d, int* out_count, int cap_total, void* stream);

#ifdef __cplusplus
}
#endif
#endif
