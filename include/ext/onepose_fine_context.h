/* libonepose_fine_context.so -- the coarse context of the LoFTR matcher's fine windows (fine_concat_coarse_feat, gfx950): the step of the
 * published FinePreprocess between the window gather and the fine transformer, for both images in one call.  C ABI; its own library, so
 * that libonepose_hip.so is built from exactly the sources it was built from before.  The header stands under include/ext/ because the
 * table of libraries (cabi.LIBRARIES) is pinned against include/onepose_*.h; this one is bound from cabi.EXTENSIONS.
 *
 * With down_proj = Linear(256, 128) (Wd, bd), merge_feat = Linear(256, 128) (Wm, bm), for every match k of image s (0, 1):
 *     c  = Wd . coarse_s[b_ids[k]][ids_s[k]] + bd                     (ids_0 = i_ids, ids_1 = j_ids)
 *     u  = Wm[:, 128:] . c + bm                                        (once per match and image)
 *     out_s[k][r] = Wm[:, :128] . win_s[k][r] + u,  r = 0 .. W * W - 1
 * which is merge_feat(cat[win_s[k][r], c]) with the repeated context never stored.  The three products take split-bf16 operands
 * (x = hi + lo, lo . lo dropped, f32 accumulation: the arithmetic of ophip_rows_linear_x3); the biases are added in f32.
 *
 * Every entry returns 0, or -1 on invalid arguments, or a positive HIP error code; opfcx_last_error() says which.  All pointers are
 * device pointers, 16-byte aligned; `stream` is a hipStream_t.
 */
#ifndef ONEPOSE_FINE_CONTEXT_H
#define ONEPOSE_FINE_CONTEXT_H
#include <stddef.h>
#ifdef __cplusplus
extern "C" {
#endif

#define OPFCX_ABI_VERSION 1
/* rows of one workgroup of either kernel */
#define OPFCX_TILE_ROWS 64
/* K * W * W of one call */
#define OPFCX_MAX_ROWS 1073741824

int opfcx_abi_version(void);
const char* opfcx_last_error(void);

/* bytes of wpack (packing.pack_fine_context): the 16-k fragments of Wd [128][256], Wm[:, :128] and Wm[:, 128:] as a hi plane, then
 * the same as a lo plane (bf16), then bd [128] and bm [128] (f32) */
size_t opfcx_wpack_bytes(void);

/* floats of the scratch `context` of a call with K matches: u of both images, [2][K][128] */
size_t opfcx_context_floats(int K);

/* win0, win1 [K][W * W][128] -> out0, out1 [K][W * W][128].  out_s == win_s (in place) and disjoint buffers give the same bits; any
 * other overlap is undefined.  coarse0 [B][L0][256], coarse1 [B][L1][256] with coarse*_bstride floats between images (0: one image for
 * every match; otherwise a multiple of 4, at least L * 256); b_ids, i_ids, j_ids [K].  A match whose b_ids / i_ids / j_ids entry lies
 * outside [0, B) / [0, L0) / [0, L1) reads a zero coarse row: nothing outside the tables is touched.  context: opfcx_context_floats(K)
 * floats, overwritten.  Two launches (the contexts, then the rows); K == 0 launches nothing and writes nothing; rows of matches >= K
 * are never touched.  -1: a null pointer, K < 0, B < 1, L0 < 1, L1 < 1, W even or outside 3 .. 11, K * W * W > OPFCX_MAX_ROWS, a
 * misaligned pointer, a bad stride. */
int opfcx_merge(const float* win0, const float* win1, const float* coarse0, long long coarse0_bstride, const float* coarse1,
                long long coarse1_bstride, const long long* b_ids, const long long* i_ids, const long long* j_ids, int K, int B, int L0,
                int L1, int W, const void* wpack, float* context, float* out0, float* out1, void* stream);

#ifdef __cplusplus
}
#endif
#endif
