/* libonepose_encoder_backward.so -- the backward of one LoFTREncoderLayer with linear attention on the device (gfx950): from the gradient
 * at the layer's output to the gradients at its two inputs and at all of its parameters.  C ABI; its own library
 * (the row of cabi.ENCODER_BACKWARD: DESIGN.md section 1b).
 *
 * This header is the specification; tests/encoder_backward_oracle.py restates it in numpy float64, one function per entry.  The function
 * differentiated is one call of the reference's LoFTREncoderLayer.forward(x, source) with attention "linear", LayerNorm, dropout 0, no
 * rezero and no masks (oracle/onepose_oracle.py::encoder_layer).  The entry takes the layer's INPUTS and recomputes the forward itself: it
 * reads nothing a forward kernel left behind.  Masks, full attention, the fine transformer's width, an optimiser: not here.
 *
 * Every entry returns 0, or -1 on invalid arguments (checked before any launch), or a positive HIP error code; openb_last_error() says
 * which.  Pointers are device pointers; `stream` is a hipStream_t; nothing is synchronised and nothing is read on the host.  No workgroup
 * waits for another; there are no float atomics and no sum whose order depends on the schedule: every sum over rows is taken in a fixed
 * order, its split a function of the shape alone, so two runs give identical bytes.
 */
#ifndef ONEPOSE_ENCODER_BACKWARD_H
#define ONEPOSE_ENCODER_BACKWARD_H
#include <stddef.h>
#ifdef __cplusplus
extern "C" {
#endif

#define OPENB_ABI_VERSION 1
#define OPENB_CHANNELS 256
#define OPENB_HEADS 8
#define OPENB_HEAD_DIM 32
#define OPENB_HIDDEN 512
#define OPENB_MAX_BATCH 65535
#define OPENB_MAX_ROWS 1048576
/* B * L and B * S are at most this */
#define OPENB_MAX_TOTAL_ROWS 4194304
/* the rows of one wave's output tile in the row GEMMs (a workgroup: OPENB_ROW_TILE rows by 256 columns) */
#define OPENB_ROW_TILE 64
/* the rows of one LayerNorm / attention workgroup */
#define OPENB_ROW_BLOCK 32
/* THE SPLIT RULE of every sum over rows that is taken by a matrix product (KV, Ks, dKV, dKs over the S or L rows of ONE frame; the six dW
 * over all B * L or B * S rows): for T rows
 *     rows_per_split = max(OPENB_SPLIT_ROWS, round_up(ceil(T / OPENB_MAX_SPLITS), 32));   splits = ceil(T / rows_per_split)
 * split s takes the rows [s * rows_per_split, min(T, (s + 1) * rows_per_split)) in ascending steps of 16 into its own partial buffer; one
 * owner thread per element then adds the partials of splits 0, 1, .. in that order from 0.0f.  Never a function of the CU count. */
#define OPENB_SPLIT_ROWS 128
/* at most this many partial buffers per sum: the bound of the workspace's weight-sized part (the largest, dW of mlp.0, is 1 MiB each) */
#define OPENB_MAX_SPLITS 16

/* params and dparams: ONE contiguous float32 buffer each, of OPENB_PARAM_FLOATS floats, 16-byte aligned; every matrix [out][in] row-major as
 * the state dict has it.  Offsets in floats: */
#define OPENB_PARAM_FLOATS 656384
#define OPENB_OFF_Q_PROJ 0
#define OPENB_OFF_K_PROJ 65536
#define OPENB_OFF_V_PROJ 131072
#define OPENB_OFF_MERGE 196608
#define OPENB_OFF_MLP0 262144
#define OPENB_OFF_MLP2 524288
#define OPENB_OFF_NORM1_WEIGHT 655360
#define OPENB_OFF_NORM1_BIAS 655616
#define OPENB_OFF_NORM2_WEIGHT 655872
#define OPENB_OFF_NORM2_BIAS 656128
/* q_proj [256][256], k_proj [256][256], v_proj [256][256], merge [256][256], mlp.0 [512][512], mlp.2 [256][512], norm1.weight [256],
 * norm1.bias [256], norm2.weight [256], norm2.bias [256].  k_proj and v_proj are neighbours on purpose: together they are one [512][256]
 * matrix Wkv, and the device forms k and v, dWk and dWv, and dsource with one product each. */

int openb_abi_version(void);
const char* openb_last_error(void);

/* The layer.  x [B][L][256], source [B][S][256], dy [B][L][256] float32 contiguous; H = 8 heads of D = 32 (head h: columns 32 h .. 32 h + 31);
 * eps = 1e-6; LayerNorm eps 1e-5.  Forward (float64 in the specification):
 *     q = x Wq^T      k = source Wk^T      v = source Wv^T
 *     Q = phi(q)      K = phi(k)           v' = v / S                  phi(t) = t > 0 ? t + 1 : exp(t)   (elu(t) + 1)
 *     KV_h = K_h^T v'_h  [32 x 32]         Ks_h = sum_s K_sh  [32]     (per frame b and head h)
 *     den_lh = Q_lh . Ks_h + eps           Z = 1 / den
 *     num_lh = Q_lh KV_h                   m_lh = num_lh * (Z_lh * S)
 *     msg = m Wm^T    n1 = LN1(msg)        hc = [x, n1]  (512)
 *     h = relu(hc W0^T)  (512)             o = h W2^T  (256)
 *     n2 = LN2(o)     y = x + n2
 *     LN(z) = zhat * weight + bias,  zhat = (z - mean) * rstd,  mean and the biased variance over the 256 columns, rstd = 1 / sqrt(var + 1e-5)
 * Backward, given dy:
 *     dn2 = dy;   do, dg2, db2 = LN2'(o; dn2)            LN'(z; dn): g = dn * weight;  dz = rstd * (g - mean_c(g) - zhat * mean_c(g * zhat));
 *                                                        dweight = sum_rows dn * zhat;  dbias = sum_rows dn
 *     dW2 = do^T h;   dh = (do W2) * [h > 0];   dW0 = dh^T hc;   dhc = dh W0
 *     dn1 = dhc[:, 256:];   dmsg, dg1, db1 = LN1'(msg; dn1);   dWm = dmsg^T m;   dm = dmsg Wm
 *     dnum = dm * (Z * S);   dden_lh = -Z_lh * (dm_lh . m_lh)            (= -Z^2 S (dm . num): m = num Z S, so num is not kept)
 *     dQ_lh = KV_h dnum_lh + dden_lh Ks_h;   dKV_h = sum_l Q_lh^T dnum_lh;   dKs_h = sum_l dden_lh Q_lh
 *     dK_sh = dKV_h v'_sh + dKs_h;   dv_sh = (K_sh dKV_h) / S
 *     dq = dQ * phi'(q);   dk = dK * phi'(k)                             phi'(t) = t > 0 ? 1 : exp(t) = min(phi(t), 1): Q and K are kept, q and k not
 *     dWq = dq^T x;   dWk = dk^T source;   dWv = dv^T source
 *     dx = (dq Wq + dy) + dhc[:, :256];   dsource = [dk, dv] Wkv  (= dk Wk + dv Wv)
 * The only kink is the ReLU; den > 0 always.
 *
 * x == source (a self layer) is allowed; the inputs are only read.  dx [B][L][256] and dsource [B][S][256] are always fully written, in
 * distinct buffers (the caller adds them where a stream is both).  dparams: accumulate == 0 writes every element; accumulate != 0 forms
 * old + new once per element, new being the complete sum of this call.  dx and dsource of frame b depend on frame b alone: a B = 2 call
 * gives the bytes of its two B = 1 halves (dparams sums over the batch and does not).
 *
 * The device works in float32 around split-bf16 matrix products (t = hi + lo, hi = bf16(t), lo = bf16(t - hi); a . b taken as
 * a_lo . b_hi + a_hi . b_lo + a_hi . b_hi on v_mfma_f32_32x32x16_bf16, f32 accumulate: tile_bf16.h).  BOTH operands of every product below
 * are split, where they are read from float32 memory; these are all the points at which a value is split:
 *     row GEMMs, contracting over columns (with the five dW launches below the layer's eighteen row products: k and v, dk Wk and dv Wv, dWk
 *     and dWv are one launch each):
 *       1  Q  = phi(x Wq^T)                              operands x, Wq
 *       2  [K, v'] = source Wkv^T, phi on the first 256 columns, times the float32 1 / S on the rest      source, Wkv
 *       6  msg = m Wm^T                                  m, Wm
 *       8  h  = relu(hc W0^T)                            hc, W0
 *       9  o  = h W2^T                                   h, W2
 *      12  dh = (do W2) * [h > 0]   (in place over h)    do, W2
 *      14  dhc = dh W0              (in place over hc)   dh, W0
 *      17  dm = dmsg Wm                                  dmsg, Wm
 *      23  dx = (dq Wq + dy) + dhc[:, :256]              dq, Wq
 *      24  dsource = [dk, dv] Wkv                        [dk, dv], Wkv
 *     row-contracted products (the A operand is read transposed from row-major memory, eight rows per lane; T2 / T10 of the kernel guide
 *     are not needed: a lane's eight values of one column are eight coalesced 128-byte wave reads), each followed by the owner's sum:
 *       3  KV_h, Ks_h  per frame and head over S         K, v' (Ks: K against bf16 ones, exact)
 *      11  dW2 = do^T h          13  dW0 = dh^T hc       16  dWm = dmsg^T m
 *      19  dKV_h, dKs_h per frame and head over L        Q, dnum, dden
 *      21  dWq = dq^T x          22  dWkv = [dk, dv]^T source
 *     The four per-head 32 x 32 applications (Q KV, KV dnum, dKV v', K dKV) and Q . Ks are float32 on the vector ALU, KV in LDS, one
 *     thread per row and head, every sum over d or v ascending from 0.0f (launches 5, 18, 20).  LayerNorm (7, 10, 15) is float32, two-pass,
 *     one wave per row; its parameter gradients are summed per OPENB_ROW_BLOCK rows (wave w: rows 8 w .. 8 w + 7 ascending, then waves 0..3),
 *     then over the blocks ascending by one thread per element (25).  Z, dden and the statistics are float32.
 * Nothing is fused beyond the epilogues named above; DESIGN.md 6v lists what a fused form would save.
 *
 * workspace: openb_layer_workspace_bytes(B, L, S) bytes (0: a shape outside the limits), 256-byte aligned.  Per row of x 2 320 floats
 * (Q, m, msg, o, do: 256 each; hc, h: 512; Z, dden: 8), per row of source 512 ([K, v']), per OPENB_ROW_BLOCK rows of x 1 024 (LayerNorm
 * partials), per frame and split the KV / Ks and dKV / dKs partials (8 448 floats) and per frame their sums, and OPENB_MAX_SPLITS weight-sized
 * partial buffers of 512 x 512 floats: O(B (L + S)) plus 16 MiB. */
size_t openb_layer_workspace_bytes(int B, int L, int S);
int openb_layer_grads(const float* x, const float* source, const float* dy, int B, int L, int S, const float* params, void* workspace,
                      size_t workspace_bytes, float* dx, float* dsource, float* dparams, int accumulate, void* stream);

#ifdef __cplusplus
}
#endif
#endif
