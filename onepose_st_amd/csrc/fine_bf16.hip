// Fine-level refinement on the bf16 matrix pipe (plain or split-bf16, tile_bf16.h); same mathematics as csrc/fine.hip
// (reference: loftr_module/fine_preprocess.py:32-55, loftr_module/transformer.py:65-171 with the loftr_fine config,
// utils/fine_matching.py:28-110).
//
// One workgroup (8 waves) refines TWO coarse matches (two 32-row token tiles: rows 0..24 window, row 25 the 3D token,
// 26..31 padding); wave (tt, ft) owns feature tile ft of match tt, so the two matches' dependent chains share each SIMD
// (2 waves/SIMD) and cover each other's MFMA->VALU latencies.  The per-match problem is tiny and latency bound: a
// layer is four GEMM phases (Q|K|V, merge, MLP up, MLP down) whose weight rings are filled one phase AHEAD (tile_bf16.h
// WRing), so no phase starts on a cold L2 round trip.  In-kernel stamps (ophip_debug_stamps) showed the register-only
// attention block to be VALU bound, hence v_exp / v_rcp forms and one phi(Q) conversion shared by both source sets.
//   * K, V are produced as D[token][feature] accumulators, Q as D[feature][token]; the per-match KV / Ksum tiles of both
//     source sets (window, 3D token) and the products phi(Q) KV are formed accumulator-to-operand, entirely in
//     registers (two 16-wide heads per 32-wide tile -> KV masked to its block diagonal);
//   * the residual stream is kept in f32 registers across both layers; the LDS planes only feed the GEMMs;
//   * a token attends to exactly one source set, so phi(Q) is masked per set on its token (lane) axis and both sets
//     accumulate into one numerator / one denominator tile.
#include "tile_bf16.h"
#include <stdlib.h>

// OPHIP_FINE_INTERLEAVE=1 (experiment): no scheduling fence between a match's K|V projection and the other match's attention block, so
// that the compiler may run the one's matrix instructions under the other's vector work
#ifndef OPHIP_FINE_INTERLEAVE
#define OPHIP_FINE_INTERLEAVE 0
#endif
#if OPHIP_FINE_INTERLEAVE
#define OPHIP_FINE_SCHED_FENCE() do {} while (0)
#else
#define OPHIP_FINE_SCHED_FENCE() __builtin_amdgcn_sched_barrier(0)
#endif

namespace {

constexpr int CF = 128, WIN = 25, TOK3D = 25;
constexpr int ROWB = CF * 2;              // X / Y plane pitch (256 B, 16 chunks)
constexpr int HROWB = 2 * CF * 2;         // hidden plane pitch: 256 features (512 B)
constexpr int KB = CF / 16, TS = KB * 64;              // K = 128
constexpr int KB2 = 2 * CF / 16, TS2 = KB2 * 64;       // K = 256
constexpr int W_ELEMS = 10 * CF * CF;                  // bf16 elements per plane and layer

struct FineBArgs {
    const float* feat_f; long long fs_b, fs_c, fs_y, fs_x; int hf, wf;
    const float* desc_f; long long ds_b, ds_c;
    const long long *b_ids, *i_ids, *j_ids;
    const int* count; int cap;   // device-side match count; capacity of the id lists (the grid covers it)
    int stagger, ncu;            // experiment (OPHIP_FINE_STAGGER): units of ~4 k cycles by which workgroups ncu .. 2 ncu - 1 (the second one of each CU) start late
    const float* mkq_c;
    const char* wpack;           // nlayers x (2 * W_ELEMS * 2 + 4 * CF * 4) bytes
    int nlayers; unsigned cross_bits; int enc_enable;
    int wc, stride;
    float fine_scale;
    const float* qscale;         // [B][2] query_image_scale (h, w factors; fine_matching.py:104) or NULL
    float* expec_f; float* mkq_f;
    float* dbg_win; float* dbg_f3;
    unsigned long long* stamps;
};

// One match's attention in the fine stage.  Tokens 0..24 = the 5 x 5 window, 25 = the 3D point (rows 26..31: padding).  A token attends to
// exactly one source set by layer kind -- "self": window -> window, 3D -> itself; "cross": window -> 3D, 3D -> window
// (transformer.py:148-159 on the fine streams) -- and `qt` (Q of feature tile ft as D[feature][token]), `kt`, `vt` (K, V as D[token][feature])
// are this wave's accumulators.  Returns the message tile D[feature][token] (linear_attention.py:29-61, v_length 25 resp. 1).
//
// Round 4: the two small products of the window set run on the EXACT-f32 matrix instruction (v_mfma_f32_32x32x2_f32: one f32 register per
// operand and lane, k = 2 per instruction) straight from the accumulators -- register t of a D[token][feature] tile holds token
// acc_row(t, h) of feature r, which is exactly A[i = r][k = h] / B[k = h][j = r] of that instruction, so
//     KV[f'][f]     = sum_t mfma(phi(K)[t], V[t])          (13 instructions: tokens 0 .. 24; rows 25 .. 31 never enter)
//     num[f][tok]   = sum_t mfma(KV[t], phi(Q)[t])         (t < 8: rows f' of the tile's first head, t >= 8: of its second)
// need no bf16 split, no fragment conversion and no block-diagonal mask: the two heads of a 32-wide tile go to two accumulators and the
// message takes registers 0..7 (rows f < 16) from the first and 8..15 from the second.  The kernel is bound by vector-ALU issue
// (profiles/r03_stamps_fine_pair.txt, DESIGN.md section 4: ~640 vector instructions per attention block, 232 of them conversions and
// masks), the matrix pipe is half idle: 29 f32 instructions (1 856 pipe cycles) replace 36 bf16 ones (1 152) and ~400 vector instructions.
// The denominator phi(Q).Ksum is 16 f32 multiply-adds per lane (Ksum = column sums of phi(K), handed to every lane through the wave's LDS
// strip like k3 / v3 below) -- one reciprocal per head and token instead of one per element.  The reference's v / v_length ... * v_length
// (an fp16 overflow guard, linear_attention.py:52,59) cancels in f32 and is not applied.
//   3D set: ONE source token, so KV = phi(k3)^T v3 has rank one and the message is v3 * a / (a + eps) with a[token][head] = phi(q) . phi(k3).
// sum over the 16 lanes of a DPP row (lanes 16 k .. 16 k + 15), result in all of them
__device__ __forceinline__ float row16_sum_dpp(float v) {
    v += dpp_f<0xB1>(v);
    v += dpp_f<0x4E>(v);
    v += dpp_f<0x141>(v);
    v += dpp_f<0x140>(v);
    return v;
}

// Round 5, "cross" layers: the window set is attended to by ONE token (the 3D point), so the two small matrix products above -- 29 exact-f32
// matrix instructions = 1 856 pipe cycles per match and layer, a tenth of the stage's matrix work -- shrink to a matrix-vector chain on the
// vector ALU: a[t][head] = phi(q3) . phi(k_t) (13 products per lane, summed over the 16 lanes of a head by DPP), message[f] = sum_t a_t v_t[f] /
// (sum_t a_t + eps).  phi(q3) reaches the lanes by feature and the message reaches the 3D token's lanes through the wave's LDS strip.
template <int NS>
__device__ __forceinline__ f32x16 attend_match(f32x16& qt, const f32x16& kt, const f32x16& vt, bool cross, float* strip, int lane) {
#pragma clang fp contract(off)                    // every fused multiply-add below is written out: the one-match and the pair kernel stay bit-identical
    const int r = lane & 31, h = lane >> 5;
    const bool is3d = r == TOK3D;                 // on the token (lane) axis of D[feature][token] tiles
    const bool use_w = cross ? is3d : !is3d;      // this token attends to the window set (else: the 3D token)
#pragma unroll
    for (int reg = 0; reg < 16; ++reg) qt[reg] = elu_plus_one_fast(qt[reg]);
    // phi(K) of the window rows: registers 0..11 hold rows <= 23 in both lane halves, register 12 holds row 24 (h = 0) / 28 (h = 1)
    static_assert(acc_row(11, 1) == 23 && acc_row(12, 0) == 24 && acc_row(13, 0) == TOK3D, "token rows of a D[token][feature] tile");
    float kw[13];
#pragma unroll
    for (int t = 0; t < 12; ++t) kw[t] = elu_plus_one_fast(kt[t]);
    kw[12] = h == 0 ? elu_plus_one_fast(kt[12]) : 0.f;
    // strip (96 floats of this wave): [0, 32) phi(k3), [32, 64) v3 (row 25 = register 13 of lanes 0..31, one feature per lane), [64, 96) Ksum
    // ("cross": phi(q3) by feature, then the 3D token's message by feature)
    if (h == 0) {
        strip[r] = elu_plus_one_fast(kt[13]);
        strip[32 + r] = vt[13];
    }
    f32x16 n0 = zero16(), n1 = zero16();
    float d0 = 0.f, d1 = 0.f;
    if (!cross) {
        f32x16 kvw = zero16();
        float ks = 0.f;
#pragma unroll
        for (int t = 0; t < 13; ++t) {
            kvw = __builtin_amdgcn_mfma_f32_32x32x2f32(kw[t], vt[t], kvw, 0, 0, 0);
            ks += kw[t];
        }
        ks += __shfl_xor(ks, 32, 64);
        if (h == 0) strip[64 + r] = ks;
#pragma unroll
        for (int t = 0; t < 8; ++t) {             // (two independent chains: the second head's instruction issues behind the first's)
            n0 = __builtin_amdgcn_mfma_f32_32x32x2f32(kvw[t], qt[t], n0, 0, 0, 0);
            n1 = __builtin_amdgcn_mfma_f32_32x32x2f32(kvw[8 + t], qt[8 + t], n1, 0, 0, 0);
        }
    } else {
        if (is3d) {                               // lanes 25 and 57: phi(q3) of feature acc_row(reg, h) sits in register reg
#pragma unroll
            for (int reg = 0; reg < 16; ++reg) strip[64 + acc_row(reg, h)] = qt[reg];
        }
        __builtin_amdgcn_wave_barrier();
        const float q3r = strip[64 + r];          // of THIS lane's feature (K, V tiles: one feature per lane)
        float num = 0.f, den = 0.f;
#pragma unroll
        for (int t = 0; t < 13; ++t) {
            const float a_t = row16_sum_dpp(kw[t] * q3r);      // phi(q3) . phi(k_t) over the 16 features of this lane's head
            num = __builtin_fmaf(a_t, vt[t], num);
            den += a_t;
        }
        num = swap32_sum(num);                    // the two halves hold different tokens
        den = swap32_sum(den);
        const float m3 = num * rcp_fast(den + 1e-6f);
        __builtin_amdgcn_wave_barrier();
        if (h == 0) strip[64 + r] = m3;           // (behind every lane's read of phi(q3): LDS operations of one wave complete in order)
    }
    // this lane's 16 features (acc_row(reg, h) = 8 (reg >> 2) + 4 h + (reg & 3): four 16-byte reads per table) of Ksum, phi(k3), v3
    __builtin_amdgcn_wave_barrier();              // (LDS operations of one wave complete in order: only the compiler needs the fence)
    float a0 = 0.f, a1 = 0.f;
    f32x4 third[4];                               // "self": Ksum, "cross": the 3D token's message -- this lane's 16 features of the strip's last table
#pragma unroll
    for (int g = 0; g < 4; ++g) {
        const f32x4 k3 = *reinterpret_cast<const f32x4*>(strip + 8 * g + 4 * h);
        third[g] = *reinterpret_cast<const f32x4*>(strip + 64 + 8 * g + 4 * h);
#pragma unroll
        for (int j = 0; j < 4; ++j) {
            if (g < 2) { a0 = __builtin_fmaf(qt[4 * g + j], k3[j], a0); if (!cross) d0 = __builtin_fmaf(qt[4 * g + j], third[g][j], d0); }      // features 0..15 of the tile: its first head
            else { a1 = __builtin_fmaf(qt[4 * g + j], k3[j], a1); if (!cross) d1 = __builtin_fmaf(qt[4 * g + j], third[g][j], d1); }
        }
    }
    a0 += __shfl_xor(a0, 32, 64);
    a1 += __shfl_xor(a1, 32, 64);
    if (!cross) {
        d0 += __shfl_xor(d0, 32, 64);
        d1 += __shfl_xor(d1, 32, 64);
    }
    // per token and head: Z of the set this token attends to ("self" window tokens: 1 / (phi(q).Ksum + eps) on the matrix result; a token that
    // attends to the 3D point: a / (a + eps) on v3; the 3D token of a "cross" layer: its message is complete)
    const float z0 = (use_w && !cross) ? rcp_fast(d0 + 1e-6f) : a0 * rcp_fast(a0 + 1e-6f);
    const float z1 = (use_w && !cross) ? rcp_fast(d1 + 1e-6f) : a1 * rcp_fast(a1 + 1e-6f);
    f32x16 out;
#pragma unroll
    for (int g = 0; g < 4; ++g) {
        const f32x4 v3 = *reinterpret_cast<const f32x4*>(strip + 32 + 8 * g + 4 * h);
#pragma unroll
        for (int j = 0; j < 4; ++j) {
            const int reg = 4 * g + j;
            const float nm = g < 2 ? n0[reg] : n1[reg];
            const float viaw = cross ? third[g][j] : nm * (g < 2 ? z0 : z1);
            out[reg] = use_w ? viaw : v3[j] * (g < 2 ? z0 : z1);
        }
    }
    __builtin_amdgcn_wave_barrier();              // the strip is rewritten by this wave's next match
    return out;
}

// ---- last stage of a match, from the residual registers (fine_matching.py:28-110) ------------------------------------------------
// sim[r] = <f3d, win[r]> / sqrt(128) over the 25 window tokens -> softmax -> expectation and standard deviation on the normalised grid.
// Every wave holds features 32 ft .. 32 ft + 31 of its 32 tokens as a D[feature][token] tile (lane (r = token, h): register 4g + j = feature
// 8g + 4h + j); the 3D token's values sit in lanes 25 (h = 0) and 57 (h = 1): v_readlane hands them to every lane, a lane forms the partial
// dot product of ITS token over its 16 features, the two lane halves are added by v_permlane32_swap, and the four feature-tile waves'
// partials meet in LDS behind one barrier.  (Until round 4 one wave per match walked the staged f32 rows: 25 lanes x 32 dependent LDS
// reads + seven ds_bpermute butterflies = 6-8 k cycles of a 118 k-cycle workgroup, profiles/r04_stamps_fine_pair.txt "end".)
__device__ __forceinline__ float corr_partial(const f32x16& x, int lane) {
#pragma clang fp contract(off)
    float p0 = 0.f, p1 = 0.f;
#pragma unroll
    for (int reg = 0; reg < 16; ++reg) {
        const float xv = x[reg];                     // (a bit_cast applied to a vector ELEMENT reads element 0 on hipcc 7.2: copy first, as in tile_x3.h)
        const int xi = __builtin_bit_cast(int, xv);
        const float a0 = __builtin_bit_cast(float, __builtin_amdgcn_readlane(xi, TOK3D));
        const float a1 = __builtin_bit_cast(float, __builtin_amdgcn_readlane(xi, 32 + TOK3D));
        p0 = __builtin_fmaf(xv, a0, p0);
        p1 = __builtin_fmaf(xv, a1, p1);
    }
    return swap32_sum((lane >> 5) ? p1 : p0);
}
// `part`: the four waves' partials of this match's tokens, part[ft * pstride + r]
__device__ __forceinline__ void expect_store(const FineBArgs& p, int k, const float* part, int pstride, int lane) {
#pragma clang fp contract(off)
    float t = -INFINITY;
    if (lane < WIN) {
        const float dot = (part[lane] + part[pstride + lane]) + (part[2 * pstride + lane] + part[3 * pstride + lane]);
        t = dot * 0.08838834764831845f;              // 1 / sqrt(128)
    }
    const float m = wave_max_dpp(t);
    const float e = lane < WIN ? expf(t - m) : 0.f;
    const float sum = wave_sum_dpp(e);
    const float pr = e / sum;
    const float gx = (float)(lane % 5 - 2) * 0.5f, gy = (float)(lane / 5 - 2) * 0.5f;
    const float ex = wave_sum_dpp(pr * gx), ey = wave_sum_dpp(pr * gy);
    const float ex2 = wave_sum_dpp(pr * gx * gx), ey2 = wave_sum_dpp(pr * gy * gy);
    if (lane == 0) {
        const float vx = ex2 - ex * ex, vy = ey2 - ey * ey;
        const float sd = sqrtf(fmaxf(vx, 1e-10f)) + sqrtf(fmaxf(vy, 1e-10f));
        p.expec_f[3 * k] = ex; p.expec_f[3 * k + 1] = ey; p.expec_f[3 * k + 2] = sd;
        store_fine_keypoint(p, k, ex, ey);
    }
}

// f32 staging image [64][128], 16-byte chunks swizzled like the planes (32 chunks per row)
__device__ __forceinline__ int stage_off(int row, int chunk) { return row * (CF * 4) + ((chunk ^ (row & 15)) << 4); }

// LayerNorm over the 128 features of a token, spread over the 4 feature-tile waves of its match (wave (tt, ft) holds
// features 32 ft .. 32 ft + 31 of tokens 32 tt .. 32 tt + 31 as a D[feature][token] accumulator).  ONE workgroup barrier: every wave
// takes the two-pass moments of its own 32 features (sum, then squared deviations from ITS mean), the four (sum, M2) pairs cross waves
// through `scratch` ([2][4][64] floats) and are merged by Chan's formula -- the accuracy of the two-pass form without its second exchange.
__device__ __forceinline__ void ln_local_moments(const f32x16& m, float& s, float& q) {
#pragma clang fp contract(off)
    s = 0.f;
#pragma unroll
    for (int reg = 0; reg < 16; ++reg) s += m[reg];
    s += __shfl_xor(s, 32, 64);
    const float mw = s * (1.0f / 32.0f);
    q = 0.f;
#pragma unroll
    for (int reg = 0; reg < 16; ++reg) {
        const float d = m[reg] - mw;
        q = __builtin_fmaf(d, d, q);
    }
    q += __shfl_xor(q, 32, 64);
}
__device__ __forceinline__ float ln_apply(float x, float mean, float rstd, float g, float b) {
#pragma clang fp contract(off)
    return __builtin_fmaf((x - mean) * rstd, g, b);
}
// merged mean and 1 / sqrt(var + eps) of token `tok` from the four waves' (sum, M2) in scratch
__device__ __forceinline__ void ln_merge(const float* scratch, int tok, float& mean, float& rstd) {
#pragma clang fp contract(off)
    const float s0 = scratch[tok], s1 = scratch[64 + tok], s2 = scratch[128 + tok], s3 = scratch[192 + tok];
    mean = ((s0 + s1) + (s2 + s3)) * (1.0f / CF);
    const float e0 = __builtin_fmaf(s0, 1.0f / 32.0f, -mean), e1 = __builtin_fmaf(s1, 1.0f / 32.0f, -mean);
    const float e2 = __builtin_fmaf(s2, 1.0f / 32.0f, -mean), e3 = __builtin_fmaf(s3, 1.0f / 32.0f, -mean);
    const float dev2 = __builtin_fmaf(e0, e0, e1 * e1) + __builtin_fmaf(e2, e2, e3 * e3);
    const float m2 = __builtin_fmaf(32.0f, dev2, (scratch[256 + tok] + scratch[320 + tok]) + (scratch[384 + tok] + scratch[448 + tok]));
    rstd = 1.0f / sqrtf(__builtin_fmaf(m2, 1.0f / CF, 1e-5f));
}
__device__ __forceinline__ void layernorm_featrow128(f32x16& m, const float* __restrict__ gamma, const float* __restrict__ beta,
                                                     float* scratch, int ft, int tt, int lane) {
    const int r = lane & 31, h = lane >> 5;
    const int tok = 32 * tt + r;
    float s, q;
    ln_local_moments(m, s, q);
    if (h == 0) { scratch[ft * 64 + tok] = s; scratch[256 + ft * 64 + tok] = q; }
    __syncthreads();
    float mean, rstd;
    ln_merge(scratch, tok, mean, rstd);
#pragma unroll
    for (int g = 0; g < 4; ++g) {
        const int f0 = 32 * ft + 8 * g + 4 * h;
        const f32x4 gv = *reinterpret_cast<const f32x4*>(gamma + f0);
        const f32x4 bv = *reinterpret_cast<const f32x4*>(beta + f0);
#pragma unroll
        for (int j = 0; j < 4; ++j) m[4 * g + j] = ln_apply(m[4 * g + j], mean, rstd, gv[j], bv[j]);
    }
}

// NM = matches per workgroup (1: 4 waves, 64 KiB LDS in split mode, two independent workgroups per CU; 2: 8 waves)
template <int NS, int NM>
__global__ __launch_bounds__(NM * 256) OPHIP_WAVES_PER_SIMD(2, 2) void fine_refine_bf16_kernel(FineBArgs p) {
    extern __shared__ __attribute__((aligned(16))) char smem[];
    constexpr int PL = NS == 3 ? 2 : 1;
    constexpr int TOK = 32 * NM, NT_ = 256 * NM;
    constexpr int XB = TOK * ROWB, HB = TOK * HROWB;   // per plane
    char* XH = smem;
    char* XL = smem + (PL - 1) * XB;
    char* YH = smem + PL * XB;
    char* YL = YH + (PL - 1) * XB;
    char* HH = smem + 2 * PL * XB;
    char* HL = HH + (PL - 1) * HB;
    // f32 staging [64][128] (32 KiB) and the LayerNorm exchange live in H while it is idle.
    // LDS total: split 32 + 32 + 64 = 128 KiB, plain 64 KiB.
    char* stage = HH;
    float* scratch = reinterpret_cast<float*>(HH);
    const int k0 = NM * blockIdx.x;
    const int total = min(*p.count, p.cap);           // a count above the lists' capacity refines the capacity's worth of matches
    if (k0 >= total) return;
    // waves: wave = 4 * tt + ft owns feature tile ft (features 32 ft .. 32 ft + 31) of match / token tile tt
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const int ft = wave & 3, tt = wave >> 2;
    const int r = lane & 31, h = lane >> 5;
    OPHIP_STAMP(p.stamps, blockIdx.x, 0);

    const int nl = p.enc_enable ? p.nlayers : 0;
    constexpr size_t LAYER_BYTES = (size_t)2 * W_ELEMS * 2 + 4 * CF * 4;
    // plane offsets in fragments: Wq | Wkv (per feature tile: K tile, V tile) | Wm | W0 | W2
    constexpr int OQ = 0, OKV = CF * CF / 8, OM = 3 * CF * CF / 8, O0 = 4 * CF * CF / 8, O2 = 8 * CF * CF / 8;
    // the first layer's Q / K|V weight fragments do not depend on the match: they travel under the gather below
    WRing<1, 2, NS> rq;
    WRing<2, 2, NS> rkv;
    if (nl > 0) {
        const bf16x8* w_hi = reinterpret_cast<const bf16x8*>(p.wpack);
        const bf16x8* w_lo = w_hi + W_ELEMS / 8;
        rq.fill(w_hi + OQ + (size_t)ft * TS + lane, w_lo + OQ + (size_t)ft * TS + lane, TS);
        rkv.fill(w_hi + OKV + (size_t)(2 * ft) * TS + lane, w_lo + OKV + (size_t)(2 * ft) * TS + lane, TS);
    }

    // ---- gather both matches into the f32 staging image --------------------------------------------
    // every load of both matches is issued before the first LDS write, so their latencies overlap
    // (named scalars + selects: a runtime-indexed array would live in scratch)
    const bool live0 = k0 < total, live1 = NM > 1 && k0 + 1 < total;
    const int b0 = (int)p.b_ids[k0], i30 = (int)p.i_ids[k0], j0 = (int)p.j_ids[k0];
    const int b1 = live1 ? (int)p.b_ids[k0 + 1] : 0, i31 = live1 ? (int)p.i_ids[k0 + 1] : 0, j1 = live1 ? (int)p.j_ids[k0 + 1] : 0;
    const int cy0 = p.stride * (j0 / p.wc), cx0 = p.stride * (j0 % p.wc);
    const int cy1 = p.stride * (j1 / p.wc), cx1 = p.stride * (j1 % p.wc);
#define MLIVE(mi) ((mi) ? live1 : live0)
#define MB(mi) ((mi) ? b1 : b0)
#define MI3(mi) ((mi) ? i31 : i30)
#define MCY(mi) ((mi) ? cy1 : cy0)
#define MCX(mi) ((mi) ? cx1 : cx0)
    if (p.fs_c == 1) {                   // channels-last: 512 B contiguous per pixel; 2 x 25 x 128 elements / 512 threads
        constexpr int NQ = NM * WIN * (CF / 4), PER = (NQ + NT_ - 1) / NT_;      // float4 items: (match, window row, 4 channels)
        f32x4 v[PER];
#pragma unroll
        for (int u = 0; u < PER; ++u) {
            const int e = tid + NT_ * u;
            v[u] = f32x4{0.f, 0.f, 0.f, 0.f};
            if (e < NQ) {
                const int mi = e / (WIN * (CF / 4)), e2 = e % (WIN * (CF / 4)), rr = e2 >> 5, c4 = e2 & 31;
                const int y = MCY(mi) + rr / 5 - 2, x = MCX(mi) + rr % 5 - 2;
                if (MLIVE(mi) && y >= 0 && y < p.hf && x >= 0 && x < p.wf)
                    v[u] = *reinterpret_cast<const f32x4*>(p.feat_f + (size_t)MB(mi) * p.fs_b + (size_t)y * p.fs_y + (size_t)x * p.fs_x + 4 * c4);
            }
        }
#pragma unroll
        for (int u = 0; u < PER; ++u) {
            const int e = tid + NT_ * u;
            if (e < NQ) {
                const int mi = e / (WIN * (CF / 4)), e2 = e % (WIN * (CF / 4)), rr = e2 >> 5, c4 = e2 & 31;
                *reinterpret_cast<f32x4*>(stage + stage_off(32 * mi + rr, c4)) = v[u];
            }
        }
    } else {                             // NCHW: one (match, channel, window row) run of 5 consecutive x per slot
        constexpr int RUNS = NM * CF * 5, PER = (RUNS + NT_ - 1) / NT_;
        float v[PER][5];
#pragma unroll
        for (int u = 0; u < PER; ++u) {
            const int q = tid + NT_ * u;
            const int mi = q / (CF * 5), q2 = q % (CF * 5), c = q2 / 5, ky = q2 % 5;
            const bool ok = q < RUNS && MLIVE(mi);
            const int m2 = mi < 2 ? mi : 0;
            const int y = MCY(m2) + ky - 2;
            const bool yin = ok && y >= 0 && y < p.hf;
            const float* src = p.feat_f + (size_t)MB(m2) * p.fs_b + (size_t)c * p.fs_c + (size_t)(yin ? y : 0) * p.fs_y;
#pragma unroll
            for (int kx = 0; kx < 5; ++kx) {
                const int x = MCX(m2) + kx - 2;
                v[u][kx] = (yin && x >= 0 && x < p.wf) ? src[(size_t)x * p.fs_x] : 0.f;
            }
        }
#pragma unroll
        for (int u = 0; u < PER; ++u) {
            const int q = tid + NT_ * u;
            if (q < RUNS) {
                const int mi = q / (CF * 5), q2 = q % (CF * 5), c = q2 / 5, ky = q2 % 5;
#pragma unroll
                for (int kx = 0; kx < 5; ++kx)
                    *reinterpret_cast<float*>(stage + stage_off(32 * mi + ky * 5 + kx, c >> 2) + 4 * (c & 3)) = v[u][kx];
            }
        }
    }
    if (tid < NM * CF) {                 // the 3D fine descriptor (row 25) of every match
        const int mi = tid >> 7, c = tid & 127;
        const float v = MLIVE(mi) ? p.desc_f[(size_t)MB(mi) * p.ds_b + (size_t)c * p.ds_c + MI3(mi)] : 0.f;
        *reinterpret_cast<float*>(stage + stage_off(32 * mi + TOK3D, c >> 2) + 4 * (c & 3)) = v;
    }
    for (int e = tid; e < NM * 6 * CF; e += NT_) {      // padding rows 26..31
        const int mi = e / (6 * CF), e2 = e % (6 * CF), rr = 26 + (e2 >> 7), c = e2 & 127;
        *reinterpret_cast<float*>(stage + stage_off(32 * mi + rr, c >> 2) + 4 * (c & 3)) = 0.f;
    }
    __syncthreads();
    OPHIP_STAMP(p.stamps, blockIdx.x, 1);
    // residual stream in registers, D[feature][token] layout: this wave's 32 features of its 32 tokens
    f32x16 xres;
#pragma unroll
    for (int g = 0; g < 4; ++g) {
        const f32x4 v = *reinterpret_cast<const f32x4*>(stage + stage_off(32 * tt + r, 8 * ft + 2 * g + h));
#pragma unroll
        for (int j = 0; j < 4; ++j) xres[4 * g + j] = v[j];
    }
    __syncthreads();                                 // staging (in H) fully consumed before anything else lands there
    store_featrow_acc<NS>(xres, XH, XL, ROWB, 32 * ft, 32 * tt, lane);
    __syncthreads();

    // this wave's token rows inside the planes
    const char* xh = XH + 32 * tt * ROWB; const char* xl = XL + 32 * tt * ROWB;
    const char* yh = YH + 32 * tt * ROWB; const char* yl = YL + 32 * tt * ROWB;
    const char* hh = HH + 32 * tt * HROWB; const char* hl = HL + 32 * tt * HROWB;

    for (int l = 0; l < nl; ++l) {
        const char* wl = p.wpack + (size_t)l * LAYER_BYTES;
        const bf16x8* w_hi = reinterpret_cast<const bf16x8*>(wl);
        const bf16x8* w_lo = w_hi + W_ELEMS / 8;
        const float* ln = reinterpret_cast<const float*>(wl + (size_t)2 * W_ELEMS * 2);
        const bool cross = (p.cross_bits >> l) & 1u;

        // ---- phase 1: Q (D[feature][token]) and K, V (D[token][feature]) of this wave's match from X ----------
        f32x16 q[1][1] = {{zero16()}};
        f32x16 kv_[2][1] = {{zero16()}, {zero16()}};
        gemm_bf16_ring<1, 1, NS, true, KB, 2>(q, rq, w_hi + OQ + (size_t)ft * TS + lane, w_lo + OQ + (size_t)ft * TS + lane, TS, xh, xl, ROWB, 0, lane);
        gemm_bf16_ring<2, 1, NS, false, KB, 2>(kv_, rkv, w_hi + OKV + (size_t)(2 * ft) * TS + lane, w_lo + OKV + (size_t)(2 * ft) * TS + lane, TS,
                                               xh, xl, ROWB, 0, lane);
        OPHIP_STAMP(p.stamps, blockIdx.x, 2 + 8 * l);
        WRing<1, 2, NS> rm;                      // merge weights: in flight during the register-only attention below
        rm.fill(w_hi + OM + (size_t)ft * TS + lane, w_lo + OM + (size_t)ft * TS + lane, TS);
        // ---- KV / Ksum of the window set, the 3D token's rank-one message, phi(Q) KV: all in registers (attend_match) ------
        {
            f32x16 num = attend_match<NS>(q[0][0], kv_[0][0], kv_[1][0], cross, scratch + 96 * (4 * tt + ft), lane);
            store_featrow_acc<NS>(num, YH, YL, ROWB, 32 * ft, 32 * tt, lane);
        }
        __syncthreads();
        OPHIP_STAMP(p.stamps, blockIdx.x, 3 + 8 * l);
        // ---- phase 2: merge + LN1 -> Y -----------------------------------------------------------------
        WRing<2, 2, NS> r0;                      // MLP-up weights (hidden tiles 2 ft, 2 ft + 1)
        {
            f32x16 m[1][1] = {{zero16()}};
            gemm_bf16_ring<1, 1, NS, true, KB, 2>(m, rm, w_hi + OM + (size_t)ft * TS + lane, w_lo + OM + (size_t)ft * TS + lane, TS, yh, yl, ROWB, 0, lane);
            r0.fill(w_hi + O0 + (size_t)(2 * ft) * TS2 + lane, w_lo + O0 + (size_t)(2 * ft) * TS2 + lane, TS2);
            OPHIP_STAMP(p.stamps, blockIdx.x, 4 + 8 * l);
            layernorm_featrow128(m[0][0], ln, ln + CF, scratch, ft, tt, lane);       // first barrier also fences the reads of Y
            store_featrow_acc<NS>(m[0][0], YH, YL, ROWB, 32 * ft, 32 * tt, lane);
        }
        __syncthreads();
        OPHIP_STAMP(p.stamps, blockIdx.x, 5 + 8 * l);
        // ---- phase 3: hidden = relu([x, msg] W0^T) -> H (256 features) ---------------------------------------
        WRing<1, 2, NS> r2;
        {
            f32x16 hd[2][1] = {{zero16()}, {zero16()}};
            gemm_bf16_ring_cat<2, 1, NS, KB2, 2>(hd, r0, w_hi + O0 + (size_t)(2 * ft) * TS2 + lane, w_lo + O0 + (size_t)(2 * ft) * TS2 + lane, TS2,
                                                 xh, xl, yh, yl, ROWB, lane);
            r2.fill(w_hi + O2 + (size_t)ft * TS2 + lane, w_lo + O2 + (size_t)ft * TS2 + lane, TS2);
            OPHIP_STAMP(p.stamps, blockIdx.x, 6 + 8 * l);
#pragma unroll
            for (int t = 0; t < 2; ++t) {
#pragma unroll
                for (int reg = 0; reg < 16; ++reg) hd[t][0][reg] = fmaxf(hd[t][0][reg], 0.f);
                store_featrow_acc<NS>(hd[t][0], HH, HL, HROWB, 64 * ft + 32 * t, 32 * tt, lane);
            }
        }
        __syncthreads();
        OPHIP_STAMP(p.stamps, blockIdx.x, 7 + 8 * l);
        // ---- phase 4: o = hidden W2^T, LN2, residual ------------------------------------------------------
        f32x16 o[1][1] = {{zero16()}};
        gemm_bf16_ring<1, 1, NS, true, KB2, 2>(o, r2, w_hi + O2 + (size_t)ft * TS2 + lane, w_lo + O2 + (size_t)ft * TS2 + lane, TS2, hh, hl, HROWB, 0, lane);
        OPHIP_STAMP(p.stamps, blockIdx.x, 8 + 8 * l);
        if (l + 1 < nl) {                        // next layer's first weights travel during LN2 and the plane rewrite
            const bf16x8* n_hi = reinterpret_cast<const bf16x8*>(wl + LAYER_BYTES);
            const bf16x8* n_lo = n_hi + W_ELEMS / 8;
            rq.fill(n_hi + OQ + (size_t)ft * TS + lane, n_lo + OQ + (size_t)ft * TS + lane, TS);
            rkv.fill(n_hi + OKV + (size_t)(2 * ft) * TS + lane, n_lo + OKV + (size_t)(2 * ft) * TS + lane, TS);
        }
        __syncthreads();                         // every wave is done reading H before the LayerNorm exchange reuses it
        layernorm_featrow128(o[0][0], ln + 2 * CF, ln + 3 * CF, scratch, ft, tt, lane);
#pragma unroll
        for (int reg = 0; reg < 16; ++reg) xres[reg] += o[0][0][reg];
        store_featrow_acc<NS>(xres, XH, XL, ROWB, 32 * ft, 32 * tt, lane);
        __syncthreads();
        OPHIP_STAMP(p.stamps, blockIdx.x, 9 + 8 * l);
    }

    // ---- correlation -> softmax -> expectation from the residual registers (the f32 staging image only for the debug outputs) ----------
    if (p.dbg_win) {
#pragma unroll
        for (int g = 0; g < 4; ++g) {
            f32x4 v = {xres[4 * g], xres[4 * g + 1], xres[4 * g + 2], xres[4 * g + 3]};
            *reinterpret_cast<f32x4*>(stage + stage_off(32 * tt + r, 8 * ft + 2 * g + h)) = v;
        }
        __syncthreads();
        for (int mi = 0; mi < NM; ++mi) {
            const int k = k0 + mi;
            if (k >= total) break;
            for (int e = tid; e < WIN * CF; e += NT_) {
                const int rr = e >> 7, c = e & 127;
                p.dbg_win[(size_t)k * WIN * CF + e] = *reinterpret_cast<const float*>(stage + stage_off(32 * mi + rr, c >> 2) + 4 * (c & 3));
            }
            if (tid < CF) p.dbg_f3[(size_t)k * CF + tid] = *reinterpret_cast<const float*>(stage + stage_off(32 * mi + TOK3D, tid >> 2) + 4 * (tid & 3));
        }
        __syncthreads();                             // the partials below share the staging image's LDS
    }
    {
        const float pp = corr_partial(xres, lane);
        if (h == 0) scratch[ft * (32 * NM) + 32 * tt + r] = pp;
    }
    __syncthreads();
    if (ft == 0 && k0 + tt < total) expect_store(p, k0 + tt, scratch + 32 * tt, 32 * NM, lane);
    OPHIP_STAMP(p.stamps, blockIdx.x, 31);
}

// a copy of v the compiler cannot see through: what is computed from it stays where it is used instead of joining the caller's
// loop invariants (and their live ranges)
__device__ __forceinline__ int opaque(int v) {
    asm volatile("" : "+v"(v));
    return v;
}

// LayerNorm over the 128 features of the tokens of BOTH matches of a pair workgroup (wave ft holds features 32 ft .. 32 ft + 31
// of tokens 0 .. 63 as two D[feature][token] accumulators).  Same arithmetic as layernorm_featrow128 (the two kernels stay
// bit-identical), `scratch` = [2][4][64] floats of its own.  1 barrier.
__device__ __forceinline__ void layernorm_pair(f32x16 (&m)[1][2], const float* __restrict__ gamma, const float* __restrict__ beta,
                                               float* scratch, int ft, int lane) {
    const int r = lane & 31, h = lane >> 5;
#pragma unroll
    for (int tt = 0; tt < 2; ++tt) {
        float s, q;
        ln_local_moments(m[0][tt], s, q);
        if (h == 0) { scratch[ft * 64 + 32 * tt + r] = s; scratch[256 + ft * 64 + 32 * tt + r] = q; }
    }
    __syncthreads();
    f32x4 gv[4], bv[4];
#pragma unroll
    for (int g = 0; g < 4; ++g) {
        const int f0 = 32 * ft + 8 * g + 4 * h;
        gv[g] = *reinterpret_cast<const f32x4*>(gamma + f0);
        bv[g] = *reinterpret_cast<const f32x4*>(beta + f0);
    }
#pragma unroll
    for (int tt = 0; tt < 2; ++tt) {
        float mean, rstd;
        ln_merge(scratch, 32 * tt + r, mean, rstd);
#pragma unroll
        for (int g = 0; g < 4; ++g)
#pragma unroll
            for (int j = 0; j < 4; ++j) m[0][tt][4 * g + j] = ln_apply(m[0][tt][4 * g + j], mean, rstd, gv[g][j], bv[g][j]);
    }
}

// TWO matches per 4-wave workgroup, sharing every weight fragment: wave ft owns feature tile ft of BOTH matches (token tiles
// tt = 0, 1 of 64-row planes), so a fragment pulled from L2 feeds two matrix instructions and the layers' 1.3 MB of (hi, lo)
// weights cross the L2 -> CU path once per two matches (one-match workgroups: 3.9 GB of L2 reads per frame at K = 2 975, which is
// what bounded the stage, profiles/r03_fine_*).  LDS stays at 66 KiB per workgroup -- two workgroups per CU as before -- because the
// hidden planes OVERLAY the X and Y planes: relu(hidden) is held in registers until every wave is done reading [x, msg], then
// written over them; the residual stream lives in f32 registers, the next layer's X planes are rewritten from it.
//   LDS map: [X hi | X lo] 32 KiB, [Y hi | Y lo] 32 KiB (= hidden planes 64 KiB; f32 staging image in the Y half), 2 KiB LayerNorm scratch
template <int NS>
__global__ __launch_bounds__(256) OPHIP_WAVES_PER_SIMD(2, 2) void fine_pair_kernel(FineBArgs p) {
    extern __shared__ __attribute__((aligned(16))) char smem[];
    constexpr int PL = NS == 3 ? 2 : 1;
    constexpr int TOK = 64, NT_ = 256;
    constexpr int XB = TOK * ROWB, HB = TOK * HROWB;   // per plane: 16 KiB, 32 KiB
    // (the same 66 KiB map in plain-bf16 mode, whose lo planes stay unused: the f32 staging image needs its 32 KiB either way)
    char* XH = smem;
    char* XL = smem + XB;
    char* YH = smem + 2 * XB;
    char* YL = YH + XB;
    char* HH = smem;                                    // overlays X and Y
    char* HL = HH + HB;
    char* stage = YH;                                   // f32 [64][128] = 32 KiB: the Y half, while Y is idle
    float* scratch = reinterpret_cast<float*>(smem + 4 * XB);
    static_assert(PL == 1 || PL == 2, "one or two planes");
    const int k0 = 2 * blockIdx.x;
    // the ids of both matches travel WITH the count (the lists are capacity-sized and the grid covers the capacity, so the reads are in
    // bounds whatever the count turns out to be): one round trip to memory in front of the gather instead of two
    const bool in1 = k0 + 1 < p.cap;
    const int b0 = (int)p.b_ids[k0], i30 = (int)p.i_ids[k0], j0 = (int)p.j_ids[k0];
    const int b1_ = in1 ? (int)p.b_ids[k0 + 1] : 0, i31_ = in1 ? (int)p.i_ids[k0 + 1] : 0, j1_ = in1 ? (int)p.j_ids[k0 + 1] : 0;
    // clamped to the capacity: with an odd capacity and a count above it, row `cap` would otherwise be the live second match of the last
    // workgroup and expec_f / mkpts_f / the debug rows would be written one row past the buffers
    const int total = min(*p.count, p.cap);
    if (k0 >= total) return;
    const int tid = threadIdx.x, lane = tid & 63, ft = tid >> 6;
    const int r = lane & 31, h = lane >> 5;
    if (p.stagger > 0 && (int)blockIdx.x >= p.ncu && (int)blockIdx.x < 2 * p.ncu)
        for (int i = 0; i < p.stagger; ++i) __builtin_amdgcn_s_sleep(64);
    OPHIP_STAMP(p.stamps, blockIdx.x, 0);

    const int nl = p.enc_enable ? p.nlayers : 0;
    constexpr size_t LAYER_BYTES = (size_t)2 * W_ELEMS * 2 + 4 * CF * 4;
    constexpr int OQ = 0, OKV = CF * CF / 8, OM = 3 * CF * CF / 8, O0 = 4 * CF * CF / 8, O2 = 8 * CF * CF / 8;
    WRing<1, 2, NS> rq;
    WRing<2, 2, NS> rkv;
    if (nl > 0) {
        const bf16x8* w_hi = reinterpret_cast<const bf16x8*>(p.wpack);
        const bf16x8* w_lo = w_hi + W_ELEMS / 8;
        rq.fill(w_hi + OQ + (size_t)ft * TS + lane, w_lo + OQ + (size_t)ft * TS + lane, TS);
    }

    // ---- gather both matches into the f32 staging image (all loads issued before the first LDS write) -------------------
    const bool live1 = k0 + 1 < total;
    const int b1 = live1 ? b1_ : 0, i31 = live1 ? i31_ : 0, j1 = live1 ? j1_ : 0;
    const int cy0 = p.stride * (j0 / p.wc), cx0 = p.stride * (j0 % p.wc);
    const int cy1 = p.stride * (j1 / p.wc), cx1 = p.stride * (j1 % p.wc);
#define PLIVE(mi) ((mi) ? live1 : true)
#define PB(mi) ((mi) ? b1 : b0)
#define PI3(mi) ((mi) ? i31 : i30)
#define PCY(mi) ((mi) ? cy1 : cy0)
#define PCX(mi) ((mi) ? cx1 : cx0)
    if (p.fs_c == 1) {
        constexpr int NQ = 2 * WIN * (CF / 4), PER = (NQ + NT_ - 1) / NT_;
        f32x4 v[PER];
#pragma unroll
        for (int u = 0; u < PER; ++u) {
            const int e = tid + NT_ * u;
            v[u] = f32x4{0.f, 0.f, 0.f, 0.f};
            if (e < NQ) {
                const int mi = e / (WIN * (CF / 4)), e2 = e % (WIN * (CF / 4)), rr = e2 >> 5, c4 = e2 & 31;
                const int y = PCY(mi) + rr / 5 - 2, x = PCX(mi) + rr % 5 - 2;
                if (PLIVE(mi) && y >= 0 && y < p.hf && x >= 0 && x < p.wf)
                    v[u] = *reinterpret_cast<const f32x4*>(p.feat_f + (size_t)PB(mi) * p.fs_b + (size_t)y * p.fs_y + (size_t)x * p.fs_x + 4 * c4);
            }
        }
#pragma unroll
        for (int u = 0; u < PER; ++u) {
            const int e = tid + NT_ * u;
            if (e < NQ) {
                const int mi = e / (WIN * (CF / 4)), e2 = e % (WIN * (CF / 4)), rr = e2 >> 5, c4 = e2 & 31;
                *reinterpret_cast<f32x4*>(stage + stage_off(32 * mi + rr, c4)) = v[u];
            }
        }
    } else {
        constexpr int RUNS = 2 * CF * 5, PER = (RUNS + NT_ - 1) / NT_;
        float v[PER][5];
#pragma unroll
        for (int u = 0; u < PER; ++u) {
            const int q = tid + NT_ * u;
            const int mi = q / (CF * 5), q2 = q % (CF * 5), c = q2 / 5, ky = q2 % 5;
            const bool ok = q < RUNS && PLIVE(mi);
            const int y = PCY(mi) + ky - 2;
            const bool yin = ok && y >= 0 && y < p.hf;
            const float* src = p.feat_f + (size_t)PB(mi) * p.fs_b + (size_t)c * p.fs_c + (size_t)(yin ? y : 0) * p.fs_y;
#pragma unroll
            for (int kx = 0; kx < 5; ++kx) {
                const int x = PCX(mi) + kx - 2;
                v[u][kx] = (yin && x >= 0 && x < p.wf) ? src[(size_t)x * p.fs_x] : 0.f;
            }
        }
#pragma unroll
        for (int u = 0; u < PER; ++u) {
            const int q = tid + NT_ * u;
            if (q < RUNS) {
                const int mi = q / (CF * 5), q2 = q % (CF * 5), c = q2 / 5, ky = q2 % 5;
#pragma unroll
                for (int kx = 0; kx < 5; ++kx)
                    *reinterpret_cast<float*>(stage + stage_off(32 * mi + ky * 5 + kx, c >> 2) + 4 * (c & 3)) = v[u][kx];
            }
        }
    }
    {                                   // the 3D fine descriptor (row 25) of both matches: 2 x 128 values = one per thread
        const int mi = tid >> 7, c = tid & 127;
        const float v = PLIVE(mi) ? p.desc_f[(size_t)PB(mi) * p.ds_b + (size_t)c * p.ds_c + PI3(mi)] : 0.f;
        *reinterpret_cast<float*>(stage + stage_off(32 * mi + TOK3D, c >> 2) + 4 * (c & 3)) = v;
    }
    for (int e = tid; e < 2 * 6 * CF; e += NT_) {       // padding rows 26..31
        const int mi = e / (6 * CF), e2 = e % (6 * CF), rr = 26 + (e2 >> 7), c = e2 & 127;
        *reinterpret_cast<float*>(stage + stage_off(32 * mi + rr, c >> 2) + 4 * (c & 3)) = 0.f;
    }
#undef PLIVE
#undef PB
#undef PI3
#undef PCY
#undef PCX
    __syncthreads();
    OPHIP_STAMP(p.stamps, blockIdx.x, 1);
    // residual stream in registers, D[feature][token] layout: this wave's 32 features of the 32 tokens of each match
    f32x16 xres[2];
#pragma unroll
    for (int tt = 0; tt < 2; ++tt)
#pragma unroll
        for (int g = 0; g < 4; ++g) {
            const f32x4 v = *reinterpret_cast<const f32x4*>(stage + stage_off(32 * tt + r, 8 * ft + 2 * g + h));
#pragma unroll
            for (int j = 0; j < 4; ++j) xres[tt][4 * g + j] = v[j];
        }
#pragma unroll
    for (int tt = 0; tt < 2; ++tt) store_featrow_acc<NS>(xres[tt], XH, XL, ROWB, 32 * ft, 32 * tt, lane);      // X region: disjoint from the staging image
    __syncthreads();


    for (int l = 0; l < nl; ++l) {
        const char* wl = p.wpack + (size_t)l * LAYER_BYTES;
        const bf16x8* w_hi = reinterpret_cast<const bf16x8*>(wl);
        const bf16x8* w_lo = w_hi + W_ELEMS / 8;
        const float* ln = reinterpret_cast<const float*>(wl + (size_t)2 * W_ELEMS * 2);
        const bool cross = (p.cross_bits >> l) & 1u;

        // ---- phase 1: Q (D[feature][token]) of both matches from X with shared weight fragments; K, V (D[token][feature]) one
        //      match at a time (their accumulators + the attention block's tiles of two matches at once do not fit 256 registers:
        //      87 spilled; the K|V fifth of the weights is therefore read once per match, the other four fifths once per pair) ----
        // (per-lane weight pointers are formed from an opaque copy of the lane index phase by phase: as loop invariants of the layer loop
        //  they would all stay live across the whole layer)
        f32x16 q[1][2] = {{zero16(), zero16()}};
        {
            const int ln_ = opaque(lane);
            rkv.fill(w_hi + OKV + (size_t)(2 * ft) * TS + ln_, w_lo + OKV + (size_t)(2 * ft) * TS + ln_, TS);      // travels under the Q GEMM
            gemm_bf16_ring<1, 2, NS, true, KB, 2>(q, rq, w_hi + OQ + (size_t)ft * TS + ln_, w_lo + OQ + (size_t)ft * TS + ln_, TS, XH, XL, ROWB, 0, lane);
        }
        OPHIP_STAMP(p.stamps, blockIdx.x, 2 + 8 * l);
        // ---- per match: K|V projection, then the attention in registers (attend_match) ---------------------------------------
#pragma unroll
        for (int tt = 0; tt < 2; ++tt) {
            f32x16 kv_[2][1] = {{zero16()}, {zero16()}};
            const int lk_ = opaque(lane);
            gemm_bf16_ring<2, 1, NS, false, KB, 2>(kv_, rkv, w_hi + OKV + (size_t)(2 * ft) * TS + lk_, w_lo + OKV + (size_t)(2 * ft) * TS + lk_, TS,
                                                   XH + 32 * tt * ROWB, XL + 32 * tt * ROWB, ROWB, 0, lane);
            OPHIP_FINE_SCHED_FENCE();
            f32x16 num = attend_match<NS>(q[0][tt], kv_[0][0], kv_[1][0], cross, scratch + 96 * ft, lane);
            store_featrow_acc<NS>(num, YH, YL, ROWB, 32 * ft, 32 * tt, lane);
            OPHIP_FINE_SCHED_FENCE();
            if (tt == 0) rkv.fill(w_hi + OKV + (size_t)(2 * ft) * TS + lk_, w_lo + OKV + (size_t)(2 * ft) * TS + lk_, TS);      // the second match's K|V weights
        }
        WRing<1, 2, NS> rm;                      // merge weights travel under the barrier
        const int lm_ = opaque(lane);
        rm.fill(w_hi + OM + (size_t)ft * TS + lm_, w_lo + OM + (size_t)ft * TS + lm_, TS);
        __syncthreads();
        OPHIP_STAMP(p.stamps, blockIdx.x, 3 + 8 * l);
        // ---- phase 2: merge + LN1 -> Y -----------------------------------------------------------------
        WRing<2, 2, NS> r0;                      // MLP-up weights (hidden tiles 2 ft, 2 ft + 1)
        {
            f32x16 m[1][2] = {{zero16(), zero16()}};
            gemm_bf16_ring<1, 2, NS, true, KB, 2>(m, rm, w_hi + OM + (size_t)ft * TS + lm_, w_lo + OM + (size_t)ft * TS + lm_, TS, YH, YL, ROWB, 0, lane);
            const int l0_ = opaque(lane);
            r0.fill(w_hi + O0 + (size_t)(2 * ft) * TS2 + l0_, w_lo + O0 + (size_t)(2 * ft) * TS2 + l0_, TS2);
            OPHIP_STAMP(p.stamps, blockIdx.x, 4 + 8 * l);
            layernorm_pair(m, ln, ln + CF, scratch, ft, lane);           // its first barrier also fences the reads of Y above
#pragma unroll
            for (int tt = 0; tt < 2; ++tt) store_featrow_acc<NS>(m[0][tt], YH, YL, ROWB, 32 * ft, 32 * tt, lane);
        }
        __syncthreads();
        OPHIP_STAMP(p.stamps, blockIdx.x, 5 + 8 * l);
        // ---- phase 3: hidden = relu([x, msg] W0^T), kept in registers until every wave has read X and Y, then written OVER them ----
        WRing<1, 2, NS> r2;
        {
            f32x16 hd[2][2] = {{zero16(), zero16()}, {zero16(), zero16()}};
            const int l0_ = opaque(lane);
            gemm_bf16_ring_cat<2, 2, NS, KB2, 2>(hd, r0, w_hi + O0 + (size_t)(2 * ft) * TS2 + l0_, w_lo + O0 + (size_t)(2 * ft) * TS2 + l0_, TS2,
                                                 XH, XL, YH, YL, ROWB, lane);
            r2.fill(w_hi + O2 + (size_t)ft * TS2 + l0_, w_lo + O2 + (size_t)ft * TS2 + l0_, TS2);
            OPHIP_STAMP(p.stamps, blockIdx.x, 6 + 8 * l);
            __syncthreads();                         // X and Y are dead from here to the end of the layer
#pragma unroll
            for (int t = 0; t < 2; ++t)
#pragma unroll
                for (int tt = 0; tt < 2; ++tt) {
#pragma unroll
                    for (int reg = 0; reg < 16; ++reg) hd[t][tt][reg] = fmaxf(hd[t][tt][reg], 0.f);
                    store_featrow_acc<NS>(hd[t][tt], HH, HL, HROWB, 64 * ft + 32 * t, 32 * tt, lane);
                }
        }
        __syncthreads();
        OPHIP_STAMP(p.stamps, blockIdx.x, 7 + 8 * l);
        // ---- phase 4: o = hidden W2^T, LN2, residual ------------------------------------------------------
        f32x16 o[1][2] = {{zero16(), zero16()}};
        {
            const int l2_ = opaque(lane);
            gemm_bf16_ring<1, 2, NS, true, KB2, 2>(o, r2, w_hi + O2 + (size_t)ft * TS2 + l2_, w_lo + O2 + (size_t)ft * TS2 + l2_, TS2, HH, HL, HROWB, 0, lane);
        }
        OPHIP_STAMP(p.stamps, blockIdx.x, 8 + 8 * l);
        if (l + 1 < nl) {                        // next layer's first weights travel during LN2 and the plane rewrite
            const bf16x8* n_hi = reinterpret_cast<const bf16x8*>(wl + LAYER_BYTES);
            const bf16x8* n_lo = n_hi + W_ELEMS / 8;
            const int ln_ = opaque(lane);
            rq.fill(n_hi + OQ + (size_t)ft * TS + ln_, n_lo + OQ + (size_t)ft * TS + ln_, TS);
        }
        layernorm_pair(o, ln + 2 * CF, ln + 3 * CF, scratch, ft, lane);  // its first barrier: every wave is done reading the hidden planes
#pragma unroll
        for (int tt = 0; tt < 2; ++tt) {
#pragma unroll
            for (int reg = 0; reg < 16; ++reg) xres[tt][reg] += o[0][tt][reg];
            if (l + 1 < nl) store_featrow_acc<NS>(xres[tt], XH, XL, ROWB, 32 * ft, 32 * tt, lane);
        }
        __syncthreads();
        OPHIP_STAMP(p.stamps, blockIdx.x, 9 + 8 * l);
    }

    // ---- correlation -> softmax -> expectation from the residual registers (the f32 staging image only for the debug outputs) ----------
    if (p.dbg_win) {
#pragma unroll
        for (int tt = 0; tt < 2; ++tt)
#pragma unroll
            for (int g = 0; g < 4; ++g) {
                f32x4 v = {xres[tt][4 * g], xres[tt][4 * g + 1], xres[tt][4 * g + 2], xres[tt][4 * g + 3]};
                *reinterpret_cast<f32x4*>(stage + stage_off(32 * tt + r, 8 * ft + 2 * g + h)) = v;
            }
        __syncthreads();
        for (int mi = 0; mi < 2; ++mi) {
            const int k = k0 + mi;
            if (k >= total) break;
            for (int e = tid; e < WIN * CF; e += NT_) {
                const int rr = e >> 7, c = e & 127;
                p.dbg_win[(size_t)k * WIN * CF + e] = *reinterpret_cast<const float*>(stage + stage_off(32 * mi + rr, c >> 2) + 4 * (c & 3));
            }
            if (tid < CF) p.dbg_f3[(size_t)k * CF + tid] = *reinterpret_cast<const float*>(stage + stage_off(32 * mi + TOK3D, tid >> 2) + 4 * (tid & 3));
        }
    }
#pragma unroll
    for (int tt = 0; tt < 2; ++tt) {
        const float pp = corr_partial(xres[tt], lane);
        if (h == 0) scratch[ft * 64 + 32 * tt + r] = pp;         // (the LayerNorm exchange is done with: the layer's last barrier is behind us)
    }
    __syncthreads();
    if (ft < 2 && k0 + ft < total) expect_store(p, k0 + ft, scratch + 32 * ft, 64, lane);      // wave 0 finishes match k0, wave 1 match k0 + 1
    OPHIP_STAMP(p.stamps, blockIdx.x, 31);
}

template <typename K>
int set_lds(K kernel, size_t bytes, const char* what) {
    return ophip_lds_attr(reinterpret_cast<const void*>(kernel), bytes, what);
}

}  // namespace

extern "C" size_t ophip_fine_bf16_wpack_bytes(int nlayers) { return (size_t)nlayers * ((size_t)2 * W_ELEMS * 2 + 4 * CF * 4); }

namespace {
int fine_bf16(const float* feat_f, long long fs_b, long long fs_c, long long fs_y, long long fs_x, int hf, int wf,
              const float* desc3d_f, long long ds_b, long long ds_c,
              const long long* b_ids, const long long* i_ids, const long long* j_ids, const int* count, int max_matches,
              const float* mkpts_c, const void* wpack, int nlayers, unsigned cross_bits, int encoder_enable, int nsplit,
              int wc, int stride, float fine_scale, float* expec_f, float* mkpts_f,
              float* dbg_win, float* dbg_f3, const float* query_scale, void* stream_) {
    if (!feat_f || !desc3d_f || !b_ids || !i_ids || !j_ids || !count || !mkpts_c || !expec_f || !mkpts_f)
        return ophip_bad_arg(__func__, "null pointer");
    if (encoder_enable && (!wpack || nlayers < 1 || nlayers > 32)) return ophip_bad_arg(__func__, "encoder enabled without weights");
    if (nsplit != 1 && nsplit != 3) return ophip_bad_arg(__func__, "nsplit must be 1 (bf16) or 3 (split bf16)");
    if (fs_c == 1 && ((reinterpret_cast<uintptr_t>(feat_f) & 15) || (fs_b & 3) || (fs_y & 3) || (fs_x & 3)))
        return ophip_bad_arg(__func__, "channels-last feat_f needs 16-byte aligned pixels (strides multiples of 4 floats)");
    if ((dbg_win == nullptr) != (dbg_f3 == nullptr)) return ophip_bad_arg(__func__, "dbg_win and dbg_f3 go together");
    if (max_matches <= 0) return 0;
    // OPHIP_FINE_PRECISION=bf16 (model config `hip_fine_precision`): the fine stage alone on PLAIN bf16 operands (one matrix instruction per product
    // instead of three) while the coarse stage keeps the split form.  The fine stage only moves a match's sub-pixel offset: match indices cannot
    // change; keypoints move by <= 0.05 px, the pose stays within north_star's 1e-4 (tests/test_gpu_parity.py::test_fine_stage_in_plain_bf16...).
    // Not the default: the default keeps every keypoint within 1e-4 relative of the reference's.  (Read per call: a test compares both forms.)
    if (nsplit == 3) { const char* e = getenv("OPHIP_FINE_PRECISION"); if (e && e[0] == 'b' && e[1] == 'f' && e[2] == '1' && e[3] == '6' && e[4] == 0) nsplit = 1; }
    FineBArgs a;
    a.feat_f = feat_f; a.fs_b = fs_b; a.fs_c = fs_c; a.fs_y = fs_y; a.fs_x = fs_x; a.hf = hf; a.wf = wf;
    a.desc_f = desc3d_f; a.ds_b = ds_b; a.ds_c = ds_c;
    a.b_ids = b_ids; a.i_ids = i_ids; a.j_ids = j_ids; a.count = count; a.cap = max_matches; a.mkq_c = mkpts_c;
    static const int stagger = [] { const char* e = getenv("OPHIP_FINE_STAGGER"); return e ? atoi(e) : 0; }();
    a.stagger = stagger; a.ncu = 256;
    if (stagger > 0) { int dev = 0, n = 0; if (hipGetDevice(&dev) == hipSuccess && hipDeviceGetAttribute(&n, hipDeviceAttributeMultiprocessorCount, dev) == hipSuccess && n > 0) a.ncu = n; }
    a.wpack = reinterpret_cast<const char*>(wpack); a.nlayers = nlayers; a.cross_bits = cross_bits; a.enc_enable = encoder_enable;
    a.wc = wc; a.stride = stride; a.fine_scale = fine_scale; a.qscale = query_scale;
    a.expec_f = expec_f; a.mkq_f = mkpts_f; a.dbg_win = dbg_win; a.dbg_f3 = dbg_f3;
    a.stamps = ophip_stamp_buffer();
    hipStream_t stream = (hipStream_t)stream_;
    // two matches per 4-wave workgroup sharing every weight fragment (fine_pair_kernel); OPHIP_FINE_PAIR=0: one match per workgroup
    static const bool pair = [] { const char* e = getenv("OPHIP_FINE_PAIR"); return !(e && e[0] == '0'); }();
    if (pair) {
        const int gridp = (max_matches + 1) / 2;
        // (OPHIP_FINE_LDS_PAD: diagnostic -- extra dynamic LDS per workgroup, e.g. 40000 leaves room for ONE workgroup per CU: tools/stamps_fine.py
        //  then shows the phases of a workgroup that has its SIMDs to itself)
        static const size_t lds_pad = [] { const char* e = getenv("OPHIP_FINE_LDS_PAD"); return e ? (size_t)atol(e) : (size_t)0; }();
        const size_t ldsp = (size_t)64 * 1024 + 2048 + lds_pad;
        if (nsplit == 3) {
            if (int rc = set_lds(fine_pair_kernel<3>, ldsp, "hipFuncSetAttribute(fine_pair)")) return rc;
            OPHIP_LAUNCH("fine_refine", stream, (fine_pair_kernel<3>), dim3(gridp), dim3(256), ldsp, stream, a);
        } else {
            if (int rc = set_lds(fine_pair_kernel<1>, ldsp, "hipFuncSetAttribute(fine_pair)")) return rc;
            OPHIP_LAUNCH("fine_refine", stream, (fine_pair_kernel<1>), dim3(gridp), dim3(256), ldsp, stream, a);
        }
        OPHIP_CHECK_LAUNCH();
        return 0;
    }
    constexpr int NM = 1;
    const int grid = (max_matches + NM - 1) / NM;
    const size_t lds = (size_t)NM * (nsplit == 3 ? (16 + 16 + 32) : (8 + 8 + 16)) * 1024;
#define OPHIP_FINE_CASE(NS_, NM_)                                                                                               \
    {                                                                                                                           \
        if (int rc = set_lds(fine_refine_bf16_kernel<NS_, NM_>, lds, "hipFuncSetAttribute(fine_refine_bf16)")) return rc; \
        OPHIP_LAUNCH("fine_refine", stream, (fine_refine_bf16_kernel<NS_, NM_>), dim3(grid), dim3(NM_ * 256), lds, stream, a);  \
    }
    if (nsplit == 3) OPHIP_FINE_CASE(3, 1)
    else OPHIP_FINE_CASE(1, 1)
#undef OPHIP_FINE_CASE
    OPHIP_CHECK_LAUNCH();
    return 0;
}
}  // namespace

extern "C" int ophip_fine_refine_bf16(const float* feat_f, long long fs_b, long long fs_c, long long fs_y, long long fs_x, int hf, int wf,
                                      const float* desc3d_f, long long ds_b, long long ds_c,
                                      const long long* b_ids, const long long* i_ids, const long long* j_ids, const int* count, int max_matches,
                                      const float* mkpts_c, const void* wpack, int nlayers, unsigned cross_bits, int encoder_enable, int nsplit,
                                      int wc, int stride, float fine_scale, float* expec_f, float* mkpts_f,
                                      float* dbg_win, float* dbg_f3, void* stream) {
    return fine_bf16(feat_f, fs_b, fs_c, fs_y, fs_x, hf, wf, desc3d_f, ds_b, ds_c, b_ids, i_ids, j_ids, count, max_matches, mkpts_c, wpack, nlayers,
                     cross_bits, encoder_enable, nsplit, wc, stride, fine_scale, expec_f, mkpts_f, dbg_win, dbg_f3, nullptr, stream);
}

// ophip_fine_refine_bf16 with query_scale [B][2] = data["query_image_scale"] ((h, w) factors; fine_matching.py:104).
extern "C" int ophip_fine_refine_bf16_scaled(const float* feat_f, long long fs_b, long long fs_c, long long fs_y, long long fs_x, int hf, int wf,
                                             const float* desc3d_f, long long ds_b, long long ds_c,
                                             const long long* b_ids, const long long* i_ids, const long long* j_ids, const int* count, int max_matches,
                                             const float* mkpts_c, const void* wpack, int nlayers, unsigned cross_bits, int encoder_enable, int nsplit,
                                             int wc, int stride, float fine_scale, float* expec_f, float* mkpts_f,
                                             float* dbg_win, float* dbg_f3, const float* query_scale, void* stream) {
    if (!query_scale) return ophip_bad_arg(__func__, "null query_scale (use ophip_fine_refine_bf16)");
    return fine_bf16(feat_f, fs_b, fs_c, fs_y, fs_x, hf, wf, desc3d_f, ds_b, ds_c, b_ids, i_ids, j_ids, count, max_matches, mkpts_c, wpack, nlayers,
                     cross_bits, encoder_enable, nsplit, wc, stride, fine_scale, expec_f, mkpts_f, dbg_win, dbg_f3, query_scale, stream);
}
