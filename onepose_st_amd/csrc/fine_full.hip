// Fine stage of the 2D-3D matcher with FULL (softmax) attention in the fine encoder (loftr_fine.attention = "full":
// loftr_module/transformer.py:29-38, linear_attention.py:64-95; utils/fine_matching.py:28-110).  Batched over all matches like the
// detector's fine stage (loftr_fine.hip): token rows in HBM, one 3D token and 25 window tokens per match, every linear layer one
// split-bf16 GEMM over all rows (ophip_rows_linear_x3), LayerNorm rows (ophip_rows_layernorm128), and the per-match pieces here:
//   fine_full_gather     5 x 5 window of the fine map around the matched cell + the matched 3D point's fine descriptor
//   fine_full_attention  softmax(q k^T / 4) v per match, 8 heads of 16, L, S <= 32 (the stage uses 1 and 25), f32 on the vector ALU
//   fine_full_match      the 3D token against its 25 window tokens -> heat-map expectation, std, refined query keypoint
// Every kernel's grid covers the CAPACITY of the match lists and reads the device-side count: rows of matches >= count are written as
// zeros (gather, attention) or skipped (match), so nothing waits for the host to learn the count.
//
// The detector's LoFTR fine stage with loftr_fine.attention = "full" (loftr.py) needs window against window, W x W up to 11 x 11:
//   fine2_full_attention softmax(q k^T / 4) v per match, 8 heads of 16, 1 <= L, S <= 121; the match count is known on the host
#include "tile.h"

namespace {

constexpr int CF = 128, NH = 8, DH = CF / NH;

struct GatherArgs {
    const float* feat;                          // fine map, element (b, c, y, x) at b fs_b + c fs_c + y fs_y + x fs_x
    long long fs_b, fs_c, fs_y, fs_x;
    int hf, wf;
    const float* desc3d;                        // [B or 1][128][N]: element (b, c, i) at b d_bs + c d_cs + i
    long long d_bs, d_cs;
    const long long *b_ids, *i_ids, *j_ids;
    const int* count;
    int wc, stride, W;
    float* win;                                 // [cap][W * W][128]
    float* f3;                                  // [cap][128]
};

__global__ __launch_bounds__(256) void fine_full_gather_kernel(GatherArgs p) {
    const int m = blockIdx.x, tid = threadIdx.x, WW = p.W * p.W;
    float* dst = p.win + (size_t)m * WW * CF;
    if (m >= *p.count) {
        for (int e = tid; e < WW * CF; e += 256) dst[e] = 0.f;
        if (tid < CF) p.f3[(size_t)m * CF + tid] = 0.f;
        return;
    }
    const long long b = p.b_ids[m];
    const int cell = (int)p.j_ids[m], half = p.W / 2;
    const int cy = p.stride * (cell / p.wc), cx = p.stride * (cell % p.wc);
    const float* fb = p.feat + b * p.fs_b;
    for (int e = tid; e < WW * CF; e += 256) {
        const int rr = e / CF, c = e % CF;
        const int y = cy + rr / p.W - half, x = cx + rr % p.W - half;
        float v = 0.f;
        if (y >= 0 && y < p.hf && x >= 0 && x < p.wf) v = fb[c * p.fs_c + y * p.fs_y + x * p.fs_x];
        dst[e] = v;
    }
    if (tid < CF) p.f3[(size_t)m * CF + tid] = p.desc3d[b * p.d_bs + tid * p.d_cs + p.i_ids[m]];
}

struct AttnArgs {
    const float *q, *k, *v;                     // [cap][L][128], [cap][S][128], [cap][S][128]
    int L, S;
    const int* count;                           // NULL: every one of the cap matches is live
    float* msg;                                 // [cap][L][128]
};

// one workgroup per match; thread (l, head) computes that query's 16 outputs of the head: max pass, then exp / sum / weighted values
__global__ __launch_bounds__(256) void fine_full_attention_kernel(AttnArgs p) {
    __shared__ float ks[32 * CF], vs[32 * CF];
    const int m = blockIdx.x, tid = threadIdx.x;
    float* og = p.msg + (size_t)m * p.L * CF;
    if (p.count && m >= *p.count) {
        for (int e = tid; e < p.L * CF; e += 256) og[e] = 0.f;
        return;
    }
    const float* kg = p.k + (size_t)m * p.S * CF;
    const float* vg = p.v + (size_t)m * p.S * CF;
    for (int e = tid; e < p.S * CF; e += 256) {
        ks[e] = kg[e];
        vs[e] = vg[e];
    }
    __syncthreads();
    const float* qg = p.q + (size_t)m * p.L * CF;
    for (int it = tid; it < p.L * NH; it += 256) {
        const int l = it / NH, hh = it % NH;
        float qr[DH];
#pragma unroll
        for (int d = 0; d < DH; ++d) qr[d] = qg[l * CF + hh * DH + d];
        float mx = -INFINITY;
        for (int s = 0; s < p.S; ++s) {
            float dot = 0.f;
#pragma unroll
            for (int d = 0; d < DH; ++d) dot += qr[d] * ks[s * CF + hh * DH + d];
            mx = fmaxf(mx, 0.25f * dot);                     // softmax_temp = 1 / sqrt(16)
        }
        float acc[DH];
#pragma unroll
        for (int d = 0; d < DH; ++d) acc[d] = 0.f;
        float sum = 0.f;
        for (int s = 0; s < p.S; ++s) {
            float dot = 0.f;
#pragma unroll
            for (int d = 0; d < DH; ++d) dot += qr[d] * ks[s * CF + hh * DH + d];
            const float e = expf(0.25f * dot - mx);
            sum += e;
#pragma unroll
            for (int d = 0; d < DH; ++d) acc[d] += e * vs[s * CF + hh * DH + d];
        }
        const float inv = 1.0f / sum;
#pragma unroll
        for (int d = 0; d < DH; ++d) og[l * CF + hh * DH + d] = acc[d] * inv;
    }
}

// ---- LoFTR windows: one workgroup per (match, head), one thread per query token ---------------------------------------------
// The head's 16 key and 16 value columns of the match sit in LDS (2 x 121 x 64 B = 15.5 KB, so many workgroups share a CU); every lane
// of a wave reads the same key row, an LDS broadcast.  f32 on the vector ALU, the two passes of fine_full_attention_kernel: the exact row
// maximum first (the score recomputed in the second pass costs 16 FMAs per key, fewer than an online rescale of 16 accumulators), then
// exp / sum / weighted values.  q is pre-scaled by 1/4 = 1/sqrt(16), exact in binary.
constexpr int FW = 121;                         // tokens of an 11 x 11 window

struct Attn2Args {
    const float *q, *k, *v;                     // [K][L][128], [K][S][128], [K][S][128]
    int L, S;
    float* msg;                                 // [K][L][128]
};

// explicit FMAs: both passes round the score identically (the maximum is one of the scores, so its exp is exactly 1)
__device__ __forceinline__ float dot16(const float (&q)[DH], const float* __restrict__ row) {
    float d = 0.f;
#pragma unroll
    for (int c = 0; c < DH / 4; ++c) {
        const f32x4 kk = *reinterpret_cast<const f32x4*>(row + 4 * c);
#pragma unroll
        for (int j = 0; j < 4; ++j) d = __builtin_fmaf(q[4 * c + j], kk[j], d);
    }
    return d;
}

__global__ __launch_bounds__(128) void fine2_full_attention_kernel(Attn2Args p) {
    __shared__ __attribute__((aligned(16))) float ks[FW * DH], vs[FW * DH];
    const int m = blockIdx.x, hh = blockIdx.y, tid = threadIdx.x;
    const float* kg = p.k + (size_t)m * p.S * CF + hh * DH;
    const float* vg = p.v + (size_t)m * p.S * CF + hh * DH;
    for (int e = tid; e < p.S * (DH / 4); e += 128) {
        const int s = e / (DH / 4), c4 = e % (DH / 4);
        *reinterpret_cast<f32x4*>(ks + s * DH + 4 * c4) = *reinterpret_cast<const f32x4*>(kg + (size_t)s * CF + 4 * c4);
        *reinterpret_cast<f32x4*>(vs + s * DH + 4 * c4) = *reinterpret_cast<const f32x4*>(vg + (size_t)s * CF + 4 * c4);
    }
    __syncthreads();
    if (tid >= p.L) return;                                  // no barriers below
    const size_t row = ((size_t)m * p.L + tid) * CF + hh * DH;
    float qr[DH];
#pragma unroll
    for (int c = 0; c < DH / 4; ++c) {
        const f32x4 t = *reinterpret_cast<const f32x4*>(p.q + row + 4 * c);
#pragma unroll
        for (int j = 0; j < 4; ++j) qr[4 * c + j] = 0.25f * t[j];
    }
    float mx = -INFINITY;
    for (int s = 0; s < p.S; ++s) mx = fmaxf(mx, dot16(qr, ks + s * DH));
    float acc[DH];
#pragma unroll
    for (int d = 0; d < DH; ++d) acc[d] = 0.f;
    float sum = 0.f;
    for (int s = 0; s < p.S; ++s) {
        const float e = expf(dot16(qr, ks + s * DH) - mx);
        sum += e;
#pragma unroll
        for (int c = 0; c < DH / 4; ++c) {
            const f32x4 vv = *reinterpret_cast<const f32x4*>(vs + s * DH + 4 * c);
#pragma unroll
            for (int j = 0; j < 4; ++j) acc[4 * c + j] += e * vv[j];
        }
    }
    const float inv = 1.0f / sum;
#pragma unroll
    for (int c = 0; c < DH / 4; ++c) {
        const f32x4 o = {acc[4 * c] * inv, acc[4 * c + 1] * inv, acc[4 * c + 2] * inv, acc[4 * c + 3] * inv};
        *reinterpret_cast<f32x4*>(p.msg + row + 4 * c) = o;
    }
}

struct MatchArgs {
    const float *f3, *win;                      // [cap][128], [cap][WW][128]
    const float* mkc;                           // [cap][2] coarse query keypoints
    const long long* b_ids;
    const float* qscale;                        // [B][2] (h, w) factors or NULL
    const int* count;
    int W;
    float scale;                                // image height / fine height
    float *expec, *mkf;                         // [cap][3], [cap][2]
};

__global__ __launch_bounds__(128) void fine_full_match_kernel(MatchArgs p) {
    __shared__ float sim[128];
    __shared__ float cen[CF];
    const int m = blockIdx.x, tid = threadIdx.x, WW = p.W * p.W;
    if (m >= *p.count) return;
    cen[tid] = p.f3[(size_t)m * CF + tid];
    __syncthreads();
    float t = -INFINITY;
    if (tid < WW) {
        const float* row = p.win + ((size_t)m * WW + tid) * CF;
        float dot = 0.f;
        for (int c = 0; c < CF; ++c) dot += cen[c] * row[c];
        t = dot * 0.08838834764831845f;                       // 1 / sqrt(128)
    }
    sim[tid] = t;
    __syncthreads();
    if (tid < 64) {
        const float a = sim[tid], b = sim[tid + 64];
        const float mx = wave_max(fmaxf(a, b));
        const float ea = tid < WW ? expf(a - mx) : 0.f, eb = tid + 64 < WW ? expf(b - mx) : 0.f;
        const float sum = wave_sum(ea + eb);
        const float pa = ea / sum, pb = eb / sum;
        const float step = 2.0f / (float)(p.W - 1);
        const int ia = tid, ib = tid + 64;
        const float gxa = -1.0f + step * (float)(ia % p.W), gya = -1.0f + step * (float)(ia / p.W);
        const float gxb = -1.0f + step * (float)(ib % p.W), gyb = -1.0f + step * (float)(ib / p.W);
        const float ex = wave_sum(pa * gxa + pb * gxb), ey = wave_sum(pa * gya + pb * gyb);
        const float ex2 = wave_sum(pa * gxa * gxa + pb * gxb * gxb), ey2 = wave_sum(pa * gya * gya + pb * gyb * gyb);
        if (tid == 0) {
            const float vx = ex2 - ex * ex, vy = ey2 - ey * ey;
            p.expec[3 * m] = ex; p.expec[3 * m + 1] = ey;
            p.expec[3 * m + 2] = sqrtf(fmaxf(vx, 1e-10f)) + sqrtf(fmaxf(vy, 1e-10f));
            // fine_matching.py:104: mkpts_query_c + coords * (W // 2) * (scale * query_image_scale[b][[1, 0]])
            float sx = p.scale, sy = p.scale;
            if (p.qscale) {
                const long long b = p.b_ids[m];
                sx = p.scale * p.qscale[2 * b + 1];
                sy = p.scale * p.qscale[2 * b];
            }
            const float hw = (float)(p.W / 2);
            p.mkf[2 * m] = p.mkc[2 * m] + ex * hw * sx;
            p.mkf[2 * m + 1] = p.mkc[2 * m + 1] + ey * hw * sy;
        }
    }
}

}  // namespace

extern "C" int ophip_fine_full_gather(const float* feat_f, long long fs_b, long long fs_c, long long fs_y, long long fs_x, int hf, int wf,
                                      const float* desc3d_f, long long d_bs, long long d_cs, const long long* b_ids, const long long* i_ids,
                                      const long long* j_ids, const int* count, int cap, int wc, int stride, int W, float* windows,
                                      float* feat3d, void* stream_) {
    if (!feat_f || !desc3d_f || !b_ids || !i_ids || !j_ids || !count || !windows || !feat3d) return ophip_bad_arg(__func__, "null pointer");
    if (cap < 0 || W < 3 || (W & 1) == 0 || W * W > 128 || hf < 1 || wf < 1 || wc < 1 || stride < 1) return ophip_bad_arg(__func__, "bad sizes");
    if (cap == 0) return 0;
    hipStream_t stream = (hipStream_t)stream_;
    GatherArgs a{feat_f, fs_b, fs_c, fs_y, fs_x, hf, wf, desc3d_f, d_bs, d_cs, b_ids, i_ids, j_ids, count, wc, stride, W, windows, feat3d};
    OPHIP_LAUNCH("fine_full_gather", stream, fine_full_gather_kernel, dim3(cap), dim3(256), 0, stream, a);
    OPHIP_CHECK_LAUNCH();
    return 0;
}

extern "C" int ophip_fine_full_attention(const float* q, const float* k, const float* v, int K, int L, int S, const int* count, float* msg,
                                         void* stream_) {
    if (!q || !k || !v || !msg) return ophip_bad_arg(__func__, "null pointer");
    if (K < 0 || L < 1 || L > 32 || S < 1 || S > 32) return ophip_bad_arg(__func__, "bad sizes (1 <= L, S <= 32)");
    if (K == 0) return 0;
    hipStream_t stream = (hipStream_t)stream_;
    AttnArgs a{q, k, v, L, S, count, msg};
    OPHIP_LAUNCH("fine_full_attention", stream, fine_full_attention_kernel, dim3(K), dim3(256), 0, stream, a);
    OPHIP_CHECK_LAUNCH();
    return 0;
}

extern "C" int ophip_fine2_full_attention(const float* q, const float* k, const float* v, int K, int L, int S, float* msg, void* stream_) {
    if (!q || !k || !v || !msg) return ophip_bad_arg(__func__, "null pointer");
    if (K < 0 || L < 1 || L > FW || S < 1 || S > FW) return ophip_bad_arg(__func__, "bad sizes (K >= 0, 1 <= L, S <= 121)");
    if (K == 0) return 0;
    hipStream_t stream = (hipStream_t)stream_;
    Attn2Args a{q, k, v, L, S, msg};
    OPHIP_LAUNCH("fine2_full_attention", stream, fine2_full_attention_kernel, dim3(K, NH), dim3(128), 0, stream, a);
    OPHIP_CHECK_LAUNCH();
    return 0;
}

extern "C" int ophip_fine_full_match(const float* feat3d, const float* windows, const float* mkpts_c, const long long* b_ids,
                                     const float* query_scale, const int* count, int cap, int W, float scale, float* expec_f, float* mkpts_f,
                                     void* stream_) {
    if (!feat3d || !windows || !mkpts_c || !b_ids || !count || !expec_f || !mkpts_f) return ophip_bad_arg(__func__, "null pointer");
    if (cap < 0 || W < 3 || (W & 1) == 0 || W * W > 128) return ophip_bad_arg(__func__, "bad sizes (odd window, 3 .. 11)");
    if (cap == 0) return 0;
    hipStream_t stream = (hipStream_t)stream_;
    MatchArgs a{feat3d, windows, mkpts_c, b_ids, query_scale, count, W, scale, expec_f, mkpts_f};
    OPHIP_LAUNCH("fine_full_match", stream, fine_full_match_kernel, dim3(cap), dim3(128), 0, stream, a);
    OPHIP_CHECK_LAUNCH();
    return 0;
}
