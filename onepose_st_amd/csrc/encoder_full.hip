// Coarse LoFTR encoder layer with FULL (softmax) attention (d_model 256, 8 heads x 32) for the 3D-point stream and the
// 2D-grid stream of one frame batch -- reference: loftr_module/transformer.py:29-38,65-94 (LoFTREncoderLayer with
// attention "full"), linear_attention.py:64-95 (FullAttention: softmax(Q K^T / sqrt(D)) V, no eps, no v_length scaling).
//
// One layer = three launches, both streams in each launch:
//   full_qkv    (over all tokens)     Q | K | V projections of every row of both streams (exact-f32 MFMA tiles of tile.h,
//               the packed weight block of the f32 layer) -> workspace [B][L][256] planes
//   full_flash  (over QUERY tokens)   split-bf16 flash attention: one wave = 32 queries of one (batch, stream, head); loop over
//               32-key tiles with an online softmax (running max and sum in f32); msg -> workspace
//   full_tail   (over QUERY tokens)   merge -> LayerNorm -> [x, msg] -> MLP 512->512 ReLU ->256 -> LayerNorm -> x + msg
// No atomics and no split of the source axis: every output is a fixed-order chain, bit-identical on any run or batch position.
//
// ophip_encoder_layer_full_x3_stream runs the same three kernels on ONE query stream against one source stream (LoFTR's sequential
// cross layer: image 0 against image 1, then image 1 against the updated image 0): slot 0 carries the queries, slot 1 the source,
// and a batch stride of 0 makes an input one image shared by the whole batch, whose projections are computed once.
#include "tile_bf16.h"

namespace {

constexpr int C = 256;          // d_model
constexpr int NH = 8;           // heads
constexpr int HD = 32;          // head dim
constexpr int LDX = C + OPHIP_PAD;
constexpr int LDH = 2 * C + OPHIP_PAD;
constexpr int QT = 128;         // queries per flash workgroup (4 waves x 32)

__device__ __forceinline__ void load_rows_tile(float* lds, int ld, const float* __restrict__ x, int tok0, int L, int tid) {
    for (int i = tid; i < OPHIP_TOK * (C / 4); i += 256) {
        const int r = i / (C / 4), c4 = i % (C / 4);
        f32x4 v = {0.f, 0.f, 0.f, 0.f};
        if (tok0 + r < L) v = *reinterpret_cast<const f32x4*>(x + (size_t)(tok0 + r) * C + 4 * c4);
        *reinterpret_cast<f32x4*>(lds + r * ld + 4 * c4) = v;
    }
}

// rows tok0 + acc_row(reg, h) < L of a 32 x 32 accumulator tile -> dst[row][col0 + (lane & 31)]
__device__ __forceinline__ void store_acc_rows(const f32x16& acc, float* __restrict__ dst, int tok0, int L, int col0, int lane) {
    const int r = lane & 31, h = lane >> 5;
#pragma unroll
    for (int reg = 0; reg < 16; ++reg) {
        const int tok = tok0 + acc_row(reg, h);
        if (tok < L) dst[(size_t)tok * C + col0 + r] = acc[reg];
    }
}

__device__ __forceinline__ float swap32_max(float v) {               // max(v(lane), v(lane ^ 32))
    const unsigned u = __builtin_bit_cast(unsigned, v);
    auto c = __builtin_amdgcn_permlane32_swap(u, u, false, false);
    const unsigned c0 = c[0], c1 = c[1];
    return fmaxf(__builtin_bit_cast(float, c0), __builtin_bit_cast(float, c1));
}

// ---- (a) Q | K | V projections ---------------------------------------------------------------------------------------
struct QkvArgs {
    const float* x[2];
    float *q[2], *k[2], *v[2];     // [B][L_s][256] each
    long long bs[2];               // batch stride (floats) of the planes of stream s
    long long xbs[2];              // batch stride (floats) of x[s] (0: one image for every batch element)
    int nb[2];                     // batch elements of stream s with planes of their own (blocks past them leave)
    int parts[2];                  // planes written for stream s: 1 = Q, 2 = K | V, 3 = all three
    int L[2];
    int tiles[2];
    const f32x4 *wq, *wkv;         // f32 layer block: Wq tiles per wave, then [w][K heads 2w, 2w+1 | V heads 2w, 2w+1]
};

__global__ __launch_bounds__(256) OPHIP_WAVES_PER_SIMD(1, 2) void full_qkv_kernel(QkvArgs a) {
    extern __shared__ __attribute__((aligned(16))) float smem[];
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const int r = lane & 31, h = lane >> 5;
    const int tile = blockIdx.x, b = blockIdx.y;
    const int s = tile >= a.tiles[0] ? 1 : 0;
    const int lt = s ? tile - a.tiles[0] : tile;
    if (b >= a.nb[s]) return;                              // a shared image: its planes are those of batch element 0
    const int L = a.L[s], tok0 = lt * OPHIP_TOK;
    const size_t boff = (size_t)b * a.bs[s];
    load_rows_tile(smem, LDX, a.x[s] + (size_t)b * a.xbs[s], tok0, L, tid);
    __syncthreads();

    constexpr int KB = C / 8, TS = KB * 64;
    const float* xa = smem + r * LDX + 4 * h;
    if (a.parts[s] & 1) {
        f32x16 q[2] = {zero16(), zero16()};
        gemm_lds_x_packed<2>(q, xa, KB, a.wq + (size_t)(2 * wave) * TS + lane, TS);
#pragma unroll
        for (int t = 0; t < 2; ++t) store_acc_rows(q[t], a.q[s] + boff, tok0, L, 64 * wave + 32 * t, lane);
    }
    if (a.parts[s] & 2) {
        f32x16 kv[4] = {zero16(), zero16(), zero16(), zero16()};
        gemm_lds_x_packed<4>(kv, xa, KB, a.wkv + (size_t)(4 * wave) * TS + lane, TS);
#pragma unroll
        for (int t = 0; t < 2; ++t) {
            store_acc_rows(kv[t], a.k[s] + boff, tok0, L, HD * (2 * wave + t), lane);
            store_acc_rows(kv[2 + t], a.v[s] + boff, tok0, L, HD * (2 * wave + t), lane);
        }
    }
}

// ---- (b) split-bf16 flash attention, head dim 32 ---------------------------------------------------------------------
// Swapped product: X = K Q^T on v_mfma_f32_32x32x16_bf16 (A = 32 keys x 16 dims, B = 16 dims x 32 queries), so a lane owns one
// query's column (lane & 31) and 16 of its 32 keys (rows acc_row(reg, h)); the other 16 sit in lane ^ 32, so the row max and
// row sum need one permlane32 swap.  X's rows are the contraction index of O^T = V^T P^T: registers 8s .. 8s + 7 of P are the
// B fragment of k-step s as they stand (k slot j of lane half h = key 16 s + 8 (j >> 2) + 4 h + (j & 3)), and the V^T fragment
// reads the values of those keys.  Every product is hi*hi + hi*lo + lo*hi (small terms first), f32 accumulate.
struct FlashArgs {
    const float* q[2];             // query planes of stream s
    const float *k[2], *v[2];      // source planes FOR query stream s (own for "self", the other stream's for "cross")
    float* o[2];
    long long qbs[2], kbs[2], obs[2];  // batch strides (floats) of the query, source and output planes
    int L[2], S[2];
    int tiles[2];                  // QT-query tiles per stream
    float scale_log2;              // log2(e) / sqrt(HD)
};

__device__ __forceinline__ f32x16 mma32x3(const bf16x8& ahi, const bf16x8& alo, const bf16x8& bhi, const bf16x8& blo, f32x16 c) {
    c = __builtin_amdgcn_mfma_f32_32x32x16_bf16(alo, bhi, c, 0, 0, 0);
    c = __builtin_amdgcn_mfma_f32_32x32x16_bf16(ahi, blo, c, 0, 0, 0);
    return __builtin_amdgcn_mfma_f32_32x32x16_bf16(ahi, bhi, c, 0, 0, 0);
}

__device__ __forceinline__ void split_row8(const float* __restrict__ p, bool live, bf16x8& hi, bf16x8& lo) {
    f32x4 v0 = {0.f, 0.f, 0.f, 0.f}, v1 = v0;
    if (live) {
        v0 = *reinterpret_cast<const f32x4*>(p);
        v1 = *reinterpret_cast<const f32x4*>(p + 4);
    }
#pragma unroll
    for (int j = 0; j < 4; ++j) {
        __bf16 hh, ll;
        split_bf16(v0[j], hh, ll); hi[j] = hh; lo[j] = ll;
        split_bf16(v1[j], hh, ll); hi[4 + j] = hh; lo[4 + j] = ll;
    }
}

__global__ __launch_bounds__(256) void full_flash_kernel(FlashArgs a) {
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const int r = lane & 31, h = lane >> 5;
    const int tile = blockIdx.x, head = blockIdx.y, b = blockIdx.z;
    const int s = tile >= a.tiles[0] ? 1 : 0;
    const int lt = s ? tile - a.tiles[0] : tile;
    const int L = a.L[s], S = a.S[s];
    const int q0 = lt * QT + wave * 32;
    if (q0 >= L) return;                                   // no barriers below: a wave past the stream's end just leaves
    const float* __restrict__ Q = a.q[s] + (size_t)b * a.qbs[s] + head * HD;
    const float* __restrict__ K = a.k[s] + (size_t)b * a.kbs[s] + head * HD;
    const float* __restrict__ V = a.v[s] + (size_t)b * a.kbs[s] + head * HD;
    const int qrow = q0 + r;
    const float sc = a.scale_log2;

    bf16x8 qhi[2], qlo[2];
#pragma unroll
    for (int st = 0; st < 2; ++st) split_row8(Q + (size_t)qrow * C + 16 * st + 8 * h, qrow < L, qhi[st], qlo[st]);

    f32x16 o = zero16();
    float m = -INFINITY, l = 0.f;
    for (int k0 = 0; k0 < S; k0 += 32) {
        // ---- scores X[key][query] = K Q^T, scaled to the log2 domain; keys >= S -> -inf
        const int krow = k0 + r;
        bf16x8 khi[2], klo[2];
#pragma unroll
        for (int st = 0; st < 2; ++st) split_row8(K + (size_t)krow * C + 16 * st + 8 * h, krow < S, khi[st], klo[st]);
        // values of this tile's keys in the k order of the P fragments (issued before the score MFMAs: their latency hides behind them)
        float vr[16];
#pragma unroll
        for (int st = 0; st < 2; ++st) {
#pragma unroll
            for (int j = 0; j < 8; ++j) {
                const int key = k0 + 16 * st + 8 * (j >> 2) + 4 * h + (j & 3);
                vr[8 * st + j] = key < S ? V[(size_t)key * C + r] : 0.f;
            }
        }
        f32x16 x = zero16();
#pragma unroll
        for (int st = 0; st < 2; ++st) x = mma32x3(khi[st], klo[st], qhi[st], qlo[st], x);
        float tmax = -INFINITY;
#pragma unroll
        for (int reg = 0; reg < 16; ++reg) {
            const float t = (k0 + acc_row(reg, h) < S) ? x[reg] * sc : -INFINITY;
            x[reg] = t;
            tmax = fmaxf(tmax, t);
        }
        // key k0 (< S) is row 0 of lane half 0: the tile max is finite after the swap, so mn is finite from the first tile on
        const float mn = fmaxf(m, swap32_max(tmax));
        const float alpha = exp2f(m - mn);                 // 0 on the first tile (m = -inf)
        float rs = 0.f;
#pragma unroll
        for (int reg = 0; reg < 16; ++reg) {
            const float p = exp2f(x[reg] - mn);            // masked keys: exp2(-inf) = 0
            x[reg] = p;
            rs += p;
        }
        l = l * alpha + swap32_sum(rs);
        m = mn;
#pragma unroll
        for (int reg = 0; reg < 16; ++reg) o[reg] *= alpha;
        // ---- O^T[dim][query] += V^T P^T
#pragma unroll
        for (int st = 0; st < 2; ++st) {
            bf16x8 phi, plo, vhi, vlo;
#pragma unroll
            for (int j = 0; j < 8; ++j) {
                __bf16 hh, ll;
                split_bf16(x[8 * st + j], hh, ll); phi[j] = hh; plo[j] = ll;
                split_bf16(vr[8 * st + j], hh, ll); vhi[j] = hh; vlo[j] = ll;
            }
            o = mma32x3(vhi, vlo, phi, plo, o);
        }
    }
    if (qrow < L) {
        const float inv = 1.0f / l;
        float* dst = a.o[s] + (size_t)b * a.obs[s] + (size_t)qrow * C + head * HD + 4 * h;
#pragma unroll
        for (int g = 0; g < 4; ++g) {
            const f32x4 w = {o[4 * g] * inv, o[4 * g + 1] * inv, o[4 * g + 2] * inv, o[4 * g + 3] * inv};
            *reinterpret_cast<f32x4*>(dst + 8 * g) = w;
        }
    }
}

// ---- (c) merge, LayerNorm 1, MLP, LayerNorm 2, residual ---------------------------------------------------------------
struct TailArgs {
    const float* x[2];
    const float* msg[2];
    float* y[2];
    long long bs[2];               // batch stride (floats) of msg and y
    long long xbs[2];              // batch stride (floats) of x (0: one image for every batch element)
    int L[2];
    int tiles[2];
    const f32x4 *wm, *w0, *w2;
    const float *g1, *b1, *g2, *b2;
};

__global__ __launch_bounds__(256) OPHIP_WAVES_PER_SIMD(1, 1) void full_tail_kernel(TailArgs a) {
    extern __shared__ __attribute__((aligned(16))) float smem[];
    float* X = smem;                         // [32][LDX] layer input tile
    float* P = X + OPHIP_TOK * LDX;          // [32][LDX] merge out -> mlp out
    float* Hh = P + OPHIP_TOK * LDX;         // [32][LDH] attention message -> hidden
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const int r = lane & 31, h = lane >> 5;
    const int tile = blockIdx.x, b = blockIdx.y;
    const int s = tile >= a.tiles[0] ? 1 : 0;
    const int lt = s ? tile - a.tiles[0] : tile;
    const int L = a.L[s], tok0 = lt * OPHIP_TOK;
    const size_t boff = (size_t)b * a.bs[s];
    load_rows_tile(X, LDX, a.x[s] + (size_t)b * a.xbs[s], tok0, L, tid);
    load_rows_tile(Hh, LDH, a.msg[s] + boff, tok0, L, tid);
    __syncthreads();

    constexpr int KB = C / 8, TS = KB * 64;         // K = 256 GEMMs
    constexpr int KB2 = 2 * C / 8, TS2 = KB2 * 64;  // K = 512 GEMMs
    const float* xa = X + r * LDX + 4 * h;
    const float* pa = P + r * LDX + 4 * h;
    const float* ha = Hh + r * LDH + 4 * h;
    {
        f32x16 mm[2] = {zero16(), zero16()};
        gemm_lds_x_packed<2>(mm, ha, KB, a.wm + (size_t)(2 * wave) * TS + lane, TS);
#pragma unroll
        for (int t = 0; t < 2; ++t) acc_to_lds(mm[t], P, LDX, 64 * wave + 32 * t, lane);
    }
    __syncthreads();
    rows_layernorm<C, true, false>(P, LDX, a.g1, a.b1, 1e-5f, wave, lane);
    __syncthreads();
    {
        f32x16 hid[4] = {zero16(), zero16(), zero16(), zero16()};
        const f32x4* w0 = a.w0 + (size_t)(4 * wave) * TS2 + lane;
        gemm_lds_x_packed<4>(hid, xa, KB, w0, TS2);
        gemm_lds_x_packed<4>(hid, pa, KB, w0 + (size_t)KB * 64, TS2);
#pragma unroll
        for (int t = 0; t < 4; ++t) {
#pragma unroll
            for (int reg = 0; reg < 16; ++reg) hid[t][reg] = fmaxf(hid[t][reg], 0.f);
            acc_to_lds(hid[t], Hh, LDH, 128 * wave + 32 * t, lane);
        }
    }
    __syncthreads();
    {
        f32x16 oo[2] = {zero16(), zero16()};
        gemm_lds_x_packed<2>(oo, ha, KB2, a.w2 + (size_t)(2 * wave) * TS2 + lane, TS2);
#pragma unroll
        for (int t = 0; t < 2; ++t) acc_to_lds(oo[t], P, LDX, 64 * wave + 32 * t, lane);
    }
    __syncthreads();
    rows_layernorm<C, true, false>(P, LDX, a.g2, a.b2, 1e-5f, wave, lane);
    float* y = a.y[s] + boff;
    for (int rr = 0; rr < 8; ++rr) {
        const int row = 8 * wave + rr;
        if (tok0 + row < L) {
            const f32x4 xv = *reinterpret_cast<const f32x4*>(X + row * LDX + 4 * lane);
            const f32x4 mv = *reinterpret_cast<const f32x4*>(P + row * LDX + 4 * lane);
            *reinterpret_cast<f32x4*>(y + (size_t)(tok0 + row) * C + 4 * lane) = xv + mv;
        }
    }
}

}  // namespace

// Q, K, V and msg planes of both streams, [B][L3d + L2d][256] f32 each
extern "C" size_t ophip_encoder_full_workspace_bytes(int B, int L3d, int L2d) {
    if (B < 1 || L3d < 1 || L2d < 1) return 0;
    return (size_t)4 * B * ((size_t)L3d + L2d) * C * sizeof(float);
}

// One coarse layer with full attention.  wpack: the f32 layer block (Wq | Wkv | Wm | W0 | W2 | g1 b1 g2 b2, packing.pack_coarse_layer).
extern "C" int ophip_encoder_layer_full_x3(const float* x3d, const float* x2d, float* y3d, float* y2d, int B, int L3d, int L2d,
                                           const float* wpack, int is_cross, void* workspace, void* stream_) {
    if (!x3d || !x2d || !y3d || !y2d || !wpack || !workspace) return ophip_bad_arg(__func__, "null pointer");
    if (reinterpret_cast<uintptr_t>(workspace) & 15) return ophip_bad_arg(__func__, "workspace must be 16-byte aligned");
    if (B < 1 || L3d < 1 || L2d < 1) return ophip_bad_arg(__func__, "B, L3d, L2d must be >= 1");
    if (x3d == y3d || x2d == y2d) return ophip_bad_arg(__func__, "in-place layer is not supported (cross layers read the pre-update streams)");
    hipStream_t stream = (hipStream_t)stream_;
    const float* wq = wpack;
    const float* wkv = wq + C * C;
    const float* wm = wkv + 2 * C * C;
    const float* w0 = wm + C * C;
    const float* w2 = w0 + 4 * C * C;
    const float* ln = w2 + 2 * C * C;
    // workspace: plane p of stream s at base + (p * B * (L3d + L2d) + B * (s ? L3d : 0)) * C
    float* base = static_cast<float*>(workspace);
    const size_t plane = (size_t)B * ((size_t)L3d + L2d) * C;
    const int Ls[2] = {L3d, L2d};
    float* pl[4][2];
    for (int p = 0; p < 4; ++p) {
        pl[p][0] = base + p * plane;
        pl[p][1] = base + p * plane + (size_t)B * L3d * C;
    }
    const int t3 = (L3d + OPHIP_TOK - 1) / OPHIP_TOK, t2 = (L2d + OPHIP_TOK - 1) / OPHIP_TOK;

    QkvArgs qa;
    for (int s = 0; s < 2; ++s) {
        qa.q[s] = pl[0][s]; qa.k[s] = pl[1][s]; qa.v[s] = pl[2][s];
        qa.bs[s] = qa.xbs[s] = (long long)Ls[s] * C;
        qa.nb[s] = B;
        qa.parts[s] = 3;
        qa.L[s] = Ls[s];
    }
    qa.x[0] = x3d; qa.x[1] = x2d;
    qa.tiles[0] = t3; qa.tiles[1] = t2;
    qa.wq = reinterpret_cast<const f32x4*>(wq);
    qa.wkv = reinterpret_cast<const f32x4*>(wkv);
    const size_t lds_qkv = (size_t)OPHIP_TOK * LDX * sizeof(float);
    OPHIP_LAUNCH("full_qkv", stream, full_qkv_kernel, dim3(t3 + t2, B), dim3(256), lds_qkv, stream, qa);
    OPHIP_CHECK_LAUNCH();

    FlashArgs fa;
    for (int s = 0; s < 2; ++s) {
        const int src = is_cross ? 1 - s : s;          // stream 0 = 3D points, 1 = 2D grid (transformer.py:148-159)
        fa.q[s] = pl[0][s]; fa.k[s] = pl[1][src]; fa.v[s] = pl[2][src]; fa.o[s] = pl[3][s];
        fa.qbs[s] = fa.obs[s] = (long long)Ls[s] * C;
        fa.kbs[s] = (long long)Ls[src] * C;
        fa.L[s] = Ls[s];
        fa.S[s] = Ls[src];
        fa.tiles[s] = (Ls[s] + QT - 1) / QT;
    }
    fa.scale_log2 = 1.4426950408889634f / sqrtf((float)HD);
    OPHIP_LAUNCH("full_flash", stream, full_flash_kernel, dim3(fa.tiles[0] + fa.tiles[1], NH, B), dim3(256), 0, stream, fa);
    OPHIP_CHECK_LAUNCH();

    TailArgs ta;
    ta.x[0] = x3d; ta.x[1] = x2d; ta.y[0] = y3d; ta.y[1] = y2d;
    for (int s = 0; s < 2; ++s) {
        ta.msg[s] = pl[3][s];
        ta.bs[s] = ta.xbs[s] = (long long)Ls[s] * C;
        ta.L[s] = Ls[s];
    }
    ta.tiles[0] = t3; ta.tiles[1] = t2;
    ta.wm = reinterpret_cast<const f32x4*>(wm);
    ta.w0 = reinterpret_cast<const f32x4*>(w0);
    ta.w2 = reinterpret_cast<const f32x4*>(w2);
    ta.g1 = ln; ta.b1 = ln + C; ta.g2 = ln + 2 * C; ta.b2 = ln + 3 * C;
    const size_t lds_tail = (size_t)OPHIP_TOK * (2 * LDX + LDH) * sizeof(float);
    if (int rc = ophip_lds_attr(reinterpret_cast<const void*>(full_tail_kernel), lds_tail, "hipFuncSetAttribute(full_tail)")) return rc;
    OPHIP_LAUNCH("full_tail", stream, full_tail_kernel, dim3(t3 + t2, B), dim3(256), lds_tail, stream, ta);
    OPHIP_CHECK_LAUNCH();
    return 0;
}

// Q and msg planes [B][L][256], K and V planes [B][S][256] (a shared input uses the first [L or S][256] of its planes)
extern "C" size_t ophip_encoder_full_stream_workspace_bytes(int B, int L, int S) {
    if (B < 1 || L < 1 || S < 1) return 0;
    return (size_t)2 * B * ((size_t)L + S) * C * sizeof(float);
}

// One coarse layer with full attention on ONE query stream: y[b] = layer(x[b] against src[b]), x [B][L][256] at batch stride x_bstride,
// src [B][S][256] at src_bstride (floats; 0 = one image for every b, projected once).  src == x with equal strides and S == L is the
// self layer (one Q | K | V pass).  wpack as ophip_encoder_layer_full_x3.
extern "C" int ophip_encoder_layer_full_x3_stream(const float* x, long long x_bstride, const float* src, long long src_bstride, float* y,
                                                  int B, int L, int S, const float* wpack, void* workspace, void* stream_) {
    if (!x || !src || !y || !wpack || !workspace) return ophip_bad_arg(__func__, "null pointer");
    if (reinterpret_cast<uintptr_t>(workspace) & 15) return ophip_bad_arg(__func__, "workspace must be 16-byte aligned");
    if (B < 1 || L < 1 || S < 1) return ophip_bad_arg(__func__, "B, L, S must be >= 1");
    if (y == x || y == src) return ophip_bad_arg(__func__, "in-place layer is not supported (y must not alias x or src)");
    if ((x_bstride != 0 && x_bstride < (long long)L * C) || (src_bstride != 0 && src_bstride < (long long)S * C) || x_bstride % 4 != 0 ||
        src_bstride % 4 != 0)
        return ophip_bad_arg(__func__, "batch strides must be 0 or whole rows of at least L (S) x 256 floats, multiples of 4");
    hipStream_t stream = (hipStream_t)stream_;
    const float* wq = wpack;
    const float* wkv = wq + C * C;
    const float* wm = wkv + 2 * C * C;
    const float* w0 = wm + C * C;
    const float* w2 = w0 + 4 * C * C;
    const float* ln = w2 + 2 * C * C;
    const int nbx = x_bstride == 0 ? 1 : B, nbs = src_bstride == 0 ? 1 : B;
    const bool self = src == x && src_bstride == x_bstride && S == L;
    float* pq = static_cast<float*>(workspace);
    float* pk = pq + (size_t)B * L * C;
    float* pv = pk + (size_t)B * S * C;
    float* pm = pv + (size_t)B * S * C;
    const int tl = (L + OPHIP_TOK - 1) / OPHIP_TOK, ts = (S + OPHIP_TOK - 1) / OPHIP_TOK;

    // slot 0: the query rows (Q, or Q | K | V for self); slot 1: the source rows (K | V), no tiles for self
    QkvArgs qa;
    qa.x[0] = x; qa.xbs[0] = x_bstride; qa.nb[0] = nbx; qa.parts[0] = self ? 3 : 1; qa.L[0] = L; qa.tiles[0] = tl;
    qa.x[1] = src; qa.xbs[1] = src_bstride; qa.nb[1] = nbs; qa.parts[1] = 2; qa.L[1] = S; qa.tiles[1] = self ? 0 : ts;
    for (int s = 0; s < 2; ++s) {
        qa.q[s] = pq; qa.k[s] = pk; qa.v[s] = pv;
        qa.bs[s] = (long long)qa.L[s] * C;
    }
    qa.wq = reinterpret_cast<const f32x4*>(wq);
    qa.wkv = reinterpret_cast<const f32x4*>(wkv);
    const size_t lds_qkv = (size_t)OPHIP_TOK * LDX * sizeof(float);
    OPHIP_LAUNCH("full_qkv", stream, full_qkv_kernel, dim3(qa.tiles[0] + qa.tiles[1], self ? nbx : (nbx > nbs ? nbx : nbs)), dim3(256), lds_qkv,
                 stream, qa);
    OPHIP_CHECK_LAUNCH();

    FlashArgs fa;
    for (int s = 0; s < 2; ++s) {
        fa.q[s] = pq; fa.k[s] = pk; fa.v[s] = pv; fa.o[s] = pm;
        fa.qbs[s] = nbx > 1 ? (long long)L * C : 0;
        fa.kbs[s] = nbs > 1 ? (long long)S * C : 0;
        fa.obs[s] = (long long)L * C;
        fa.L[s] = L; fa.S[s] = S;
    }
    fa.tiles[0] = (L + QT - 1) / QT;
    fa.tiles[1] = 0;
    fa.scale_log2 = 1.4426950408889634f / sqrtf((float)HD);
    OPHIP_LAUNCH("full_flash", stream, full_flash_kernel, dim3(fa.tiles[0], NH, B), dim3(256), 0, stream, fa);
    OPHIP_CHECK_LAUNCH();

    TailArgs ta;
    for (int s = 0; s < 2; ++s) {
        ta.x[s] = x; ta.msg[s] = pm; ta.y[s] = y;
        ta.bs[s] = (long long)L * C;
        ta.xbs[s] = x_bstride;
        ta.L[s] = L;
    }
    ta.tiles[0] = tl;
    ta.tiles[1] = 0;
    ta.wm = reinterpret_cast<const f32x4*>(wm);
    ta.w0 = reinterpret_cast<const f32x4*>(w0);
    ta.w2 = reinterpret_cast<const f32x4*>(w2);
    ta.g1 = ln; ta.b1 = ln + C; ta.g2 = ln + 2 * C; ta.b2 = ln + 3 * C;
    const size_t lds_tail = (size_t)OPHIP_TOK * (2 * LDX + LDH) * sizeof(float);
    if (int rc = ophip_lds_attr(reinterpret_cast<const void*>(full_tail_kernel), lds_tail, "hipFuncSetAttribute(full_tail)")) return rc;
    OPHIP_LAUNCH("full_tail", stream, full_tail_kernel, dim3(tl, B), dim3(256), lds_tail, stream, ta);
    OPHIP_CHECK_LAUNCH();
    return 0;
}

// The attention step alone (timing and tests): q [B][L][256], k, v [B][S][256] -> msg [B][L][256], one stream, 8 heads of 32.
extern "C" int ophip_full_attention_h8d32(const float* q, const float* k, const float* v, int B, int L, int S, float* msg, void* stream_) {
    if (!q || !k || !v || !msg) return ophip_bad_arg(__func__, "null pointer");
    if (B < 1 || L < 1 || S < 1) return ophip_bad_arg(__func__, "B, L, S must be >= 1");
    FlashArgs fa;
    for (int s = 0; s < 2; ++s) {
        fa.q[s] = q; fa.k[s] = k; fa.v[s] = v; fa.o[s] = msg;
        fa.qbs[s] = fa.obs[s] = (long long)L * C;
        fa.kbs[s] = (long long)S * C;
        fa.L[s] = L; fa.S[s] = S;
    }
    fa.tiles[0] = (L + QT - 1) / QT;
    fa.tiles[1] = 0;
    fa.scale_log2 = 1.4426950408889634f / sqrtf((float)HD);
    hipStream_t stream = (hipStream_t)stream_;
    OPHIP_LAUNCH("full_flash", stream, full_flash_kernel, dim3(fa.tiles[0], NH, B), dim3(256), 0, stream, fa);
    OPHIP_CHECK_LAUNCH();
    return 0;
}
