// The backward of one LoFTREncoderLayer with linear attention (include/ext/onepose_encoder_backward.h).  The header is
// the specification: the formulas, every launch by its number, every point at which a value is split, the split rule of the sums over rows.
//
// rows_gemm_kernel<NN>   C[r][n] = epilogue(sum_k A[r][k] B[k][n]) over rows; B[k][n] = W[n][k] (NN = false: a forward product with a state
//                        dict's [out][in] matrix) or W[k][n] (NN = true: the dX product).  A wave: 64 rows x 64 columns (2 x 2 accumulators),
//                        operands read from float32 memory and split in registers; a workgroup: 64 rows x 256 columns.
// rows_tn_kernel         P[split][n][k] = sum over the split's rows of Y[r][n] X[r][k]: the dW products.  A wave: 64 x 64 of the output.
// head_tn_kernel         per frame, head and split: K_h^T V_h [32 x 32] and K_h^T w [32] (w: a per-row weight, or ones) -- KV / Ks, dKV / dKs.
// sum_splits_kernel      the owner's sum of the partials in ascending split order; writes, or adds once to what is there.
// attn_*_kernel          the per-head 32 x 32 applications in float32, one thread per row and head, KV in LDS.
// ln_*_kernel            LayerNorm forward (into hc = [x, n1]) and backward with per-block parameter partials; ln_params_kernel sums them.
// No float atomics, no sum whose order depends on the schedule.
#include "tile_bf16.h"
#include "capi_error.h"
#include "ext/onepose_encoder_backward.h"
#include <math.h>

namespace {

using capi::bad_arg;
using capi::blocks_of;

constexpr int kThreads = 256, C = OPENB_CHANNELS, H = OPENB_HEADS, D = OPENB_HEAD_DIM, HID = OPENB_HIDDEN, RT = OPENB_ROW_TILE,
              RB = OPENB_ROW_BLOCK;
static_assert(C == 256 && H == 8 && D == 32 && HID == 512 && RT == 64 && RB == 32 && H * D == C, "the kernels are written for these");
static_assert(OPENB_OFF_V_PROJ == OPENB_OFF_K_PROJ + C * C && OPENB_OFF_NORM2_BIAS + C == OPENB_PARAM_FLOATS, "the parameter layout");
constexpr float kEps = 1e-6f, kLnEps = 1e-5f;

enum Epilogue { EPI_NONE = 0, EPI_RELU, EPI_MASK, EPI_ADD2, EPI_PHI, EPI_PHI_SCALE };

__device__ __forceinline__ float phi(float t) { return t > 0.f ? t + 1.0f : expf(t); }

__device__ __forceinline__ void split8(const float (&v)[8], bf16x8& hi, bf16x8& lo) {
#pragma unroll
    for (int j = 0; j < 8; ++j) {
        __bf16 hh, ll;
        split_bf16(v[j], hh, ll);
        hi[j] = hh;
        lo[j] = ll;
    }
}

// eight consecutive floats (16-byte aligned)
__device__ __forceinline__ void load8(const float* src, float (&v)[8]) {
    const f32x4 a = *reinterpret_cast<const f32x4*>(src), b = *reinterpret_cast<const f32x4*>(src + 4);
#pragma unroll
    for (int j = 0; j < 4; ++j) {
        v[j] = a[j];
        v[4 + j] = b[j];
    }
}

struct GemmArgs {
    const float* A; int lda;
    const float* W; int ldw;
    float* Cout; int ldc;
    int R, K, epi;
    const float* e1; int lde1;      // EPI_MASK: the sign source; EPI_ADD2: the first addend
    const float* e2; int lde2;      // EPI_ADD2: the second addend
    float scale;                    // EPI_PHI_SCALE: the factor of the columns from 256
};

// grid: x = blocks of 64 rows, y = blocks of 256 columns
template <bool NN>
__global__ __launch_bounds__(kThreads) void rows_gemm_kernel(GemmArgs p) {
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6, r = lane & 31, h = lane >> 5;
    const int m0 = blockIdx.x * RT, n0 = blockIdx.y * 256 + wave * 64;
    f32x16 acc[2][2];
#pragma unroll
    for (int a = 0; a < 2; ++a)
#pragma unroll
        for (int b = 0; b < 2; ++b) acc[a][b] = zero16();
    const float* arow[2];
    bool live[2];
#pragma unroll
    for (int tm = 0; tm < 2; ++tm) {
        const int row = m0 + 32 * tm + r;
        live[tm] = row < p.R;
        arow[tm] = p.A + (size_t)(live[tm] ? row : 0) * p.lda + 8 * h;
    }
    for (int k0 = 0; k0 < p.K; k0 += 16) {
        bf16x8 ah[2], al[2], bh[2], bl[2];
#pragma unroll
        for (int tm = 0; tm < 2; ++tm) {
            float v[8] = {0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f};
            if (live[tm]) load8(arow[tm] + k0, v);
            split8(v, ah[tm], al[tm]);
        }
#pragma unroll
        for (int tn = 0; tn < 2; ++tn) {
            const int col = n0 + 32 * tn + r;
            float v[8];
            if (!NN) {
                load8(p.W + (size_t)col * p.ldw + k0 + 8 * h, v);
            } else {
#pragma unroll
                for (int j = 0; j < 8; ++j) v[j] = p.W[(size_t)(k0 + 8 * h + j) * p.ldw + col];
            }
            split8(v, bh[tn], bl[tn]);
        }
#pragma unroll
        for (int tm = 0; tm < 2; ++tm)
#pragma unroll
            for (int tn = 0; tn < 2; ++tn) acc[tm][tn] = mma_bf16<3>(ah[tm], al[tm], bh[tn], bl[tn], acc[tm][tn]);
    }
#pragma unroll
    for (int tm = 0; tm < 2; ++tm)
#pragma unroll
        for (int tn = 0; tn < 2; ++tn)
#pragma unroll
            for (int reg = 0; reg < 16; ++reg) {
                const int row = m0 + 32 * tm + acc_row(reg, h), col = n0 + 32 * tn + r;
                if (row >= p.R) continue;
                float v = acc[tm][tn][reg];
                switch (p.epi) {
                case EPI_RELU: v = fmaxf(v, 0.f); break;
                case EPI_MASK: v = p.e1[(size_t)row * p.lde1 + col] > 0.f ? v : 0.f; break;
                case EPI_ADD2: v = (v + p.e1[(size_t)row * p.lde1 + col]) + p.e2[(size_t)row * p.lde2 + col]; break;
                case EPI_PHI: v = phi(v); break;
                case EPI_PHI_SCALE: v = col < C ? phi(v) : v * p.scale; break;
                default: break;
                }
                p.Cout[(size_t)row * p.ldc + col] = v;
            }
}

struct TnArgs {
    const float* Y; int ldy;
    const float* X; int ldx;
    float* part;                    // [split][nout][kout]
    int R, rows_per_split, nout, kout;
};

// eight values of one column, rows row0 .. row0 + 7, zero from `end`
__device__ __forceinline__ void load_col8(const float* base, int ld, int row0, int end, float (&v)[8]) {
#pragma unroll
    for (int j = 0; j < 8; ++j) v[j] = row0 + j < end ? base[(size_t)(row0 + j) * ld] : 0.f;
}

// grid: x = the output's 64 x 64 tiles / 4 (a wave each), y = split
__global__ __launch_bounds__(kThreads) void rows_tn_kernel(TnArgs p) {
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6, r = lane & 31, h = lane >> 5;
    const int tile = blockIdx.x * 4 + wave, kt = p.kout / 64, n0 = 64 * (tile / kt), k0 = 64 * (tile % kt);
    const int begin = blockIdx.y * p.rows_per_split, end = min(p.R, begin + p.rows_per_split);
    f32x16 acc[2][2];
#pragma unroll
    for (int a = 0; a < 2; ++a)
#pragma unroll
        for (int b = 0; b < 2; ++b) acc[a][b] = zero16();
    for (int row = begin; row < end; row += 16) {
        bf16x8 ah[2], al[2], bh[2], bl[2];
#pragma unroll
        for (int t = 0; t < 2; ++t) {
            float v[8];
            load_col8(p.Y + n0 + 32 * t + r, p.ldy, row + 8 * h, end, v);
            split8(v, ah[t], al[t]);
            load_col8(p.X + k0 + 32 * t + r, p.ldx, row + 8 * h, end, v);
            split8(v, bh[t], bl[t]);
        }
#pragma unroll
        for (int tn = 0; tn < 2; ++tn)
#pragma unroll
            for (int tk = 0; tk < 2; ++tk) acc[tn][tk] = mma_bf16<3>(ah[tn], al[tn], bh[tk], bl[tk], acc[tn][tk]);
    }
    float* out = p.part + (size_t)blockIdx.y * p.nout * p.kout;
#pragma unroll
    for (int tn = 0; tn < 2; ++tn)
#pragma unroll
        for (int tk = 0; tk < 2; ++tk)
#pragma unroll
            for (int reg = 0; reg < 16; ++reg)
                out[(size_t)(n0 + 32 * tn + acc_row(reg, h)) * p.kout + k0 + 32 * tk + r] = acc[tn][tk][reg];
}

struct HeadTnArgs {
    const float* A; int lda;        // [B * T][lda], head h: columns 32 h ..
    const float* V; int ldv;
    const float* w;                 // [B * T][8] per row and head, or NULL: ones
    float* part_m;                  // [B][splits][8][32][32]
    float* part_v;                  // [B][splits][8][32]
    int T, rows_per_split;
};

// grid: x = head, y = split, z = frame; one wave
__global__ __launch_bounds__(64) void head_tn_kernel(HeadTnArgs p) {
    const int lane = threadIdx.x, r = lane & 31, h = lane >> 5, head = blockIdx.x, b = blockIdx.z;
    const int begin = blockIdx.y * p.rows_per_split, end = min(p.T, begin + p.rows_per_split);
    const float* A = p.A + (size_t)b * p.T * p.lda + D * head + r;
    const float* V = p.V + (size_t)b * p.T * p.ldv + D * head + r;
    const float* w = p.w ? p.w + (size_t)b * p.T * H + head : nullptr;
    f32x16 am = zero16(), av = zero16();
    for (int row = begin; row < end; row += 16) {
        bf16x8 ah, al, bh, bl, wh, wl;
        float v[8];
        load_col8(A, p.lda, row + 8 * h, end, v);
        split8(v, ah, al);
        load_col8(V, p.ldv, row + 8 * h, end, v);
        split8(v, bh, bl);
        if (w) load_col8(w, H, row + 8 * h, end, v);
        else
#pragma unroll
            for (int j = 0; j < 8; ++j) v[j] = 1.0f;
        split8(v, wh, wl);
        am = mma_bf16<3>(ah, al, bh, bl, am);
        av = mma_bf16<3>(ah, al, wh, wl, av);       // every column of av is the weighted column sum
    }
    const size_t item = ((size_t)b * gridDim.y + blockIdx.y) * H + head;
#pragma unroll
    for (int reg = 0; reg < 16; ++reg) {
        p.part_m[item * (D * D) + acc_row(reg, h) * D + r] = am[reg];
        if (r == 0) p.part_v[item * D + acc_row(reg, h)] = av[reg];
    }
}

// out[item][e] = (accumulate ? out[item][e] : 0) + (((0 + part[item][0][e]) + part[item][1][e]) + ..): one thread per element
__global__ __launch_bounds__(kThreads) void sum_splits_kernel(const float* __restrict__ part, float* __restrict__ out, int n, int splits,
                                                              int accumulate) {
    const int e = blockIdx.x * kThreads + threadIdx.x, item = blockIdx.y;
    if (e >= n) return;
    const float* src = part + (size_t)item * splits * n + e;
    float s = 0.f;
    for (int k = 0; k < splits; ++k) s = s + src[(size_t)k * n];
    float* dst = out + (size_t)item * n + e;
    *dst = accumulate ? *dst + s : s;
}

struct AttnArgs {
    float* Q;                       // [B * L][256]  (attn_bwd_k: [K, v'] [B * S][512], rewritten as [dk, dv])
    float* m;                       // forward: out; attn_bwd_q: in, rewritten as dnum
    float* dm;                      // attn_bwd_q: in, rewritten as dq
    float* Z;                       // [B * L][8]
    float* dden;                    // [B * L][8]
    const float* KV;                // [B][8][32][32]  (attn_bwd_k: dKV)
    const float* Ks;                // [B][8][32]      (attn_bwd_k: dKs)
    int T, S;                       // the rows of a frame; the source length
};

__device__ __forceinline__ void stage_kv(const AttnArgs& p, int b, float* kv, float* ks) {
    for (int e = threadIdx.x; e < H * D * D; e += kThreads) kv[e] = p.KV[(size_t)b * H * D * D + e];
    if (threadIdx.x < H * D) ks[threadIdx.x] = p.Ks[(size_t)b * H * D + threadIdx.x];
    __syncthreads();
}

__device__ __forceinline__ void load32(const float* src, float (&v)[D]) {
#pragma unroll
    for (int q = 0; q < D / 4; ++q) {
        const f32x4 a = *reinterpret_cast<const f32x4*>(src + 4 * q);
#pragma unroll
        for (int j = 0; j < 4; ++j) v[4 * q + j] = a[j];
    }
}
__device__ __forceinline__ void store32(float* dst, const float (&v)[D]) {
#pragma unroll
    for (int q = 0; q < D / 4; ++q) {
        const f32x4 a = {v[4 * q], v[4 * q + 1], v[4 * q + 2], v[4 * q + 3]};
        *reinterpret_cast<f32x4*>(dst + 4 * q) = a;
    }
}

// out[v] = sum_d a[d] * kv[d][v], d ascending from 0.0f
__device__ __forceinline__ void apply_rows(const float (&a)[D], const float* kv, float (&out)[D]) {
#pragma unroll
    for (int v = 0; v < D; ++v) out[v] = 0.f;
#pragma unroll
    for (int d = 0; d < D; ++d) {
#pragma unroll
        for (int q = 0; q < D / 4; ++q) {
            const f32x4 k4 = *reinterpret_cast<const f32x4*>(kv + d * D + 4 * q);
#pragma unroll
            for (int j = 0; j < 4; ++j) out[4 * q + j] = out[4 * q + j] + a[d] * k4[j];
        }
        __builtin_amdgcn_sched_barrier(0);          // one row of KV in flight: hoisted, the 1 024 LDS reads do not fit the registers
    }
}
// out[d] = sum_v kv[d][v] * a[v], v ascending from 0.0f
__device__ __forceinline__ void apply_cols(const float (&a)[D], const float* kv, float (&out)[D]) {
#pragma unroll
    for (int d = 0; d < D; ++d) {
        float s = 0.f;
#pragma unroll
        for (int q = 0; q < D / 4; ++q) {
            const f32x4 k4 = *reinterpret_cast<const f32x4*>(kv + d * D + 4 * q);
#pragma unroll
            for (int j = 0; j < 4; ++j) s = s + k4[j] * a[4 * q + j];
        }
        out[d] = s;
        __builtin_amdgcn_sched_barrier(0);
    }
}

// grid: x = blocks of 32 rows, y = frame; thread: row = tid & 31, head = tid >> 5
__global__ __launch_bounds__(kThreads) void attn_fwd_kernel(AttnArgs p) {
    __shared__ __attribute__((aligned(16))) float kv[H * D * D];
    __shared__ float ks[H * D];
    const int b = blockIdx.y, head = threadIdx.x >> 5, row = blockIdx.x * RB + (threadIdx.x & 31);
    stage_kv(p, b, kv, ks);
    if (row >= p.T) return;
    const size_t at = (size_t)b * p.T + row;
    float q[D], num[D];
    load32(p.Q + at * C + D * head, q);
    float den = 0.f;
#pragma unroll
    for (int d = 0; d < D; ++d) den = den + q[d] * ks[D * head + d];
    const float z = 1.0f / (den + kEps), zs = z * (float)p.S;
    apply_rows(q, kv + head * D * D, num);
#pragma unroll
    for (int v = 0; v < D; ++v) num[v] = num[v] * zs;
    store32(p.m + at * C + D * head, num);
    p.Z[at * H + head] = z;
}

__global__ __launch_bounds__(kThreads) void attn_bwd_q_kernel(AttnArgs p) {
    __shared__ __attribute__((aligned(16))) float kv[H * D * D];
    __shared__ float ks[H * D];
    const int b = blockIdx.y, head = threadIdx.x >> 5, row = blockIdx.x * RB + (threadIdx.x & 31);
    stage_kv(p, b, kv, ks);
    if (row >= p.T) return;
    const size_t at = (size_t)b * p.T + row;
    float q[D], dm[D], t[D];
    load32(p.Q + at * C + D * head, q);
    load32(p.dm + at * C + D * head, dm);
    load32(p.m + at * C + D * head, t);
    const float z = p.Z[at * H + head], zs = z * (float)p.S;
    float dot = 0.f;
#pragma unroll
    for (int v = 0; v < D; ++v) dot = dot + dm[v] * t[v];
    const float dden = -z * dot;
#pragma unroll
    for (int v = 0; v < D; ++v) dm[v] = dm[v] * zs;                 // dnum
    store32(p.m + at * C + D * head, dm);
    p.dden[at * H + head] = dden;
    apply_cols(dm, kv + head * D * D, t);                           // KV dnum
#pragma unroll
    for (int d = 0; d < D; ++d) t[d] = (t[d] + dden * ks[D * head + d]) * fminf(q[d], 1.0f);
    store32(p.dm + at * C + D * head, t);                           // dq
}

// over the source rows: Q is [K, v'] with 512 columns, KV is dKV, Ks is dKs; T = S
__global__ __launch_bounds__(kThreads) void attn_bwd_k_kernel(AttnArgs p) {
    __shared__ __attribute__((aligned(16))) float kv[H * D * D];
    __shared__ float ks[H * D];
    const int b = blockIdx.y, head = threadIdx.x >> 5, row = blockIdx.x * RB + (threadIdx.x & 31);
    stage_kv(p, b, kv, ks);
    if (row >= p.T) return;
    float* at = p.Q + ((size_t)b * p.T + row) * HID + D * head;
    float k[D], vp[D], t[D];
    load32(at, k);
    load32(at + C, vp);
    apply_cols(vp, kv + head * D * D, t);                           // dKV v'
#pragma unroll
    for (int d = 0; d < D; ++d) t[d] = (t[d] + ks[D * head + d]) * fminf(k[d], 1.0f);
    store32(at, t);                                                 // dk
    apply_rows(k, kv + head * D * D, t);                            // K dKV
    const float s = (float)p.S;
#pragma unroll
    for (int v = 0; v < D; ++v) t[v] = t[v] / s;
    store32(at + C, t);                                             // dv
}

struct LnArgs {
    const float* z; int ldz;        // the pre-norm rows
    const float* x;                 // forward: the rows copied into hc[:, :256]
    const float* dn; int lddn;      // backward: the gradient at the output
    const float* weight;
    const float* bias;
    float* out; int ldo;            // forward: hc (n1 at column 256); backward: dz
    float* part;                    // backward: [blocks][512]: dweight, dbias of the block's rows
    int R;
};

__device__ __forceinline__ void row_stats(const float (&v)[4], float& mean, float& rstd) {
    mean = wave_sum((v[0] + v[1]) + (v[2] + v[3])) * (1.0f / C);
    float q = 0.f;
#pragma unroll
    for (int e = 0; e < 4; ++e) q = q + (v[e] - mean) * (v[e] - mean);
    rstd = 1.0f / sqrtf(wave_sum(q) * (1.0f / C) + kLnEps);
}

// grid: blocks of 32 rows; wave w: rows 8 w .. 8 w + 7; lane: columns lane + 64 e
__global__ __launch_bounds__(kThreads) void ln_fwd_kernel(LnArgs p) {
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    for (int rr = 0; rr < 8; ++rr) {
        const int row = blockIdx.x * RB + 8 * wave + rr;
        if (row >= p.R) return;
        float v[4], mean, rstd;
#pragma unroll
        for (int e = 0; e < 4; ++e) v[e] = p.z[(size_t)row * p.ldz + lane + 64 * e];
        row_stats(v, mean, rstd);
#pragma unroll
        for (int e = 0; e < 4; ++e) {
            const int c = lane + 64 * e;
            p.out[(size_t)row * p.ldo + c] = p.x[(size_t)row * C + c];
            p.out[(size_t)row * p.ldo + C + c] = ((v[e] - mean) * rstd) * p.weight[c] + p.bias[c];
        }
    }
}

__global__ __launch_bounds__(kThreads) void ln_bwd_kernel(LnArgs p) {
    __shared__ float red[4][2 * C];
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    float dw[4] = {0.f, 0.f, 0.f, 0.f}, db[4] = {0.f, 0.f, 0.f, 0.f}, w[4];
#pragma unroll
    for (int e = 0; e < 4; ++e) w[e] = p.weight[lane + 64 * e];
    for (int rr = 0; rr < 8; ++rr) {
        const int row = blockIdx.x * RB + 8 * wave + rr;
        if (row >= p.R) break;
        float v[4], dn[4], g[4], mean, rstd;
#pragma unroll
        for (int e = 0; e < 4; ++e) {
            v[e] = p.z[(size_t)row * p.ldz + lane + 64 * e];
            dn[e] = p.dn[(size_t)row * p.lddn + lane + 64 * e];
        }
        row_stats(v, mean, rstd);
        float sg = 0.f, sgz = 0.f;
#pragma unroll
        for (int e = 0; e < 4; ++e) {
            v[e] = (v[e] - mean) * rstd;                            // zhat
            g[e] = dn[e] * w[e];
            sg = sg + g[e];
            sgz = sgz + g[e] * v[e];
            dw[e] = dw[e] + dn[e] * v[e];
            db[e] = db[e] + dn[e];
        }
        const float mg = wave_sum(sg) * (1.0f / C), mgz = wave_sum(sgz) * (1.0f / C);
#pragma unroll
        for (int e = 0; e < 4; ++e) p.out[(size_t)row * p.ldo + lane + 64 * e] = rstd * ((g[e] - mg) - v[e] * mgz);
    }
#pragma unroll
    for (int e = 0; e < 4; ++e) {
        red[wave][lane + 64 * e] = dw[e];
        red[wave][C + lane + 64 * e] = db[e];
    }
    __syncthreads();
    for (int c = threadIdx.x; c < 2 * C; c += kThreads)
        p.part[(size_t)blockIdx.x * 2 * C + c] = ((red[0][c] + red[1][c]) + red[2][c]) + red[3][c];
}

// thread c of 512: the sum over the blocks ascending; columns 0..255 into dweight, the rest into dbias (they are neighbours in dparams)
__global__ __launch_bounds__(kThreads) void ln_params_kernel(const float* __restrict__ part, int blocks, float* __restrict__ out, int accumulate) {
    const int c = blockIdx.x * kThreads + threadIdx.x;
    float s = 0.f;
    for (int k = 0; k < blocks; ++k) s = s + part[(size_t)k * 2 * C + c];
    out[c] = accumulate ? out[c] + s : s;
}

size_t align256(size_t n) { return (n + 255) & ~(size_t)255; }

int rows_per_split(int T) {
    const int even = (((T + OPENB_MAX_SPLITS - 1) / OPENB_MAX_SPLITS) + 31) / 32 * 32;
    return even > OPENB_SPLIT_ROWS ? even : OPENB_SPLIT_ROWS;
}
int splits_of(int T) { return (T + rows_per_split(T) - 1) / rows_per_split(T); }

struct Layout {
    size_t Q, kv, m, msg, hc, h, o, d_o, Z, dden, ln1, ln2, part_kv, part_ks, KV, Ks, part_dkv, part_dks, dKV, dKs, part_w, total;
};

Layout layout_of(int B, int L, int S) {
    Layout l;
    size_t at = 0;
    auto take = [&](size_t floats) {
        const size_t here = at;
        at += align256(floats * 4);
        return here;
    };
    const size_t RX = (size_t)B * L, RS = (size_t)B * S, blocks = (RX + RB - 1) / RB;
    l.Q = take(RX * C);
    l.kv = take(RS * HID);
    l.m = take(RX * C);
    l.msg = take(RX * C);
    l.hc = take(RX * HID);
    l.h = take(RX * HID);
    l.o = take(RX * C);
    l.d_o = take(RX * C);
    l.Z = take(RX * H);
    l.dden = take(RX * H);
    l.ln1 = take(blocks * 2 * C);
    l.ln2 = take(blocks * 2 * C);
    l.part_kv = take((size_t)B * splits_of(S) * H * D * D);
    l.part_ks = take((size_t)B * splits_of(S) * H * D);
    l.KV = take((size_t)B * H * D * D);
    l.Ks = take((size_t)B * H * D);
    l.part_dkv = take((size_t)B * splits_of(L) * H * D * D);
    l.part_dks = take((size_t)B * splits_of(L) * H * D);
    l.dKV = take((size_t)B * H * D * D);
    l.dKs = take((size_t)B * H * D);
    l.part_w = take((size_t)OPENB_MAX_SPLITS * HID * HID);
    l.total = at;
    return l;
}

bool shape_ok(int B, int L, int S) {
    return B >= 1 && B <= OPENB_MAX_BATCH && L >= 1 && L <= OPENB_MAX_ROWS && S >= 1 && S <= OPENB_MAX_ROWS &&
           (long long)B * L <= OPENB_MAX_TOTAL_ROWS && (long long)B * S <= OPENB_MAX_TOTAL_ROWS;
}

bool overlap(const void* a, size_t na, const void* b, size_t nb) {
    const uintptr_t x = (uintptr_t)a, y = (uintptr_t)b;
    return x < y + nb && y < x + na;
}

int gemm(hipStream_t stream, bool nn, const float* A, int lda, const float* W, int ldw, float* out, int ldc, int R, int N, int K, int epi,
         const float* e1 = nullptr, int lde1 = 0, const float* e2 = nullptr, int lde2 = 0, float scale = 1.0f) {
    const GemmArgs a = {A, lda, W, ldw, out, ldc, R, K, epi, e1, lde1, e2, lde2, scale};
    const dim3 grid(blocks_of(R, RT), N / 256);
    if (nn) rows_gemm_kernel<true><<<grid, kThreads, 0, stream>>>(a);
    else rows_gemm_kernel<false><<<grid, kThreads, 0, stream>>>(a);
    CAPI_CHECK_LAUNCH();
    return 0;
}

// dW [nout][kout] = Y^T X over R rows, into (or added once to) `out`
int weight_grad(hipStream_t stream, const float* Y, int ldy, const float* X, int ldx, int R, int nout, int kout, float* part, float* out,
                int accumulate) {
    const int rps = rows_per_split(R), splits = splits_of(R);
    const TnArgs a = {Y, ldy, X, ldx, part, R, rps, nout, kout};
    rows_tn_kernel<<<dim3((nout / 64) * (kout / 64) / 4, splits), kThreads, 0, stream>>>(a);
    CAPI_CHECK_LAUNCH();
    sum_splits_kernel<<<dim3(blocks_of((long long)nout * kout, kThreads), 1), kThreads, 0, stream>>>(part, out, nout * kout, splits, accumulate);
    CAPI_CHECK_LAUNCH();
    return 0;
}

int head_sums(hipStream_t stream, const float* A, int lda, const float* V, int ldv, const float* w, int B, int T, float* part_m, float* part_v,
              float* out_m, float* out_v) {
    const int rps = rows_per_split(T), splits = splits_of(T);
    const HeadTnArgs a = {A, lda, V, ldv, w, part_m, part_v, T, rps};
    head_tn_kernel<<<dim3(H, splits, B), 64, 0, stream>>>(a);
    CAPI_CHECK_LAUNCH();
    sum_splits_kernel<<<dim3(blocks_of(H * D * D, kThreads), B), kThreads, 0, stream>>>(part_m, out_m, H * D * D, splits, 0);
    CAPI_CHECK_LAUNCH();
    sum_splits_kernel<<<dim3(blocks_of(H * D, kThreads), B), kThreads, 0, stream>>>(part_v, out_v, H * D, splits, 0);
    CAPI_CHECK_LAUNCH();
    return 0;
}

}  // namespace

#define OPENB_TRY(call)          \
    do {                         \
        if (int rc__ = (call)) return rc__; \
    } while (0)

extern "C" {

int openb_abi_version(void) { return OPENB_ABI_VERSION; }
const char* openb_last_error(void) { return capi::g_error; }

size_t openb_layer_workspace_bytes(int B, int L, int S) { return shape_ok(B, L, S) ? layout_of(B, L, S).total : 0; }

int openb_layer_grads(const float* x, const float* source, const float* dy, int B, int L, int S, const float* params, void* workspace,
                      size_t workspace_bytes, float* dx, float* dsource, float* dparams, int accumulate, void* stream_) {
    if (x == nullptr || source == nullptr || dy == nullptr || params == nullptr || workspace == nullptr || dx == nullptr || dsource == nullptr ||
        dparams == nullptr)
        return bad_arg(__func__, "null pointer");
    if (B < 1 || B > OPENB_MAX_BATCH) return bad_arg(__func__, "B outside [1, OPENB_MAX_BATCH]");
    if (L < 1 || L > OPENB_MAX_ROWS || S < 1 || S > OPENB_MAX_ROWS) return bad_arg(__func__, "L and S: in [1, OPENB_MAX_ROWS]");
    if (!shape_ok(B, L, S)) return bad_arg(__func__, "B * L and B * S: at most OPENB_MAX_TOTAL_ROWS");
    const void* all[] = {x, source, dy, params, dx, dsource, dparams};
    for (const void* a : all)
        if (((uintptr_t)a & 15) != 0) return bad_arg(__func__, "x, source, dy, params, dx, dsource, dparams: 16-byte aligned");
    if (((uintptr_t)workspace & 255) != 0) return bad_arg(__func__, "workspace: 256-byte aligned");
    const Layout l = layout_of(B, L, S);
    if (workspace_bytes < l.total) return bad_arg(__func__, "workspace_bytes below openb_layer_workspace_bytes(B, L, S)");
    const int RX = B * L, RS = B * S;
    const size_t nx = (size_t)RX * C * 4, ns = (size_t)RS * C * 4, np = (size_t)OPENB_PARAM_FLOATS * 4;
    const void* ins[] = {x, source, dy, params, workspace};
    const size_t in_bytes[] = {nx, ns, nx, np, l.total};
    const void* outs[] = {dx, dsource, dparams};
    const size_t out_bytes[] = {nx, ns, np};
    for (int o = 0; o < 3; ++o) {
        for (int i = 0; i < 5; ++i)
            if (overlap(outs[o], out_bytes[o], ins[i], in_bytes[i])) return bad_arg(__func__, "an output overlaps an input or the workspace");
        for (int q = o + 1; q < 3; ++q)
            if (overlap(outs[o], out_bytes[o], outs[q], out_bytes[q])) return bad_arg(__func__, "two outputs overlap");
    }
    for (int i = 0; i < 4; ++i)
        if (overlap(workspace, l.total, ins[i], in_bytes[i])) return bad_arg(__func__, "an input overlaps the workspace");

    hipStream_t stream = (hipStream_t)stream_;
    char* ws = static_cast<char*>(workspace);
    auto f = [&](size_t off) { return reinterpret_cast<float*>(ws + off); };
    float *Q = f(l.Q), *kv = f(l.kv), *m = f(l.m), *msg = f(l.msg), *hc = f(l.hc), *h = f(l.h), *o = f(l.o), *d_o = f(l.d_o), *Z = f(l.Z),
          *dden = f(l.dden), *part_w = f(l.part_w);
    const float *Wq = params + OPENB_OFF_Q_PROJ, *Wkv = params + OPENB_OFF_K_PROJ, *Wm = params + OPENB_OFF_MERGE, *W0 = params + OPENB_OFF_MLP0,
                *W2 = params + OPENB_OFF_MLP2;
    const int acc = accumulate != 0, blocks = (int)blocks_of(RX, RB);
    const dim3 xgrid(blocks_of(L, RB), B), sgrid(blocks_of(S, RB), B);

    // the forward, recomputed (the header's launch numbers)
    OPENB_TRY(gemm(stream, false, x, C, Wq, C, Q, C, RX, C, C, EPI_PHI));                                                         // 1
    OPENB_TRY(gemm(stream, false, source, C, Wkv, C, kv, HID, RS, HID, C, EPI_PHI_SCALE, nullptr, 0, nullptr, 0, 1.0f / (float)S));  // 2
    OPENB_TRY(head_sums(stream, kv, HID, kv + C, HID, nullptr, B, S, f(l.part_kv), f(l.part_ks), f(l.KV), f(l.Ks)));              // 3, 4
    AttnArgs at = {Q, m, d_o, Z, dden, f(l.KV), f(l.Ks), L, S};
    attn_fwd_kernel<<<xgrid, kThreads, 0, stream>>>(at);                                                                          // 5
    CAPI_CHECK_LAUNCH();
    OPENB_TRY(gemm(stream, false, m, C, Wm, C, msg, C, RX, C, C, EPI_NONE));                                                      // 6
    LnArgs ln = {msg, C, x, nullptr, 0, params + OPENB_OFF_NORM1_WEIGHT, params + OPENB_OFF_NORM1_BIAS, hc, HID, nullptr, RX};
    ln_fwd_kernel<<<blocks, kThreads, 0, stream>>>(ln);                                                                           // 7
    CAPI_CHECK_LAUNCH();
    OPENB_TRY(gemm(stream, false, hc, HID, W0, HID, h, HID, RX, HID, HID, EPI_RELU));                                             // 8
    OPENB_TRY(gemm(stream, false, h, HID, W2, HID, o, C, RX, C, HID, EPI_NONE));                                                  // 9

    // the backward
    ln = {o, C, nullptr, dy, C, params + OPENB_OFF_NORM2_WEIGHT, nullptr, d_o, C, f(l.ln2), RX};
    ln_bwd_kernel<<<blocks, kThreads, 0, stream>>>(ln);                                                                           // 10
    CAPI_CHECK_LAUNCH();
    OPENB_TRY(weight_grad(stream, d_o, C, h, HID, RX, C, HID, part_w, dparams + OPENB_OFF_MLP2, acc));                            // 11
    OPENB_TRY(gemm(stream, true, d_o, C, W2, HID, h, HID, RX, HID, C, EPI_MASK, h, HID));                                         // 12: dh over h
    OPENB_TRY(weight_grad(stream, h, HID, hc, HID, RX, HID, HID, part_w, dparams + OPENB_OFF_MLP0, acc));                         // 13
    OPENB_TRY(gemm(stream, true, h, HID, W0, HID, hc, HID, RX, HID, HID, EPI_NONE));                                              // 14: dhc over hc
    ln = {msg, C, nullptr, hc + C, HID, params + OPENB_OFF_NORM1_WEIGHT, nullptr, o, C, f(l.ln1), RX};
    ln_bwd_kernel<<<blocks, kThreads, 0, stream>>>(ln);                                                                           // 15: dmsg over o
    CAPI_CHECK_LAUNCH();
    OPENB_TRY(weight_grad(stream, o, C, m, C, RX, C, C, part_w, dparams + OPENB_OFF_MERGE, acc));                                 // 16
    OPENB_TRY(gemm(stream, true, o, C, Wm, C, d_o, C, RX, C, C, EPI_NONE));                                                       // 17: dm over do
    attn_bwd_q_kernel<<<xgrid, kThreads, 0, stream>>>(at);                                                                        // 18: dq over dm, dnum over m
    CAPI_CHECK_LAUNCH();
    OPENB_TRY(head_sums(stream, Q, C, m, C, dden, B, L, f(l.part_dkv), f(l.part_dks), f(l.dKV), f(l.dKs)));                       // 19
    at = {kv, nullptr, nullptr, nullptr, nullptr, f(l.dKV), f(l.dKs), S, S};
    attn_bwd_k_kernel<<<sgrid, kThreads, 0, stream>>>(at);                                                                        // 20: [dk, dv] over [K, v']
    CAPI_CHECK_LAUNCH();
    OPENB_TRY(weight_grad(stream, d_o, C, x, C, RX, C, C, part_w, dparams + OPENB_OFF_Q_PROJ, acc));                              // 21
    OPENB_TRY(weight_grad(stream, kv, HID, source, C, RS, HID, C, part_w, dparams + OPENB_OFF_K_PROJ, acc));                      // 22
    OPENB_TRY(gemm(stream, true, d_o, C, Wq, C, dx, C, RX, C, C, EPI_ADD2, dy, C, hc, HID));                                      // 23
    OPENB_TRY(gemm(stream, true, kv, HID, Wkv, C, dsource, C, RS, C, HID, EPI_NONE));                                             // 24
    ln_params_kernel<<<2, kThreads, 0, stream>>>(f(l.ln1), blocks, dparams + OPENB_OFF_NORM1_WEIGHT, acc);                        // 25
    CAPI_CHECK_LAUNCH();
    ln_params_kernel<<<2, kThreads, 0, stream>>>(f(l.ln2), blocks, dparams + OPENB_OFF_NORM2_WEIGHT, acc);
    CAPI_CHECK_LAUNCH();
    return 0;
}

}  // extern "C"
