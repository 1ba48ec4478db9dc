// LoFTR's optimal-transport coarse matching (loftr/utils/coarse_matching.py, match_type 'sinkhorn', inference) with SuperGlue's
// log_optimal_transport, between the coarse grids of two images.  m = N rows (image 0), n = M columns (image 1):
//   S = <f0 / sqrt(C), f1 / sqrt(C)>  (no temperature);  Z = [[S, a 1_m], [a 1_n^T, a]]  (a = bin_score: the dustbin row and column)
//   norm = -log(m + n), log_mu = [norm x m, log n + norm], log_nu = [norm x n, log m + norm], u = v = 0, then `iters` times
//     u = log_mu - logsumexp(Z + v[None, :], dim=1);  v = log_nu - logsumexp(Z + u[:, None], dim=0)
//   assign = exp(((Z + u[:, None]) + v[None, :]) - norm),  conf_matrix = assign[:-1, :-1]
//   prefilter: rows whose argmax over j (bin included) is the dustbin, and columns whose argmax over i is the dustbin, are zeroed;
//   argmax takes the first maximum and the dustbin is last, so it wins only when its exp'd f32 value is strictly greater.
//
// Launch chain (deterministic: no float atomics, every cross-workgroup reduction is a fixed-order combine):
//   ophip_coarse_sim_store  (csrc/coarse_match.hip) fragment planes + similarity tiles: S into conf once, the tiles' row (max, sum exp)
//                           merged -- the first u update (v = 0) without a sweep
//   skh_rows     one wave per row: u_i from a dwordx4 sweep of row i of S with v from L2; the dustbin row's u from v alone
//   skh_cols     a workgroup per (256-column strip, 128-row chunk): (max, sum exp) of S_ij + u_i per column and chunk
//   skh_colcomb  8 lanes per column merge the chunks in a fixed order: v_j, and on the last update the column prefilter from the exact
//                max_i (S_ij + u_i); one workgroup computes the dustbin column's v from u alone
//   skh_final    one wave per row: a first read decides the row prefilter, a second writes the confidences (a filtered row: zeros, no
//                read) with the row's best candidate above the threshold and the column maxima in the records select_decide reads
//   select       ophip_coarse_select_2d: threshold, border on all sides, mutual test, first-j ties, ordered compaction
// HBM passes over the N x M matrix for 3 iterations with the prefilter: S written once, 5 sweeps, 2 reads + 1 write at the end = 9.
#include "tile.h"
#include "onepose_hip.h"
#include "x3w8_internal.h"
#include <math.h>

namespace {

constexpr int SKH_CR = 128;           // rows per column-sweep chunk (32 per wave)
constexpr int SKH_RB = 8;             // rows per column-sweep batch / float4 groups per lane and row-sweep step

__device__ __forceinline__ float skh_exp(float x) { return __expf(x); }

// (m, s) += the K values x: one exponential per value, one rescale per batch
template <int K>
__device__ __forceinline__ void lse_batch(float& m, float& s, const float (&x)[K]) {
    float mx = x[0];
#pragma unroll
    for (int k = 1; k < K; ++k) mx = fmaxf(mx, x[k]);
    const float mn = fmaxf(m, mx);
    if (mn == -INFINITY) return;
    float acc = 0.f;
#pragma unroll
    for (int k = 0; k < K; ++k) acc += skh_exp(x[k] - mn);
    s = s * skh_exp(m - mn) + acc;
    m = mn;
}

__device__ __forceinline__ void lse_merge(float& m, float& s, float m2, float s2) {
    const float mm = fmaxf(m, m2);
    if (mm == -INFINITY) { m = mm; s = 0.f; return; }
    s = s * expf(m - mm) + s2 * expf(m2 - mm);
    m = mm;
}

// over the 64 lanes, the lower lane's value first on both sides of every step: a fixed order, the result in every lane
__device__ __forceinline__ void lse_wave(float& m, float& s) {
    const int lane = threadIdx.x & 63;
#pragma unroll
    for (int o = 1; o < 64; o <<= 1) {
        const float m2 = __shfl_xor(m, o, 64), s2 = __shfl_xor(s, o, 64);
        float ma = m, sa = s, mb = m2, sb = s2;
        if (lane & o) { ma = m2; sa = s2; mb = m; sb = s; }
        lse_merge(ma, sa, mb, sb);
        m = ma; s = sa;
    }
}

struct SkhArgs {
    const float* S;           // [B][N][M]: the conf buffer holding S until skh_final
    float* u;                 // [B][up]  u_0 .. u_{N-1}, dustbin u_N
    float* v;                 // [B][vp]  v_0 .. v_{M-1}, dustbin v_M (vp % 4 == 0: float4 reads of v)
    const float* rowstat;     // [B][N][2] merged (max, sum exp) of the similarity tiles' rows (first row update)
    float* colpart;           // [B][nchunk][M][2] (max, sum exp) of S_ij + u_i per row chunk
    unsigned char* filt1;     // [B][M] column prefilter (1: the dustbin row wins column j)
    int N, M, up, vp, nchunk;
    float alpha, norm, logmu_bin, lognu_bin;
};

// u update.  Wave w of block x owns row i = 4x + w (i == N: the dustbin row, Z = alpha in every column, bin included).
// FROM_STATS: the first update (v = 0): logsumexp_j S_ij is the merged tile statistics.
template <bool VEC, bool FROM_STATS>
__global__ __launch_bounds__(256) void skh_rows_kernel(SkhArgs p) {
    const int lane = threadIdx.x & 63, b = blockIdx.y;
    const int i = 4 * blockIdx.x + (threadIdx.x >> 6);
    if (i > p.N) return;
    const float* vb = p.v + (size_t)b * p.vp;
    float m = -INFINITY, s = 0.f;
    if (i == p.N) {
        for (int j0 = 0; j0 <= p.M; j0 += 64 * SKH_RB) {
            float x[SKH_RB];
#pragma unroll
            for (int k = 0; k < SKH_RB; ++k) {
                const int j = j0 + 64 * k + lane;
                x[k] = j <= p.M ? p.alpha + vb[j] : -INFINITY;
            }
            lse_batch(m, s, x);
        }
    } else if (FROM_STATS) {
        if (lane == 0) { m = p.rowstat[((size_t)b * p.N + i) * 2]; s = p.rowstat[((size_t)b * p.N + i) * 2 + 1]; }
    } else {
        const float* row = p.S + ((size_t)b * p.N + i) * p.M;
        if (VEC) {
            for (int j0 = 0; j0 < p.M; j0 += 256 * SKH_RB) {
                f32x4 sv[SKH_RB], vv[SKH_RB];
#pragma unroll
                for (int k = 0; k < SKH_RB; ++k) {
                    const int j = j0 + 256 * k + 4 * lane;
                    if (j < p.M) {
                        sv[k] = *reinterpret_cast<const f32x4*>(row + j);
                        vv[k] = *reinterpret_cast<const f32x4*>(vb + j);
                    }
                }
                float x[4 * SKH_RB];
#pragma unroll
                for (int k = 0; k < SKH_RB; ++k) {
                    const bool in = j0 + 256 * k + 4 * lane < p.M;
#pragma unroll
                    for (int e = 0; e < 4; ++e) x[4 * k + e] = in ? sv[k][e] + vv[k][e] : -INFINITY;
                }
                lse_batch(m, s, x);
            }
        } else {
            for (int j0 = 0; j0 < p.M; j0 += 64 * SKH_RB) {
                float x[SKH_RB];
#pragma unroll
                for (int k = 0; k < SKH_RB; ++k) {
                    const int j = j0 + 64 * k + lane;
                    x[k] = j < p.M ? row[j] + vb[j] : -INFINITY;
                }
                lse_batch(m, s, x);
            }
        }
    }
    lse_wave(m, s);
    if (lane == 0) {
        if (i < p.N) lse_merge(m, s, p.alpha + vb[p.M], 1.f);          // the dustbin column
        p.u[(size_t)b * p.up + i] = (i < p.N ? p.norm : p.logmu_bin) - (m + logf(s));
    }
}

// column partials: block (strip, chunk, b); lane l of wave w owns columns 256 strip + 4l .. + 3 over rows 128 chunk + 32 w .. + 31
template <bool VEC>
__global__ __launch_bounds__(256) void skh_cols_kernel(SkhArgs p) {
    __shared__ float red[4][256][2];
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6, b = blockIdx.z;
    const int jq = 256 * blockIdx.x + 4 * lane;
    const int r0 = SKH_CR * blockIdx.y + (SKH_CR / 4) * wave;
    const float* Sb = p.S + (size_t)b * p.N * p.M;
    const float* ub = p.u + (size_t)b * p.up;
    float m[4] = {-INFINITY, -INFINITY, -INFINITY, -INFINITY}, s[4] = {0.f, 0.f, 0.f, 0.f};
    for (int rb = 0; rb < SKH_CR / 4; rb += SKH_RB) {
        float x[4][SKH_RB];
#pragma unroll
        for (int q = 0; q < SKH_RB; ++q) {
            const int i = r0 + rb + q;
            const bool row_in = i < p.N;
            const float ui = row_in ? ub[i] : 0.f;
            const float* row = Sb + (size_t)(row_in ? i : 0) * p.M;
            if (VEC) {
                f32x4 sv = {0.f, 0.f, 0.f, 0.f};
                if (row_in && jq < p.M) sv = *reinterpret_cast<const f32x4*>(row + jq);
#pragma unroll
                for (int e = 0; e < 4; ++e) x[e][q] = (row_in && jq < p.M) ? sv[e] + ui : -INFINITY;
            } else {
#pragma unroll
                for (int e = 0; e < 4; ++e) x[e][q] = (row_in && jq + e < p.M) ? row[jq + e] + ui : -INFINITY;
            }
        }
#pragma unroll
        for (int e = 0; e < 4; ++e) lse_batch(m[e], s[e], x[e]);
    }
#pragma unroll
    for (int e = 0; e < 4; ++e) { red[wave][4 * lane + e][0] = m[e]; red[wave][4 * lane + e][1] = s[e]; }
    __syncthreads();
    const int j = 256 * blockIdx.x + tid;
    if (j < p.M) {
        float mm = red[0][tid][0], ss = red[0][tid][1];
#pragma unroll
        for (int w = 1; w < 4; ++w) lse_merge(mm, ss, red[w][tid][0], red[w][tid][1]);
        float* o = p.colpart + (((size_t)b * p.nchunk + blockIdx.y) * p.M + j) * 2;
        o[0] = mm; o[1] = ss;
    }
}

// v update (update_v) and / or the column prefilter (filter) from the chunk partials; 8 lanes per column (lane q merges chunks q, q + 8,
// ... in order, then a butterfly with the lower lane first).  The last block: the dustbin column's v from u alone.
__global__ __launch_bounds__(256) void skh_colcomb_kernel(SkhArgs p, int update_v, int filter) {
    const int tid = threadIdx.x, b = blockIdx.y;
    const float* ub = p.u + (size_t)b * p.up;
    float* vb = p.v + (size_t)b * p.vp;
    if (blockIdx.x == gridDim.x - 1) {
        if (!update_v) return;
        __shared__ float wred[4][2];
        float m = -INFINITY, s = 0.f;
        for (int i0 = 0; i0 <= p.N; i0 += 256 * 4) {
            float x[4];
#pragma unroll
            for (int k = 0; k < 4; ++k) {
                const int i = i0 + 256 * k + tid;
                x[k] = i <= p.N ? p.alpha + ub[i] : -INFINITY;
            }
            lse_batch(m, s, x);
        }
        lse_wave(m, s);
        if ((tid & 63) == 0) { wred[tid >> 6][0] = m; wred[tid >> 6][1] = s; }
        __syncthreads();
        if (tid == 0) {
            m = wred[0][0]; s = wred[0][1];
            for (int w = 1; w < 4; ++w) lse_merge(m, s, wred[w][0], wred[w][1]);
            vb[p.M] = p.lognu_bin - (m + logf(s));
        }
        return;
    }
    const int j = 32 * blockIdx.x + (tid >> 3), q = tid & 7;
    const bool live = j < p.M;
    float m = -INFINITY, s = 0.f;
    if (live)
        for (int t = q; t < p.nchunk; t += 8) {
            const float* c = p.colpart + (((size_t)b * p.nchunk + t) * p.M + j) * 2;
            lse_merge(m, s, c[0], c[1]);
        }
#pragma unroll
    for (int o = 1; o < 8; o <<= 1) {
        const float m2 = __shfl_xor(m, o, 64), s2 = __shfl_xor(s, o, 64);
        float ma = m, sa = s, mb = m2, sb = s2;
        if (q & o) { ma = m2; sa = s2; mb = m; sb = s; }
        lse_merge(ma, sa, mb, sb);
        m = ma; s = sa;
    }
    if (!live || q != 0) return;
    const float smax = m;                                 // exact max_i (S_ij + u_i): the partials' maxima are exact
    const float ubin = ub[p.N];
    float vj = vb[j];
    if (update_v) {
        lse_merge(m, s, p.alpha + ubin, 1.f);             // the dustbin row
        vj = p.norm - (m + logf(s));
        vb[j] = vj;
    }
    if (filter) {
        // argmax over i of exp(((Z_ij + u_i) + v_j) - norm), bin last: f32 addition and exp are monotone, so the real rows' maximum is
        // that of max_i (S_ij + u_i)
        const float real = skh_exp((smax + vj) - p.norm);
        const float bin = skh_exp(((p.alpha + ubin) + vj) - p.norm);
        p.filt1[(size_t)b * p.M + j] = bin > real ? 1 : 0;
    }
}

struct SkhFinalArgs {
    float* conf;              // [B][N][M]: S in, confidences out
    float* rowbest;           // [B][1][N][3] (value, j as float bits, tie count as float bits) -- select_decide's records
    unsigned* colmax_bits;    // [B][M] column maxima of the candidates (cleared by stat_combine)
    float thr;
    int prefilter;
};

// one wave per row: (prefilter) max_j of ((S_ij + u_i) + v_j) against the dustbin column decides the row; then the confidences
template <bool VEC>
__global__ __launch_bounds__(256) void skh_final_kernel(SkhArgs p, SkhFinalArgs f) {
    const int lane = threadIdx.x & 63, b = blockIdx.y;
    const int i = 4 * blockIdx.x + (threadIdx.x >> 6);
    if (i >= p.N) return;
    const float* vb = p.v + (size_t)b * p.vp;
    const unsigned char* fb = p.filt1 + (size_t)b * p.M;
    const float ui = p.u[(size_t)b * p.up + i];
    float* row = f.conf + ((size_t)b * p.N + i) * p.M;
    bool zero_row = false;
    if (f.prefilter) {
        float tmax = -INFINITY;
        if (VEC) {
            for (int j0 = 0; j0 < p.M; j0 += 256 * SKH_RB) {
                f32x4 sv[SKH_RB], vv[SKH_RB];
#pragma unroll
                for (int k = 0; k < SKH_RB; ++k) {
                    const int j = j0 + 256 * k + 4 * lane;
                    if (j < p.M) {
                        sv[k] = *reinterpret_cast<const f32x4*>(row + j);
                        vv[k] = *reinterpret_cast<const f32x4*>(vb + j);
                    }
                }
#pragma unroll
                for (int k = 0; k < SKH_RB; ++k)
                    if (j0 + 256 * k + 4 * lane < p.M)
#pragma unroll
                        for (int e = 0; e < 4; ++e) tmax = fmaxf(tmax, (sv[k][e] + ui) + vv[k][e]);
            }
        } else {
            for (int j = lane; j < p.M; j += 64) tmax = fmaxf(tmax, (row[j] + ui) + vb[j]);
        }
        tmax = wave_max(tmax);
        zero_row = skh_exp(((p.alpha + ui) + vb[p.M]) - p.norm) > skh_exp(tmax - p.norm);
    }
    float bv = -1.f;
    int bj = 0x7fffffff, bc = 0;
    unsigned* cb = f.colmax_bits + (size_t)b * p.M;
    auto track = [&](float c, int j) {
        if (c > f.thr) {
            atomicMax(cb + j, __float_as_uint(c));
            if (c > bv) { bv = c; bj = j; bc = 1; }
            else if (c == bv) { bc += 1; bj = min(bj, j); }
        }
    };
    if (VEC) {
        for (int j0 = 0; j0 < p.M; j0 += 256 * SKH_RB) {
            f32x4 sv[SKH_RB], vv[SKH_RB];
            if (!zero_row) {
#pragma unroll
                for (int k = 0; k < SKH_RB; ++k) {
                    const int j = j0 + 256 * k + 4 * lane;
                    if (j < p.M) {
                        sv[k] = *reinterpret_cast<const f32x4*>(row + j);
                        vv[k] = *reinterpret_cast<const f32x4*>(vb + j);
                    }
                }
            }
#pragma unroll
            for (int k = 0; k < SKH_RB; ++k) {
                const int j = j0 + 256 * k + 4 * lane;
                if (j >= p.M) continue;
                f32x4 c = {0.f, 0.f, 0.f, 0.f};
                if (!zero_row) {
#pragma unroll
                    for (int e = 0; e < 4; ++e) {
                        const bool cut = f.prefilter && fb[j + e];
                        c[e] = cut ? 0.f : skh_exp(((sv[k][e] + ui) + vv[k][e]) - p.norm);
                        track(c[e], j + e);
                    }
                }
                __builtin_nontemporal_store(c, reinterpret_cast<f32x4*>(row + j));
            }
        }
    } else {
        for (int j = lane; j < p.M; j += 64) {
            float c = 0.f;
            if (!zero_row && !(f.prefilter && fb[j])) {
                c = skh_exp(((row[j] + ui) + vb[j]) - p.norm);
                track(c, j);
            }
            row[j] = c;
        }
    }
    // wave reduce: max value, lowest j among the maxima, number of maxima (conf_kernel's record)
    const float wv = wave_max(bv);
    int cj = (bv == wv) ? bj : 0x7fffffff;
    int cc = (bv == wv) ? bc : 0;
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) {
        cj = min(cj, __shfl_xor(cj, o, 64));
        cc += __shfl_xor(cc, o, 64);
    }
    if (lane == 0) {
        float* o = f.rowbest + ((size_t)b * p.N + i) * 3;
        o[0] = wv; o[1] = __int_as_float(cj); o[2] = __int_as_float(cc);
    }
}

struct SkhWs {
    size_t u, v, colpart, filt1, total;
    int up, vp, nchunk;
};
SkhWs skh_ws(int B, int N, int M) {
    SkhWs w;
    w.up = (N + 1 + 3) / 4 * 4;
    w.vp = (M + 1 + 3) / 4 * 4;
    w.nchunk = (N + SKH_CR - 1) / SKH_CR;
    size_t f = 0;
    w.u = f; f += (size_t)B * w.up;
    w.v = f; f += (size_t)B * w.vp;
    w.colpart = f; f += (size_t)B * w.nchunk * M * 2;
    w.filt1 = f; f += ((size_t)B * M + 3) / 4;
    w.total = f + 16;                                  // + alignment of the region's start to 64 bytes
    return w;
}

}  // namespace

extern "C" size_t ophip_coarse_sinkhorn_workspace_floats(int B, int L0, int L1) {
    if (B < 1 || L0 < 1 || L1 < 1) return 0;
    return ophip_coarse_workspace_floats(B, L0, L1) + skh_ws(B, L0, L1).total;
}

namespace {
int sinkhorn_impl(const float* feat0, const float* feat1, const float* points0, long long points_bstride,
                  int B, int L0, int L1, int w0c, int w1c, float bin_score, int iters, int prefilter,
                  float thr, int border_rm, float scale, float* conf, float* workspace,
                  long long* b_ids, long long* i_ids, long long* j_ids, float* mconf, float* mkpts0,
                  float* mkpts1_c, long long* m_bids, unsigned char* gt_mask, int* count, void* stream_,
                  const unsigned char* mask0, const unsigned char* mask1) {
    if (!feat0 || !feat1 || !points0 || !conf || !workspace || !b_ids || !i_ids || !j_ids || !mconf || !mkpts0 || !mkpts1_c || !count)
        return ophip_bad_arg(__func__, "null pointer (conf is required)");
    if (reinterpret_cast<uintptr_t>(workspace) & 15) return ophip_bad_arg(__func__, "workspace must be 16-byte aligned");
    if (B < 1 || L0 < 1 || L1 < 1 || w0c < 1 || w1c < 1 || L0 % w0c != 0 || L1 % w1c != 0)
        return ophip_bad_arg(__func__, "bad sizes (need L0 == h0c * w0c, L1 == h1c * w1c)");
    if (iters < 0) return ophip_bad_arg(__func__, "iters must be >= 0");
    if (prefilter != 0 && prefilter != 1) return ophip_bad_arg(__func__, "prefilter must be 0 or 1");
    if (!(bin_score - bin_score == 0.f)) return ophip_bad_arg(__func__, "bin_score must be finite");
    hipStream_t stream = (hipStream_t)stream_;
    const int N = L0, M = L1;
    const SkhWs sw = skh_ws(B, N, M);
    float* base = workspace + ophip_coarse_workspace_floats(B, N, M);
    base += (16 - ((reinterpret_cast<uintptr_t>(base) >> 2) & 15)) & 15;

    const float* rowstat;
    float* rowbest;
    unsigned* colmax_bits;
    if (int rc = ophip_coarse_sim_store(feat0, feat1, B, N, M, conf, workspace, &rowstat, &rowbest, &colmax_bits, stream, mask0, mask1)) return rc;

    // the reference's f32 marginals: norm = -log(m + n), log_mu = [norm x m, log n + norm], log_nu = [norm x n, log m + norm]
    const float fm = (float)N, fn = (float)M;
    const float norm = -logf(fm + fn);
    SkhArgs a{conf, base + sw.u, base + sw.v, rowstat, base + sw.colpart, reinterpret_cast<unsigned char*>(base + sw.filt1),
              N, M, sw.up, sw.vp, sw.nchunk, bin_score, norm, logf(fn) + norm, logf(fm) + norm};
    if (hipError_t e = hipMemsetAsync(a.v, 0, sizeof(float) * B * sw.vp, stream)) return ophip_fail(e, __func__);
    if (iters == 0)
        if (hipError_t e = hipMemsetAsync(a.u, 0, sizeof(float) * B * sw.up, stream)) return ophip_fail(e, __func__);
    const bool vec = M % 4 == 0;
    const dim3 rows_grid((N + 1 + 3) / 4, B), cols_grid((M + 255) / 256, sw.nchunk, B), comb_grid((M + 31) / 32 + 1, B);
    auto col_update = [&](int update_v, int filter) -> int {
        if (vec) OPHIP_LAUNCH("skh_cols", stream, skh_cols_kernel<true>, cols_grid, dim3(256), 0, stream, a);
        else OPHIP_LAUNCH("skh_cols", stream, skh_cols_kernel<false>, cols_grid, dim3(256), 0, stream, a);
        OPHIP_CHECK_LAUNCH();
        OPHIP_LAUNCH("skh_colcomb", stream, skh_colcomb_kernel, comb_grid, dim3(256), 0, stream, a, update_v, filter);
        OPHIP_CHECK_LAUNCH();
        return 0;
    };
    for (int it = 0; it < iters; ++it) {
        if (it == 0) OPHIP_LAUNCH("skh_rows", stream, (skh_rows_kernel<true, true>), rows_grid, dim3(256), 0, stream, a);
        else if (vec) OPHIP_LAUNCH("skh_rows", stream, (skh_rows_kernel<true, false>), rows_grid, dim3(256), 0, stream, a);
        else OPHIP_LAUNCH("skh_rows", stream, (skh_rows_kernel<false, false>), rows_grid, dim3(256), 0, stream, a);
        OPHIP_CHECK_LAUNCH();
        if (int rc = col_update(1, prefilter && it == iters - 1)) return rc;
    }
    if (iters == 0 && prefilter)
        if (int rc = col_update(0, 1)) return rc;                  // u = v = 0: the column prefilter still needs max_i S_ij

    SkhFinalArgs fa{conf, rowbest, colmax_bits, thr, prefilter};
    const dim3 fin_grid((N + 3) / 4, B);
    if (vec) OPHIP_LAUNCH("skh_final", stream, skh_final_kernel<true>, fin_grid, dim3(256), 0, stream, a, fa);
    else OPHIP_LAUNCH("skh_final", stream, skh_final_kernel<false>, fin_grid, dim3(256), 0, stream, a, fa);
    OPHIP_CHECK_LAUNCH();
    return ophip_coarse_select_2d(conf, 1, points0, points_bstride, B, N, M, w0c, w1c, thr, border_rm, scale, workspace,
                                  b_ids, i_ids, j_ids, mconf, mkpts0, mkpts1_c, m_bids, gt_mask, count, stream, mask0, mask1);
}
}  // namespace

extern "C" int ophip_coarse_match_2d_sinkhorn(const float* feat0, const float* feat1, const float* points0, long long points_bstride,
                                              int B, int L0, int L1, int w0c, int w1c, float bin_score, int iters, int prefilter,
                                              float thr, int border_rm, float scale, float* conf, float* workspace,
                                              long long* b_ids, long long* i_ids, long long* j_ids, float* mconf, float* mkpts0,
                                              float* mkpts1_c, long long* m_bids, unsigned char* gt_mask, int* count, void* stream) {
    return sinkhorn_impl(feat0, feat1, points0, points_bstride, B, L0, L1, w0c, w1c, bin_score, iters, prefilter, thr, border_rm, scale,
                         conf, workspace, b_ids, i_ids, j_ids, mconf, mkpts0, mkpts1_c, m_bids, gt_mask, count, stream, nullptr, nullptr);
}

// ophip_coarse_match_2d_sinkhorn with LoFTR's padding masks mask0 [B][L0] / mask1 [B][L1] (1 = real cell; both required): S =
// <f0, f1> / C with S.masked_fill_(~(mask0[:, :, None] & mask1[:, None, :]), -1e9) in the similarity tiles, then the unchanged
// log_optimal_transport -- its norm = -log(m + n) and dustbin masses use the PADDED m = L0, n = L1, so the output is not invariant under
// padding (the reference's behaviour) -- and the prefilter; the selection's border follows each pair's valid extent (mask_border_with_padding,
// as ophip_coarse_match_2d_masked).
extern "C" int ophip_coarse_match_2d_sinkhorn_masked(const float* feat0, const float* feat1, const float* points0, long long points_bstride,
                                                     int B, int L0, int L1, int w0c, int w1c, float bin_score, int iters, int prefilter,
                                                     float thr, int border_rm, float scale, float* conf, float* workspace,
                                                     long long* b_ids, long long* i_ids, long long* j_ids, float* mconf, float* mkpts0,
                                                     float* mkpts1_c, long long* m_bids, unsigned char* gt_mask, int* count,
                                                     const unsigned char* mask0, const unsigned char* mask1, void* stream) {
    if (!mask0 || !mask1) return ophip_bad_arg(__func__, "null mask (use ophip_coarse_match_2d_sinkhorn)");
    return sinkhorn_impl(feat0, feat1, points0, points_bstride, B, L0, L1, w0c, w1c, bin_score, iters, prefilter, thr, border_rm, scale,
                         conf, workspace, b_ids, i_ids, j_ids, mconf, mkpts0, mkpts1_c, m_bids, gt_mask, count, stream, mask0, mask1);
}
