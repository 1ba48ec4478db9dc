// The backward of the training loss down to the matcher's feature boundaries (include/ext/onepose_loss_backward.h).
// The header is the specification: the formulas, every pass and every sum order.
//
// count_kernel       one workgroup: n_pos by an integer tree, the two weights times the caller's scale.
// planes_kernel      one wave per 1 KiB fragment pair: feat / 16 as (hi, lo) bf16 in the S layout (the forward's frag_planes_kernel) and in
//                    the transposed layout of the gradient product; the first wave of a tile also writes the tile's ground-truth row and
//                    the zeros of the statistics' padding.
// sweep_kernel<MODE> the owned-row kernel in two roles: a wave keeps the fragments of its 32 owned rows in registers, the workgroup streams
//                    the other side's 32-row tiles through two LDS buffers by LDS-DMA (one 1 KiB fragment per wave-instruction, lane-linear
//                    image: conflict-free ds_read_b128); the transposed S tile puts the swept index on the accumulator's ROW, so dS is the A
//                    operand of the second product without an LDS trip (tile_bf16.h, lines 16-18).
//                    MODE 0: lr / lc.  MODE 1: r / c.  MODE 2: grad0 / grad1.
// fine_grads_kernel  one wave per match in float64; the bookkeeping of opsup_fine_loss recomputed by every workgroup in its order.
// No float atomics, no cross-workgroup float sum: an owned row's sums are taken by its two lanes in ascending tile order.
#include "tile_bf16.h"
#include "capi_error.h"
#include "device_loop.h"
#include "ext/onepose_loss_backward.h"
#include "reduce_f64.h"
#include <math.h>

#pragma clang fp contract(off)

namespace {

using capi::bad_arg;
using capi::blocks_of;
using devloop::align_up;
using devloop::clamped_count;

constexpr int kThreads = OPBWD_BLOCK, C = OPBWD_CHANNELS, CF = OPBWD_FINE_CHANNELS, R = OPBWD_OWNED_ROWS, SW = OPBWD_SWEPT_ROWS;
static_assert(kThreads == 256 && R == 4 * 32 && SW == 32 && C == 256 && CF == 128, "the kernels are written for these");
constexpr int TILE_BYTES = SW * C * 2 * 2;                      // one 32-row tile in one layout: (hi, lo) bf16 of 256 channels = 32 KiB
constexpr int STAT_BYTES = 3 * 256;                             // lse, usum, gt of 64 rows from the tile's first
constexpr float kLo = 1e-6f, kHi = (float)(1.0 - 1e-6);

struct Layout {
    size_t sp[2], tp[2], lse[2], usum[2], gt[2], consts, total;
    int tiles[2];
};

// side 0: feat0 (N rows), side 1: feat1 (M rows); the statistics of a frame are 32 * tiles + 32 entries apart (a DMA reads 64 from a tile's first)
Layout layout_of(int B, int N, int M) {
    Layout l;
    const int rows[2] = {N, M};
    size_t at = 0;
    for (int s = 0; s < 2; ++s) {
        l.tiles[s] = (rows[s] + SW - 1) / SW;
        const size_t planes = (size_t)B * l.tiles[s] * TILE_BYTES, stats = align_up((size_t)B * (SW * l.tiles[s] + SW) * 4);
        l.sp[s] = at; at += planes;
        l.tp[s] = at; at += planes;
        l.lse[s] = at; at += stats;
        l.usum[s] = at; at += stats;
        l.gt[s] = at; at += stats;
    }
    l.consts = at; at += 256;
    l.total = at;
    return l;
}

__global__ __launch_bounds__(kThreads) void count_kernel(const long long* __restrict__ gt_j, long long rows, int M, long long per_batch,
                                                         double pos_weight, double neg_weight, double scale, float* __restrict__ consts) {
    __shared__ long long cnt[kThreads];
    const int tid = threadIdx.x;
    long long n = 0;
    for (long long r = tid; r < rows; r += kThreads) {
        const long long gj = gt_j[r];
        n += (gj >= 0 && gj < M) ? 1 : 0;
    }
    cnt[tid] = n;
    __syncthreads();
    for (int s = kThreads / 2; s > 0; s >>= 1) {
        if (tid < s) cnt[tid] += cnt[tid + s];
        __syncthreads();
    }
    if (tid != 0) return;
    const long long n_pos = cnt[0], n_neg = per_batch - n_pos;
    const double wpos = n_pos > 0 ? pos_weight / (double)n_pos : 0.0, wneg = n_neg > 0 ? neg_weight / (double)n_neg : 0.0;
    consts[0] = (float)(scale * wpos);
    consts[1] = (float)(scale * wneg);
}

struct PlaneArgs {
    const float* x[2];          // [B][rows][256]
    const long long* gt_j;      // [B][N]
    char* sp[2];
    char* tp[2];
    float* lse[2];
    float* usum[2];
    int* gt[2];
    int rows[2], tiles[2];
};

// block (8 per tile): wave job 4 * (blockIdx.x & 7) + wave; jobs 0..15 are the S fragments (k-step = job), 16..31 the transposed ones
__global__ __launch_bounds__(kThreads) void planes_kernel(PlaneArgs p) {
    const int b = blockIdx.y, lane = threadIdx.x & 63, wave = threadIdx.x >> 6, r = lane & 31, h = lane >> 5;
    int T = blockIdx.x >> 3;
    const int side = T >= p.tiles[0];
    if (side) T -= p.tiles[0];
    const int job = 4 * (blockIdx.x & 7) + wave, rows = p.rows[side], tiles = p.tiles[side];
    const float* x = p.x[side] + (size_t)b * rows * C;
    bf16x8 vh, vl;
    char* dst;
    if (job < 16) {
        const int row = SW * T + r, k0 = 16 * job + 8 * h;
        const f32x4 z = {0.f, 0.f, 0.f, 0.f};
        const f32x4 v0 = row < rows ? *reinterpret_cast<const f32x4*>(x + (size_t)row * C + k0) : z;
        const f32x4 v1 = row < rows ? *reinterpret_cast<const f32x4*>(x + (size_t)row * C + k0 + 4) : z;
#pragma unroll
        for (int j = 0; j < 4; ++j) {
            __bf16 hh, ll;
            split_bf16(v0[j] * 0.0625f, hh, ll); vh[j] = hh; vl[j] = ll;          // feat / sqrt(C): an exact power of two
            split_bf16(v1[j] * 0.0625f, hh, ll); vh[4 + j] = hh; vl[4 + j] = ll;
        }
        dst = p.sp[side] + ((size_t)b * tiles + T) * TILE_BYTES + (size_t)(2 * job) * 1024 + 16 * lane;
    } else {
        const int s = (job - 16) >> 3, ct = (job - 16) & 7, ch = 32 * ct + r;
#pragma unroll
        for (int e = 0; e < 8; ++e) {
            const int row = SW * T + 16 * s + 8 * (e >> 2) + 4 * h + (e & 3);
            __bf16 hh, ll;
            split_bf16(row < rows ? x[(size_t)row * C + ch] * 0.0625f : 0.f, hh, ll);
            vh[e] = hh; vl[e] = ll;
        }
        dst = p.tp[side] + ((size_t)b * tiles + T) * TILE_BYTES + (size_t)(2 * (job - 16)) * 1024 + 16 * lane;
    }
    *reinterpret_cast<bf16x8*>(dst) = vh;
    *reinterpret_cast<bf16x8*>(dst + 1024) = vl;
    if (job != 0) return;
    // the tile's statistics rows: the ground truth (side 0; none: -1) and zeros where no sweep will write; the last tile also owns the 32
    // entries behind the padded rows
    const size_t base = (size_t)b * (SW * tiles + SW);
    for (int e = lane; e < (T == tiles - 1 ? 2 * SW : SW); e += 64) {
        const int row = SW * T + e;
        int g = -1;
        if (side == 0 && row < rows) {
            const long long gj = p.gt_j[(size_t)b * rows + row];
            g = (gj >= 0 && gj < p.rows[1]) ? (int)gj : -1;
        }
        p.gt[side][base + row] = g;
        if (row >= rows) {
            p.lse[side][base + row] = 0.f;
            p.usum[side][base + row] = 0.f;
        }
    }
}

struct SweepArgs {
    const char* sp[2];
    const char* tp[2];
    float* lse[2];
    float* usum[2];
    const int* gt[2];
    float* grad[2];
    int rows[2], tiles[2], nblk0;       // nblk0: the blocks that own rows of side 0 (they come first)
    float inv_t, out_scale, alpha, gamma;
    const float* consts;
};

__device__ __forceinline__ float focal_p(float v, float gamma) { return gamma == 2.0f ? v * v : powf(v, gamma); }
__device__ __forceinline__ float focal_q(float v, float gamma) { return gamma == 2.0f ? v : powf(v, gamma - 1.0f); }

// d loss / d conf times the weight, for a confidence inside the clamp's bounds
__device__ __forceinline__ float focal_grad(float c, bool pos, float wpos, float wneg, float alpha, float gamma) {
    if (pos) {
        const float v = 1.0f - c;
        return wpos * (alpha * gamma * focal_q(v, gamma) * logf(c) - alpha * focal_p(v, gamma) / c);
    }
    return wneg * (-(1.0f - alpha) * (gamma * focal_q(c, gamma) * log1pf(-c) - focal_p(c, gamma) / (1.0f - c)));
}

template <int MODE>
constexpr int buf_bytes() { return (MODE == 2 ? 2 : 1) * TILE_BYTES + STAT_BYTES; }

template <int MODE>
__global__ __launch_bounds__(kThreads) OPHIP_WAVES_PER_SIMD(1, 1) void sweep_kernel(SweepArgs p) {
    extern __shared__ __attribute__((aligned(16))) char smem[];
    constexpr int BUF = buf_bytes<MODE>();
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6, r = lane & 31, h = lane >> 5, b = blockIdx.y;
    const int role = (int)blockIdx.x >= p.nblk0, own = role, swp = 1 - role;
    const int blk = (int)blockIdx.x - (role ? p.nblk0 : 0);
    const int own_rows = p.rows[own], sw_rows = p.rows[swp], own_tiles = p.tiles[own], sw_tiles = p.tiles[swp];
    const bool live = 4 * blk + wave < own_tiles;                  // a wave past the last tile takes part in the staging only
    const int To = live ? 4 * blk + wave : own_tiles - 1;
    const int i = SW * To + r;                                      // this lane's owned row
    const size_t own_stat = (size_t)b * (SW * own_tiles + SW), sw_stat = (size_t)b * (SW * sw_tiles + SW);

    const char* g_sp = p.sp[swp] + (size_t)b * sw_tiles * TILE_BYTES + (size_t)(8 * wave) * 1024 + 16 * lane;
    const char* g_tp = p.tp[swp] + (size_t)b * sw_tiles * TILE_BYTES + (size_t)(8 * wave) * 1024 + 16 * lane;
    const float* g_lse = p.lse[swp] + sw_stat + lane;
    const float* g_usum = p.usum[swp] + sw_stat + lane;
    const int* g_gt = p.gt[swp] + sw_stat + lane;
    // tile t into buffer buf: each wave 8 (MODE 2: 16) fragments of 1 KiB; wave 0 also the 64 statistics entries from the tile's first row
    auto issue = [&](int t, int buf) {
        char* dst = smem + buf * BUF + (8 * wave) * 1024;
#pragma unroll
        for (int f = 0; f < 8; ++f)
            __builtin_amdgcn_global_load_lds((const __attribute__((address_space(1))) void*)(g_sp + (size_t)t * TILE_BYTES + f * 1024),
                                             (__attribute__((address_space(3))) void*)(dst + f * 1024), 16, 0, 0);
        if (MODE == 2) {
#pragma unroll
            for (int f = 0; f < 8; ++f)
                __builtin_amdgcn_global_load_lds((const __attribute__((address_space(1))) void*)(g_tp + (size_t)t * TILE_BYTES + f * 1024),
                                                 (__attribute__((address_space(3))) void*)(dst + TILE_BYTES + f * 1024), 16, 0, 0);
        }
        if (MODE >= 1 && wave == 0) {
            char* st = smem + buf * BUF + (MODE == 2 ? 2 : 1) * TILE_BYTES;
            __builtin_amdgcn_global_load_lds((const __attribute__((address_space(1))) void*)(g_lse + SW * t),
                                             (__attribute__((address_space(3))) void*)st, 4, 0, 0);
            if (MODE == 2)
                __builtin_amdgcn_global_load_lds((const __attribute__((address_space(1))) void*)(g_usum + SW * t),
                                                 (__attribute__((address_space(3))) void*)(st + 256), 4, 0, 0);
            if (role)
                __builtin_amdgcn_global_load_lds((const __attribute__((address_space(1))) void*)(g_gt + SW * t),
                                                 (__attribute__((address_space(3))) void*)(st + 512), 4, 0, 0);
        }
    };
    issue(0, 0);

    // the owned rows' fragments (B operand of the transposed S tile): 16 k-steps x (hi, lo)
    bf16x8 oh[16], ol[16];
    {
        const char* src = p.sp[own] + ((size_t)b * own_tiles + To) * TILE_BYTES + 16 * lane;
#pragma unroll
        for (int s = 0; s < 16; ++s) {
            oh[s] = *reinterpret_cast<const bf16x8*>(src + (2 * s) * 1024);
            ol[s] = *reinterpret_cast<const bf16x8*>(src + (2 * s + 1) * 1024);
        }
    }
    float lse_own = 0.f, usum_own = 0.f, wpos = 0.f, wneg = 0.f;
    int gt_own = -1;
    if (MODE >= 1) {
        lse_own = p.lse[own][own_stat + i];
        wpos = p.consts[0];
        wneg = p.consts[1];
        if (!role) gt_own = p.gt[0][own_stat + i];
    }
    if (MODE == 2) usum_own = p.usum[own][own_stat + i];

    float run_m = -INFINITY, run_l = 0.f, run_u = 0.f;             // MODE 0: the online (max, sum exp); MODE 1: the sum of u
    f32x16 G[MODE == 2 ? 8 : 1];
#pragma unroll
    for (int ct = 0; ct < (MODE == 2 ? 8 : 1); ++ct) G[ct] = zero16();

    for (int t = 0; t < sw_tiles; ++t) {
        // tile t has landed for this wave, then for all (barrier); every wave is also done reading the other buffer (tile t - 1).  Wait
        // and barrier are ONE asm statement with a memory clobber (see sim_frag_kernel of coarse_match.hip)
        asm volatile("s_waitcnt vmcnt(0) lgkmcnt(0)\n\ts_barrier" ::: "memory");
        if (t + 1 < sw_tiles) issue(t + 1, (t + 1) & 1);
        const char* base = smem + (t & 1) * BUF + 16 * lane;
        // S^T[swept row][owned column].  The two cross sums are kept apart and added first: an element then has the SAME BITS whichever
        // side owns it (the roles exchange the two sums, and a + b == b + a), so s - lr_i and s - lc_j cancel in both roles as they
        // did where lr and lc were formed.  (In one chain the roles differ by a few ulp of S: 4e-6 against a 1 - conf of 1e-2.)
        f32x16 st = zero16(), cross_a = zero16(), cross_b = zero16();
#pragma unroll
        for (int s = 0; s < 16; ++s) {
            const bf16x8 yh = *reinterpret_cast<const bf16x8*>(base + (2 * s) * 1024);
            const bf16x8 yl = *reinterpret_cast<const bf16x8*>(base + (2 * s + 1) * 1024);
            cross_a = mma_bf16<1>(yl, yl, oh[s], oh[s], cross_a);   // swept lo . owned hi
            cross_b = mma_bf16<1>(yh, yh, ol[s], ol[s], cross_b);   // swept hi . owned lo
            st = mma_bf16<1>(yh, yh, oh[s], oh[s], st);
        }
#pragma unroll
        for (int reg = 0; reg < 16; ++reg) st[reg] = (cross_a[reg] + cross_b[reg]) + st[reg];
        const int j0 = SW * t;
        if (MODE == 0) {
            float mx = -INFINITY;
#pragma unroll
            for (int reg = 0; reg < 16; ++reg) {
                st[reg] = st[reg] * p.inv_t;
                if (j0 + acc_row(reg, h) < sw_rows) mx = fmaxf(mx, st[reg]);
            }
            if (mx > -INFINITY) {
                const float m_new = fmaxf(run_m, mx);
                float l = run_l * expf(run_m - m_new);
#pragma unroll
                for (int reg = 0; reg < 16; ++reg)
                    if (j0 + acc_row(reg, h) < sw_rows) l = l + expf(st[reg] - m_new);
                run_m = m_new;
                run_l = l;
            }
        } else {
            const char* stat = smem + (t & 1) * BUF + (MODE == 2 ? 2 : 1) * TILE_BYTES;
            f32x4 lsw[4], usw[4];
            int gsw[16];
#pragma unroll
            for (int g = 0; g < 4; ++g) {
                lsw[g] = *reinterpret_cast<const f32x4*>(stat + 4 * (8 * g + 4 * h));
                if (MODE == 2) usw[g] = *reinterpret_cast<const f32x4*>(stat + 256 + 4 * (8 * g + 4 * h));
#pragma unroll
                for (int e = 0; e < 4; ++e) gsw[4 * g + e] = role ? *reinterpret_cast<const int*>(stat + 512 + 4 * (8 * g + 4 * h + e)) : -1;
            }
#pragma unroll
            for (int reg = 0; reg < 16; ++reg) {
                const int j = j0 + acc_row(reg, h);
                const bool valid = j < sw_rows;
                const float s = st[reg] * p.inv_t;
                const float p_own = expf(s - lse_own), p_sw = expf(s - lsw[reg >> 2][reg & 3]);
                const float conf = p_own * p_sw;
                float u = 0.f;
                if (valid && conf >= kLo && conf <= kHi) {
                    const bool pos = role ? gsw[reg] == i : gt_own == j;
                    u = conf * focal_grad(conf, pos, wpos, wneg, p.alpha, p.gamma);
                }
                if (MODE == 1) run_u = run_u + u;
                if (MODE == 2) st[reg] = valid ? (2.0f * u - p_own * usum_own) - p_sw * usw[reg >> 2][reg & 3] : 0.f;
            }
            if (MODE == 2) {
#pragma unroll
                for (int s2 = 0; s2 < 2; ++s2) {
                    bf16x8 dh, dl;
                    acc_frag<3>(st, s2, dh, dl);                     // registers 8 s2 .. 8 s2 + 7: 16 swept rows in the transposed planes' order
#pragma unroll
                    for (int ct = 0; ct < 8; ++ct) {
                        const bf16x8 yh = *reinterpret_cast<const bf16x8*>(base + TILE_BYTES + (2 * (8 * s2 + ct)) * 1024);
                        const bf16x8 yl = *reinterpret_cast<const bf16x8*>(base + TILE_BYTES + (2 * (8 * s2 + ct) + 1) * 1024);
                        G[ct] = mma_bf16<3>(dh, dl, yh, yl, G[ct]);  // grad[owned row][channel]
                    }
                }
            }
        }
    }

    if (MODE == 0) {
        const float m2 = __shfl_xor(run_m, 32, 64), l2 = __shfl_xor(run_l, 32, 64);
        if (h == 0 && live && i < own_rows) {
            const float m = fmaxf(run_m, m2);
            const float l = run_l * expf(run_m - m) + l2 * expf(m2 - m);
            p.lse[own][own_stat + i] = m + logf(l);
        }
    } else if (MODE == 1) {
        const float u2 = __shfl_xor(run_u, 32, 64);
        if (h == 0 && live && i < own_rows) p.usum[own][own_stat + i] = run_u + u2;
    } else if (live) {
        float* out = p.grad[own] + (size_t)b * own_rows * C + r;
#pragma unroll
        for (int ct = 0; ct < 8; ++ct)
#pragma unroll
            for (int reg = 0; reg < 16; ++reg) {
                const int row = SW * To + acc_row(reg, h);
                if (row < own_rows) out[(size_t)row * C + 32 * ct] = G[ct][reg] * p.out_scale;
            }
    }
}

struct FineArgs {
    const float* f0;            // [cap][128]
    const float* f1;            // [cap][WW][128]
    const float* expec_f;       // [cap][3]
    const float* expec_f_gt;    // [cap][2]
    const int* count;
    int cap, W, WW, training;
    double correct_thr, scale;
    float* g0;
    float* g1;
    int* n_correct;
    int* status;
};

constexpr double kInvSqrtCF = 0.08838834764831843;                  // 1 / sqrt(128.0)

__device__ __forceinline__ double wave_max(double x) {
    for (int off = 32; off >= 1; off >>= 1) {
        const double y = __shfl_xor(x, off, 64);
        x = y > x ? y : x;
    }
    return x;
}

__global__ __launch_bounds__(kThreads) void fine_grads_kernel(FineArgs p) {
    __shared__ double red[kThreads];
    __shared__ double dsw[4][128];
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6, n = clamped_count(p.count, p.cap), WW = p.WW;
    auto inverse = [&](int k) {
        const double s = (double)p.expec_f[3 * (long long)k + 2];
        return 1.0 / (s < 1e-10 ? 1e-10 : s);
    };
    auto correct = [&](int k) {
        const double ax = fabs((double)p.expec_f_gt[2 * (long long)k]), ay = fabs((double)p.expec_f_gt[2 * (long long)k + 1]);
        return (ax > ay ? ax : ay) < p.correct_thr && ax == ax && ay == ay;
    };
    double acc[1] = {0.0};
    for (int k = tid; k < n; k += kThreads) acc[0] = acc[0] + inverse(k);
    red64::block_sums<kThreads>(acc, 1, red);
    const double mean_inv = acc[0] / (double)n;
    acc[0] = 0.0;
    for (int k = tid; k < n; k += kThreads)
        if (correct(k)) acc[0] = acc[0] + 1.0;                      // whole numbers below 2^53: exact in any order
    red64::block_sums<kThreads>(acc, 1, red);
    const int status = acc[0] > 0.0 ? OPBWD_OK : (!p.training ? OPBWD_NONE : (n > 0 ? OPBWD_FORCED : OPBWD_EMPTY));
    if (blockIdx.x == 0 && tid == 0) {
        *p.n_correct = status == OPBWD_OK ? (int)acc[0] : (status == OPBWD_FORCED ? 1 : 0);
        *p.status = status;
    }
    const int k = 4 * blockIdx.x + wave;
    if (k >= n) return;                                             // no workgroup barrier below
    bool counts = false;
    double wk = 0.0, nc = 1.0;
    if (status == OPBWD_OK) {
        counts = correct(k);
        wk = inverse(k) / mean_inv;
        nc = acc[0];
    } else if (status == OPBWD_FORCED) {
        counts = k == 0;
        wk = 1e-6;
    }
    const float* f0 = p.f0 + (size_t)k * CF;
    const float* f1 = p.f1 + (size_t)k * WW * CF;
    float* g0 = p.g0 + (size_t)k * CF;
    float* g1 = p.g1 + (size_t)k * WW * CF;
    if (!counts) {
        for (int c = lane; c < CF; c += 64) g0[c] = 0.f;
        for (int e = lane; e < WW * CF; e += 64) g1[e] = 0.f;
        return;
    }
    const double step = 2.0 / (double)(p.W - 1);
    double x[2], e[2], gx[2], gy[2];
    for (int q = 0; q < 2; ++q) {
        const int r = lane + 64 * q;
        x[q] = -INFINITY;
        gx[q] = gy[q] = 0.0;
        if (r < WW) {
            double sim = 0.0;
            for (int c = 0; c < CF; ++c) sim = sim + (double)f0[c] * (double)f1[(size_t)r * CF + c];
            x[q] = sim * kInvSqrtCF;
            gx[q] = -1.0 + (double)(r % p.W) * step;
            gy[q] = -1.0 + (double)(r / p.W) * step;
        }
    }
    const double m = wave_max(x[0] > x[1] ? x[0] : x[1]);
    for (int q = 0; q < 2; ++q) e[q] = lane + 64 * q < WW ? exp(x[q] - m) : 0.0;
    const double Z = red64::wave_sum(e[0] + e[1]);
    const double p0 = e[0] / Z, p1 = e[1] / Z;
    const double cox = red64::wave_sum(p0 * gx[0] + p1 * gx[1]), coy = red64::wave_sum(p0 * gy[0] + p1 * gy[1]);
    const double k2 = p.scale * -2.0;
    const double dcx = (k2 * ((double)p.expec_f_gt[2 * (long long)k] - cox)) * wk / nc;
    const double dcy = (k2 * ((double)p.expec_f_gt[2 * (long long)k + 1] - coy)) * wk / nc;
    const double mid = cox * dcx + coy * dcy;
    dsw[wave][lane] = p0 * ((gx[0] * dcx + gy[0] * dcy) - mid);
    dsw[wave][lane + 64] = p1 * ((gx[1] * dcx + gy[1] * dcy) - mid);
    __builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront");
    __builtin_amdgcn_wave_barrier();
    __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "wavefront");
    for (int c = lane; c < CF; c += 64) {
        double s = 0.0;
        for (int r = 0; r < WW; ++r) s = s + dsw[wave][r] * (double)f1[(size_t)r * CF + c];
        g0[c] = (float)(kInvSqrtCF * s);
    }
    for (int r = 0; r < WW; ++r) {
        const double v = kInvSqrtCF * dsw[wave][r];
        for (int c = lane; c < CF; c += 64) g1[(size_t)r * CF + c] = (float)(v * (double)f0[c]);
    }
}

bool misaligned(const void* a) { return ((uintptr_t)a & 15) != 0; }

template <int MODE>
int launch_sweep(const SweepArgs& a, int B, hipStream_t stream, const char* where) {
    static bool raised[64] = {};                                    // the limit is a property of the kernel as one device has loaded it
    constexpr size_t lds = 2 * (size_t)buf_bytes<MODE>();
    int dev = 0;
    if (hipGetDevice(&dev) != hipSuccess || dev < 0 || dev >= 64) dev = -1;
    if (dev < 0 || !raised[dev]) {
        const hipError_t e = hipFuncSetAttribute(reinterpret_cast<const void*>(sweep_kernel<MODE>), hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds);
        if (e != hipSuccess) return capi::fail(e, where);
        if (dev >= 0) raised[dev] = true;
    }
    const unsigned blocks = a.nblk0 + blocks_of(a.rows[1], R);
    hipLaunchKernelGGL(sweep_kernel<MODE>, dim3(blocks, B), dim3(kThreads), lds, stream, a);
    const hipError_t e = hipGetLastError();
    return e != hipSuccess ? capi::fail(e, where) : 0;
}

}  // namespace

extern "C" {

int opbwd_abi_version(void) { return OPBWD_ABI_VERSION; }
const char* opbwd_last_error(void) { return capi::g_error; }

size_t opbwd_coarse_workspace_bytes(int B, int N, int M) {
    if (B < 1 || B > OPBWD_MAX_BATCH || N < 1 || N > OPBWD_MAX_ROWS || M < 1 || M > OPBWD_MAX_ROWS) return 0;
    return layout_of(B, N, M).total;
}

int opbwd_coarse_grads(const float* feat0, const float* feat1, const long long* gt_j, const long long* gt_i, int B, int N, int M,
                       double temperature, double alpha, double gamma, double pos_weight, double neg_weight, double scale, void* workspace,
                       size_t workspace_bytes, float* grad0, float* grad1, void* stream_) {
    (void)gt_i;                                                     // both roles take the positive from gt_j (the header says why)
    if (feat0 == nullptr || feat1 == nullptr || gt_j == nullptr || workspace == nullptr || grad0 == nullptr || grad1 == nullptr)
        return bad_arg(__func__, "null pointer");
    if (B < 1 || B > OPBWD_MAX_BATCH) return bad_arg(__func__, "B outside [1, OPBWD_MAX_BATCH]");
    if (N < 1 || N > OPBWD_MAX_ROWS || M < 1 || M > OPBWD_MAX_ROWS) return bad_arg(__func__, "N and M: in [1, OPBWD_MAX_ROWS]");
    if (misaligned(feat0) || misaligned(feat1) || misaligned(grad0) || misaligned(grad1) || ((uintptr_t)workspace & 255) != 0)
        return bad_arg(__func__, "feat0, feat1, grad0, grad1: 16-byte aligned; workspace: 256-byte aligned");
    if (!(isfinite(temperature) && isfinite(alpha) && isfinite(gamma) && isfinite(pos_weight) && isfinite(neg_weight) && isfinite(scale)))
        return bad_arg(__func__, "temperature, alpha, gamma, pos_weight, neg_weight, scale: finite");
    const float t = (float)(temperature + 1e-4);
    if (!(t > 0.0f)) return bad_arg(__func__, "temperature + 1e-4: positive");
    const Layout l = layout_of(B, N, M);
    if (workspace_bytes < l.total) return bad_arg(__func__, "workspace_bytes below opbwd_coarse_workspace_bytes(B, N, M)");
    hipStream_t stream = (hipStream_t)stream_;
    char* ws = static_cast<char*>(workspace);
    float* consts = reinterpret_cast<float*>(ws + l.consts);
    count_kernel<<<1, kThreads, 0, stream>>>(gt_j, (long long)B * N, M, (long long)B * N * M, pos_weight, neg_weight, scale, consts);
    CAPI_CHECK_LAUNCH();
    PlaneArgs pa;
    SweepArgs sa;
    for (int s = 0; s < 2; ++s) {
        pa.x[s] = s ? feat1 : feat0;
        pa.sp[s] = ws + l.sp[s];
        pa.tp[s] = ws + l.tp[s];
        pa.lse[s] = reinterpret_cast<float*>(ws + l.lse[s]);
        pa.usum[s] = reinterpret_cast<float*>(ws + l.usum[s]);
        pa.gt[s] = reinterpret_cast<int*>(ws + l.gt[s]);
        pa.rows[s] = s ? M : N;
        pa.tiles[s] = l.tiles[s];
        sa.sp[s] = pa.sp[s];
        sa.tp[s] = pa.tp[s];
        sa.lse[s] = pa.lse[s];
        sa.usum[s] = pa.usum[s];
        sa.gt[s] = pa.gt[s];
        sa.grad[s] = s ? grad1 : grad0;
        sa.rows[s] = pa.rows[s];
        sa.tiles[s] = pa.tiles[s];
    }
    pa.gt_j = gt_j;
    planes_kernel<<<dim3(8 * (l.tiles[0] + l.tiles[1]), B), kThreads, 0, stream>>>(pa);
    CAPI_CHECK_LAUNCH();
    sa.nblk0 = (int)blocks_of(N, R);
    sa.inv_t = 1.0f / t;
    sa.out_scale = 0.0625f / t;
    sa.alpha = (float)alpha;
    sa.gamma = (float)gamma;
    sa.consts = consts;
    if (int rc = launch_sweep<0>(sa, B, stream, __func__)) return rc;
    if (int rc = launch_sweep<1>(sa, B, stream, __func__)) return rc;
    return launch_sweep<2>(sa, B, stream, __func__);
}

int opbwd_fine_grads(const float* feat_f0, const float* feat_f1, const float* expec_f, const float* expec_f_gt, const int* count, int cap,
                     int W, double correct_thr, int training, double scale, float* grad_f0, float* grad_f1, int* n_correct, int* status,
                     void* stream) {
    if (feat_f0 == nullptr || feat_f1 == nullptr || expec_f == nullptr || expec_f_gt == nullptr || grad_f0 == nullptr || grad_f1 == nullptr ||
        n_correct == nullptr || status == nullptr)
        return bad_arg(__func__, "null pointer");
    if (cap < 1 || cap > OPBWD_MAX_ROWS) return bad_arg(__func__, "cap outside [1, OPBWD_MAX_ROWS]");
    if (W < 3 || W > 11 || (W & 1) == 0) return bad_arg(__func__, "window: odd, from 3 to 11");
    if (!(correct_thr == correct_thr)) return bad_arg(__func__, "correct_thr: not NaN");
    if (!isfinite(scale)) return bad_arg(__func__, "scale: finite");
    const FineArgs a = {feat_f0, feat_f1, expec_f, expec_f_gt, count, cap, W, W * W, training != 0, correct_thr, scale, grad_f0, grad_f1, n_correct,
                        status};
    fine_grads_kernel<<<blocks_of(cap, 4), kThreads, 0, (hipStream_t)stream>>>(a);
    CAPI_CHECK_LAUNCH();
    return 0;
}

}  // extern "C"
