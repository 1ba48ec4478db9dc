// The supervised signals of training and validation (include/ext/onepose_supervision.h), forward only.  The header is
// the specification: float32 steps in float32, float64 steps in float64, every expression in the written order.
//
// gt_fill_kernel     one lane per table entry: the "none" values of gt_j, gt_xy, gt_i, owner and the zero of n_gt.
// gt_claim_kernel    one lane per annotation row: project, snap, test; an integer atomicMin of the row index on the row's cell.
// gt_keep_kernel     the same lanes and the same arithmetic: a row that owns its cell writes the three tables and counts itself.
// fine_targets_kernel  one lane per match.
// focal_const_kernel one lane: the negative term of an element clamped to 1e-6, which is almost every element of a real matrix.
// focal_rows_kernel  one workgroup per row of conf: lane k streams j = k, k + 256, ... (a wave reads 256 consecutive bytes per load,
//                    four loads in flight per lane); an element at or below 1e-6 adds the constant, any other goes through log / pow in
//                    a branch that is empty for most waves; the block tree; lane 0 writes the row's pair.
// focal_finish_kernel, fine_loss_kernel  one workgroup each: sums in the same order, the means and the branches of the reference.
// No float atomics; the two integer atomics (minimum of row indices, a counter) do not depend on their order.
#include "capi_error.h"
#include "device_loop.h"
#include "ext/onepose_supervision.h"
#include "reduce_f64.h"
#include <limits.h>
#include <math.h>

#pragma clang fp contract(off)

namespace {

using capi::bad_arg;
using capi::blocks_of;
using devloop::clamped_count;

constexpr int kThreads = OPSUP_BLOCK;
static_assert(kThreads == 256, "the header fixes the tree: it starts at stride 128");
constexpr double kLo = 1e-6, kHi = 1 - 1e-6;
// loads a lane of focal_rows_kernel issues before it adds the first.  8 measured no faster than 4 on the MI355X (c4: 0.453 against 0.442 ms)
// and costs a wave of occupancy (110 against 96 VGPRs)
constexpr int kInFlight = 4;

struct Frame {
    const float* keypoints3d;
    long long kp_bstride;
    const long long* point_ids;
    const int* counts;
    const float* pose_gt;
    const float* K;
    int k_shared, B, N, A, H, W, stride, w_c, M;
};

// row r of frame b: its point, its cell (or -1: dropped) and its projection
__device__ __forceinline__ long long project_row(const Frame& f, int b, int r, long long& i, float& px, float& py) {
    i = f.point_ids[(long long)b * f.A + r];
    if (i < 0 || i >= f.N) return -1;
    const float* x = f.keypoints3d + (long long)b * f.kp_bstride + 3 * i;
    const float* P = f.pose_gt + (long long)b * 16;
    const float* K = f.K + (f.k_shared ? 0 : (long long)b * 9);
    const float X = x[0], Y = x[1], Z = x[2];
    float c[3], q[3];
    for (int k = 0; k < 3; ++k) c[k] = ((P[4 * k] * X + P[4 * k + 1] * Y) + P[4 * k + 2] * Z) + P[4 * k + 3];
    for (int k = 0; k < 3; ++k) q[k] = (K[3 * k] * c[0] + K[3 * k + 1] * c[1]) + K[3 * k + 2] * c[2];
    const float d = q[2] + 1e-6f, s = (float)f.stride;
    px = q[0] / d;
    py = q[1] / d;
    const float rx = rintf(px / s) * s, ry = rintf(py / s) * s;
    if (!(rx >= 0.0f && rx <= (float)(f.W - 1) && ry >= 0.0f && ry <= (float)(f.H - 1))) return -1;
    const long long j = (long long)((ry / s) * (float)f.w_c + rx / s);
    return j >= f.M ? -1 : j;
}

__global__ __launch_bounds__(kThreads) void gt_fill_kernel(int B, int N, int M, int* __restrict__ owner, long long* __restrict__ gt_j,
                                                           float* __restrict__ gt_xy, long long* __restrict__ gt_i, int* __restrict__ n_gt) {
    const long long e = (long long)blockIdx.x * kThreads + threadIdx.x;
    if (e < (long long)B * N) {
        gt_j[e] = -1;
        gt_xy[2 * e] = -50.0f;
        gt_xy[2 * e + 1] = -50.0f;
    }
    if (e < (long long)B * M) {
        gt_i[e] = -1;
        owner[e] = INT_MAX;
    }
    if (e < B) n_gt[e] = 0;
}

__global__ __launch_bounds__(kThreads) void gt_claim_kernel(Frame f, int* __restrict__ owner) {
    const int r = blockIdx.x * kThreads + threadIdx.x, b = blockIdx.y;
    if (r >= clamped_count(f.counts ? f.counts + b : nullptr, f.A)) return;
    long long i;
    float px, py;
    const long long j = project_row(f, b, r, i, px, py);
    if (j >= 0) atomicMin(&owner[(long long)b * f.M + j], r);
}

__global__ __launch_bounds__(kThreads) void gt_keep_kernel(Frame f, const int* __restrict__ owner, long long* __restrict__ gt_j,
                                                           float* __restrict__ gt_xy, long long* __restrict__ gt_i, int* __restrict__ n_gt) {
    const int r = blockIdx.x * kThreads + threadIdx.x, b = blockIdx.y;
    if (r >= clamped_count(f.counts ? f.counts + b : nullptr, f.A)) return;
    long long i;
    float px, py;
    const long long j = project_row(f, b, r, i, px, py);
    if (j < 0 || owner[(long long)b * f.M + j] != r) return;
    const long long row = (long long)b * f.N + i;          // one owner per cell, one cell per point: no two lanes write one entry
    gt_j[row] = j;
    gt_xy[2 * row] = px;
    gt_xy[2 * row + 1] = py;
    gt_i[(long long)b * f.M + j] = i;
    atomicAdd(&n_gt[b], 1);
}

__device__ __forceinline__ long long floor_div(long long a, long long b) {         // b > 0
    const long long q = a / b;
    return (a % b != 0 && a < 0) ? q - 1 : q;
}

__global__ __launch_bounds__(kThreads) void fine_targets_kernel(const long long* __restrict__ b_ids, const long long* __restrict__ i_ids,
                                                                const long long* __restrict__ j_ids, const int* __restrict__ count, int cap,
                                                                const long long* __restrict__ gt_j, const float* __restrict__ gt_xy, int B, int N,
                                                                int w_c, int coarse_res, int fine_res, int radius,
                                                                const float* __restrict__ scale, float* __restrict__ out) {
    const int k = blockIdx.x * kThreads + threadIdx.x;
    if (k >= clamped_count(count, cap)) return;
    const long long b = b_ids[k], i = i_ids[k], j = j_ids[k];
    const bool b_ok = b >= 0 && b < B;
    float loc[2] = {-50.0f, -50.0f};
    if (b_ok && i >= 0 && i < N && gt_j[b * N + i] == j) {
        loc[0] = gt_xy[2 * (b * N + i)];
        loc[1] = gt_xy[2 * (b * N + i) + 1];
    }
    const long long jy = floor_div(j, w_c), jx = j - jy * w_c;
    const long long cell[2] = {jx, jy};
    for (int a = 0; a < 2; ++a) {
        float g, fs;
        if (scale == nullptr) {
            fs = (float)fine_res;
            g = (float)(cell[a] * fine_res);
        } else {
            const float sc = b_ok ? scale[2 * b + (1 - a)] : 1.0f;
            const float cs = (float)coarse_res * sc;
            fs = (float)fine_res * sc;
            g = (float)cell[a] * cs;
        }
        out[2 * (long long)k + a] = ((loc[a] - g) / fs) / (float)radius;
    }
}

struct Focal {
    double alpha, gamma;
};

__device__ __forceinline__ double focal_power(double v, double gamma) { return gamma == 2.0 ? v * v : pow(v, gamma); }

__device__ __forceinline__ double clamp_conf(double x) { return x < kLo ? kLo : (x > kHi ? kHi : x); }

__device__ __forceinline__ double negative_term(double c, Focal f) { return ((-(1.0 - f.alpha)) * focal_power(c, f.gamma)) * log(1.0 - c); }

__device__ __forceinline__ double positive_term(double c, Focal f) { return ((-f.alpha) * focal_power(1.0 - c, f.gamma)) * log(c); }

__global__ void focal_const_kernel(Focal f, double* __restrict__ consts) {
    consts[0] = negative_term(kLo, f);
    consts[1] = 0.0;
}

__global__ __launch_bounds__(kThreads) void focal_rows_kernel(const float* __restrict__ conf, long long bstride, long long rstride,
                                                              const long long* __restrict__ gt_j, int N, int M, Focal f,
                                                              const double* __restrict__ consts, double* __restrict__ partials) {
    __shared__ double red[kThreads];
    const int tid = threadIdx.x, i = blockIdx.x, b = blockIdx.y;
    const long long row = (long long)b * N + i;
    const float* x = conf + b * bstride + i * rstride;
    const long long gj = gt_j[row];
    const double t_lo = consts[0];
    double acc[1] = {0.0};
    auto element = [&](int j, float v) {
        const double d = (double)v;
        if (j == gj) return;                                // the row's positive: below
        if (d <= kLo) acc[0] = acc[0] + t_lo;
        else acc[0] = acc[0] + negative_term(clamp_conf(d), f);
    };
    int j = tid;
    for (; j + (kInFlight - 1) * kThreads < M; j += kInFlight * kThreads) {     // kInFlight loads in flight, added in ascending order
        float v[kInFlight];
#pragma unroll
        for (int u = 0; u < kInFlight; ++u) v[u] = x[j + u * kThreads];
#pragma unroll
        for (int u = 0; u < kInFlight; ++u) element(j + u * kThreads, v[u]);
    }
    for (; j < M; j += kThreads) element(j, x[j]);
    red64::block_sums<kThreads>(acc, 1, red);
    if (tid == 0) {
        partials[2 * row] = (gj >= 0 && gj < M) ? positive_term(clamp_conf((double)x[gj]), f) : 0.0;
        partials[2 * row + 1] = acc[0];
    }
}

__global__ __launch_bounds__(kThreads) void focal_finish_kernel(const double* __restrict__ partials, const long long* __restrict__ gt_j,
                                                                long long rows, int M, long long per_batch, double pos_weight,
                                                                double neg_weight, double* __restrict__ sums, long long* __restrict__ counts) {
    __shared__ double red[2 * kThreads];
    __shared__ long long cnt[kThreads];
    const int tid = threadIdx.x;
    double acc[2] = {0.0, 0.0};
    long long n = 0;
    for (long long r = tid; r < rows; r += kThreads) {
        acc[0] = acc[0] + partials[2 * r];
        acc[1] = acc[1] + partials[2 * r + 1];
        const long long gj = gt_j[r];
        n += (gj >= 0 && gj < M) ? 1 : 0;
    }
    red64::block_sums<kThreads>(acc, 2, red);
    cnt[tid] = n;
    __syncthreads();
    for (int s = kThreads / 2; s > 0; s >>= 1) {
        if (tid < s) cnt[tid] += cnt[tid + s];
        __syncthreads();
    }
    if (tid != 0) return;
    const long long n_pos = cnt[0], n_neg = per_batch - n_pos;
    sums[0] = acc[0];
    sums[1] = acc[1];
    counts[0] = n_pos;
    counts[1] = n_neg;
    if (n_pos == 0) sums[2] = neg_weight * (acc[1] / (double)n_neg);
    else if (n_neg == 0) sums[2] = pos_weight * (acc[0] / (double)n_pos);
    else sums[2] = pos_weight * (acc[0] / (double)n_pos) + neg_weight * (acc[1] / (double)n_neg);
}

__global__ __launch_bounds__(kThreads) void fine_loss_kernel(const float* __restrict__ expec_f, const float* __restrict__ expec_f_gt,
                                                             const int* __restrict__ count, int cap, double correct_thr, int training,
                                                             double* __restrict__ loss_f, int* __restrict__ n_correct, int* __restrict__ status) {
    __shared__ double red[2 * kThreads];
    const int tid = threadIdx.x, n = clamped_count(count, cap);
    auto inverse = [&](int k) {
        const double s = (double)expec_f[3 * (long long)k + 2];
        return 1.0 / (s < 1e-10 ? 1e-10 : s);
    };
    auto squared = [&](int k) {
        const double dx = (double)expec_f_gt[2 * (long long)k] - (double)expec_f[3 * (long long)k];
        const double dy = (double)expec_f_gt[2 * (long long)k + 1] - (double)expec_f[3 * (long long)k + 1];
        return dx * dx + dy * dy;
    };
    double acc[2] = {0.0, 0.0};                             // the inverse stds; then the correct rows' terms and their number
    for (int k = tid; k < n; k += kThreads) acc[0] = acc[0] + inverse(k);
    red64::block_sums<kThreads>(acc, 1, red);
    const double mean_inv = acc[0] / (double)n;
    acc[0] = 0.0;
    for (int k = tid; k < n; k += kThreads) {
        const double ax = fabs((double)expec_f_gt[2 * (long long)k]), ay = fabs((double)expec_f_gt[2 * (long long)k + 1]);
        if ((ax > ay ? ax : ay) < correct_thr && ax == ax && ay == ay) {
            acc[0] = acc[0] + squared(k) * (inverse(k) / mean_inv);
            acc[1] = acc[1] + 1.0;                          // whole numbers below 2^53: exact in any order
        }
    }
    red64::block_sums<kThreads>(acc, 2, red);
    if (tid != 0) return;
    if (acc[1] > 0.0) {
        *loss_f = acc[0] / acc[1];
        *n_correct = (int)acc[1];
        *status = OPSUP_OK;
    } else if (!training) {
        *loss_f = __builtin_nan("");
        *n_correct = 0;
        *status = OPSUP_NONE;
    } else if (n > 0) {
        *loss_f = squared(0) * 1e-6;
        *n_correct = 1;
        *status = OPSUP_FORCED;
    } else {
        *loss_f = __builtin_nan("");
        *n_correct = 0;
        *status = OPSUP_EMPTY;
    }
}

}  // namespace

extern "C" {

int opsup_abi_version(void) { return OPSUP_ABI_VERSION; }
const char* opsup_last_error(void) { return capi::g_error; }

int opsup_ground_truth(const float* keypoints3d, long long kp_bstride, const long long* point_ids, const int* counts, const float* pose_gt,
                       const float* K, int k_shared, int B, int N, int A, int H, int W, int stride, int* owner, long long* gt_j,
                       float* gt_xy, long long* gt_i, int* n_gt, void* stream) {
    if (keypoints3d == nullptr || point_ids == nullptr || pose_gt == nullptr || K == nullptr || owner == nullptr || gt_j == nullptr ||
        gt_xy == nullptr || gt_i == nullptr || n_gt == nullptr)
        return bad_arg(__func__, "null pointer");
    if (B < 1 || B > OPSUP_MAX_BATCH) return bad_arg(__func__, "B outside [1, OPSUP_MAX_BATCH]");
    if (N < 1 || N > OPSUP_MAX_ROWS || A < 1 || A > OPSUP_MAX_ROWS) return bad_arg(__func__, "N and A: in [1, OPSUP_MAX_ROWS]");
    if (stride < 1 || H < stride || W < stride || H > 32768 || W > 32768) return bad_arg(__func__, "image: stride >= 1, stride <= H, W <= 32768");
    if (kp_bstride != 0 && kp_bstride < 3LL * N) return bad_arg(__func__, "kp_bstride: 0 (shared) or at least 3 * N");
    const int w_c = W / stride, M = (H / stride) * w_c;
    const Frame f = {keypoints3d, kp_bstride, point_ids, counts, pose_gt, K, k_shared, B, N, A, H, W, stride, w_c, M};
    const long long entries = (long long)B * (N > M ? N : M);
    gt_fill_kernel<<<blocks_of(entries, kThreads), kThreads, 0, (hipStream_t)stream>>>(B, N, M, owner, gt_j, gt_xy, gt_i, n_gt);
    CAPI_CHECK_LAUNCH();
    gt_claim_kernel<<<dim3(blocks_of(A, kThreads), B), kThreads, 0, (hipStream_t)stream>>>(f, owner);
    CAPI_CHECK_LAUNCH();
    gt_keep_kernel<<<dim3(blocks_of(A, kThreads), B), kThreads, 0, (hipStream_t)stream>>>(f, owner, gt_j, gt_xy, gt_i, n_gt);
    CAPI_CHECK_LAUNCH();
    return 0;
}

int opsup_fine_targets(const long long* b_ids, const long long* i_ids, const long long* j_ids, const int* count, int cap,
                       const long long* gt_j, const float* gt_xy, int B, int N, int w_c, int coarse_res, int fine_res, int radius,
                       const float* scale, float* expec_f_gt, void* stream) {
    if (b_ids == nullptr || i_ids == nullptr || j_ids == nullptr || gt_j == nullptr || gt_xy == nullptr || expec_f_gt == nullptr)
        return bad_arg(__func__, "null pointer");
    if (cap < 1 || cap > OPSUP_MAX_ROWS) return bad_arg(__func__, "cap outside [1, OPSUP_MAX_ROWS]");
    if (B < 1 || B > OPSUP_MAX_BATCH || N < 1 || N > OPSUP_MAX_ROWS) return bad_arg(__func__, "B in [1, OPSUP_MAX_BATCH], N in [1, OPSUP_MAX_ROWS]");
    if (w_c < 1 || coarse_res < 1 || fine_res < 1 || radius < 1) return bad_arg(__func__, "w_c, coarse_res, fine_res, radius: at least 1");
    fine_targets_kernel<<<blocks_of(cap, kThreads), kThreads, 0, (hipStream_t)stream>>>(b_ids, i_ids, j_ids, count, cap, gt_j, gt_xy, B, N, w_c,
                                                                                         coarse_res, fine_res, radius, scale, expec_f_gt);
    CAPI_CHECK_LAUNCH();
    return 0;
}

int opsup_coarse_loss(const float* conf, long long conf_bstride, long long conf_rstride, const long long* gt_j, int B, int N, int M,
                      double alpha, double gamma, double pos_weight, double neg_weight, double* partials, double* sums,
                      long long* counts, void* stream) {
    if (conf == nullptr || gt_j == nullptr || partials == nullptr || sums == nullptr || counts == nullptr)
        return bad_arg(__func__, "null pointer");
    if (B < 1 || B > OPSUP_MAX_BATCH) return bad_arg(__func__, "B outside [1, OPSUP_MAX_BATCH]");
    if (N < 1 || N > OPSUP_MAX_ROWS || M < 1 || M > OPSUP_MAX_ROWS) return bad_arg(__func__, "N and M: in [1, OPSUP_MAX_ROWS]");
    if (conf_rstride < M || (B > 1 && conf_bstride < 0)) return bad_arg(__func__, "strides: conf_rstride >= M, conf_bstride >= 0");
    if (!(isfinite(alpha) && isfinite(gamma) && isfinite(pos_weight) && isfinite(neg_weight)))
        return bad_arg(__func__, "alpha, gamma, pos_weight, neg_weight: finite");
    const Focal f = {alpha, gamma};
    const long long rows = (long long)B * N;
    focal_const_kernel<<<1, 1, 0, (hipStream_t)stream>>>(f, partials + 2 * rows);
    CAPI_CHECK_LAUNCH();
    focal_rows_kernel<<<dim3(N, B), kThreads, 0, (hipStream_t)stream>>>(conf, conf_bstride, conf_rstride, gt_j, N, M, f, partials + 2 * rows,
                                                                        partials);
    CAPI_CHECK_LAUNCH();
    focal_finish_kernel<<<1, kThreads, 0, (hipStream_t)stream>>>(partials, gt_j, rows, M, rows * M, pos_weight, neg_weight, sums, counts);
    CAPI_CHECK_LAUNCH();
    return 0;
}

int opsup_fine_loss(const float* expec_f, const float* expec_f_gt, const int* count, int cap, double correct_thr, int training,
                    double* loss_f, int* n_correct, int* status, void* stream) {
    if (expec_f == nullptr || expec_f_gt == nullptr || loss_f == nullptr || n_correct == nullptr || status == nullptr)
        return bad_arg(__func__, "null pointer");
    if (cap < 1 || cap > OPSUP_MAX_ROWS) return bad_arg(__func__, "cap outside [1, OPSUP_MAX_ROWS]");
    if (!(correct_thr == correct_thr)) return bad_arg(__func__, "correct_thr: not NaN");
    fine_loss_kernel<<<1, kThreads, 0, (hipStream_t)stream>>>(expec_f, expec_f_gt, count, cap, correct_thr, training != 0, loss_f, n_correct,
                                                              status);
    CAPI_CHECK_LAUNCH();
    return 0;
}

}  // extern "C"
