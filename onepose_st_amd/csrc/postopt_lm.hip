// The second-order solver of the keypoint-free SfM depth refinement (include/onepose_postopt_lm.h): Levenberg-Marquardt on the problem that
// postopt.hip solves with Adam, in float64, every expression in the written order.
//
// fold_row (postopt_fold.h) turns every residual row into h(d) = d * a + b, and every track owns one scalar depth, so the normal
// equations are diagonal: LM is P independent scalar problems.  One launch solves them all.  One wave owns a track at a time; lane l
// owns the rows r0 + l, r0 + l + 64, ... of it.  A track of at most 64 rows folds its row inside the kernel and keeps the 8 doubles
// in registers over all iterations; a longer one folds once into the rows workspace, and every lane re-reads only the rows it wrote
// itself (same thread, same address: program order, no fence).  The sums c, g, H go through the xor butterfly, after which every lane
// holds the same three numbers, so the accept / reject loop is wave-uniform.  No atomics, no LDS.  A second, one-workgroup launch sums
// the per-track costs in index order into the two totals.
#include "capi_error.h"
#include "postopt_fold.h"
#include "reduce_f64.h"
#include "onepose_postopt_lm.h"
#include <stdint.h>

namespace {

using capi::bad_arg;
using capi::fail;
using capi::g_error;
using red64::uniform;
using red64::wave_sum;

constexpr int kThreads = 256;                // 4 waves, one track per wave at a time
constexpr int kMaxBlocks = 2048;             // wave w of the grid owns tracks w, w + 4 * grid, ... (the step kernel's rule)
constexpr int kMaxIters = 1 << 20;

struct LmArgs {
    FoldInputs in;
    const long long* offs;              // [P + 1] first row of every track
    double* depth;                      // [P] in / out
    double* rows;                       // [L][kRow] workspace, written only for tracks of more than 64 rows
    int *iterations, *rejects, *status; // [P]
    double *lambda, *cost0, *cost1;     // [P]
    double* resid;                      // optional [L][2]: the residuals at the returned depths
    double lam0, up, down, lam_min, lam_max, step_tol;
    long long L;
    int P, max_iters;
};

struct Sums {
    double c, g, H;
};

// one folded row q at depth d: c += 0.5 r^2, g += J r, H += J^2 over its two components, J = d r / d d = (a - p * a2) / z
__device__ __forceinline__ void add_row(const double* q, double d, Sums& s, double* resid) {
#pragma clang fp contract(off)
    const double z = d * q[2] + q[5];
    const double px = (d * q[0] + q[3]) / z, py = (d * q[1] + q[4]) / z;
    const double rx = px - q[6], ry = py - q[7];
    const double jx = (q[0] - px * q[2]) / z, jy = (q[1] - py * q[2]) / z;
    s.c += (0.5 * rx) * rx + (0.5 * ry) * ry;
    s.g += jx * rx + jy * ry;
    s.H += jx * jx + jy * jy;
    if (resid) {
        resid[0] = rx;
        resid[1] = ry;
    }
}

__device__ __forceinline__ void load_row(const double* rows, long long r, double* q) {
    const double2* v = reinterpret_cast<const double2*>(rows + r * kRow);
    const double2 q0 = v[0], q1 = v[1], q2 = v[2], q3 = v[3];
    q[0] = q0.x; q[1] = q0.y; q[2] = q1.x; q[3] = q1.y; q[4] = q2.x; q[5] = q2.y; q[6] = q3.x; q[7] = q3.y;
}

// the track's sums at depth d; `own` is this lane's row of a short track (valid where has_own), rows r0 + lane, + 64, ... otherwise
__device__ __forceinline__ Sums evaluate(const double* own, bool is_short, bool has_own, const double* rows, long long r0, long long r1,
                                         int lane, double d, double* resid) {
    Sums s{0.0, 0.0, 0.0};
    if (is_short) {
        if (has_own) add_row(own, d, s, resid ? resid + 2 * (r0 + lane) : nullptr);
    } else {
        for (long long r = r0 + lane; r < r1; r += 64) {
            double q[kRow];
            load_row(rows, r, q);
            add_row(q, d, s, resid ? resid + 2 * r : nullptr);
        }
    }
    s.c = uniform(wave_sum(s.c));
    s.g = uniform(wave_sum(s.g));
    s.H = uniform(wave_sum(s.H));
    return s;
}

__global__ __launch_bounds__(kThreads) void postopt_lm_kernel(LmArgs a) {
#pragma clang fp contract(off)
    const int lane = threadIdx.x & 63;
    const int wave = __builtin_amdgcn_readfirstlane((int)(blockIdx.x * (kThreads / 64) + (threadIdx.x >> 6)));
    const int nwaves = gridDim.x * (kThreads / 64);
    for (int p = wave; p < a.P; p += nwaves) {
        const long long r0 = a.offs[p], r1 = a.offs[p + 1];
        double d = a.depth[p];
        int k = 0, rej = 0, status = OPLM_DEGENERATE;
        double lam = a.lam0, c0 = __builtin_nan(""), c1 = __builtin_nan("");
        if (r0 >= 0 && r0 < r1 && r1 <= a.L) {                   // the host validates; a bad table entry reads and writes nothing
            const bool is_short = r1 - r0 <= 64, has_own = r0 + lane < r1;
            double own[kRow] = {0.0, 0.0, 0.0, 0.0, 0.0, 0.0, 0.0, 0.0};
            if (is_short) {
                if (has_own) fold_row(a.in, r0 + lane, own);
            } else {
                for (long long r = r0 + lane; r < r1; r += 64) fold_row(a.in, r, a.rows + r * kRow);
            }
            Sums s = evaluate(own, is_short, has_own, a.rows, r0, r1, lane, d, nullptr);
            c0 = c1 = s.c;
            if (isfinite(s.c) && s.H > 0.0) {
                for (;;) {
                    const double delta = -s.g / (s.H * (1.0 + lam));
                    if (fabs(delta) <= a.step_tol * (fabs(d) + a.step_tol)) { status = OPLM_CONVERGED; break; }
                    if (k >= a.max_iters) { status = OPLM_MAX_ITERS; break; }
                    ++k;
                    const Sums t = evaluate(own, is_short, has_own, a.rows, r0, r1, lane, d + delta, nullptr);
                    if (isfinite(t.c) && t.c < s.c && t.H > 0.0) {
                        d = d + delta;
                        s = t;
                        lam = fmax(lam * a.down, a.lam_min);
                    } else {
                        ++rej;
                        lam = lam * a.up;
                        if (lam > a.lam_max) { status = OPLM_STALLED; break; }
                    }
                }
                c1 = s.c;
            }
            if (a.resid) evaluate(own, is_short, has_own, a.rows, r0, r1, lane, d, a.resid);
        }
        if (lane == 0) {
            a.depth[p] = d;
            a.iterations[p] = k;
            a.rejects[p] = rej;
            a.status[p] = status;
            a.lambda[p] = lam;
            a.cost0[p] = c0;
            a.cost1[p] = c1;
        }
    }
}

// the two totals: thread t sums tracks t, t + 256, ... in order, then a tree over the 256 partials -- the same order every run
__global__ __launch_bounds__(kThreads) void postopt_lm_totals_kernel(const double* cost0, const double* cost1, int P, double* total0,
                                                                     double* total1) {
#pragma clang fp contract(off)
    __shared__ double red0[kThreads], red1[kThreads];
    double s0 = 0.0, s1 = 0.0;
    for (int p = threadIdx.x; p < P; p += kThreads) {
        s0 += cost0[p];
        s1 += cost1[p];
    }
    red0[threadIdx.x] = s0;
    red1[threadIdx.x] = s1;
    __syncthreads();
    for (int h = kThreads / 2; h >= 1; h >>= 1) {
        if ((int)threadIdx.x < h) {
            red0[threadIdx.x] = red0[threadIdx.x] + red0[threadIdx.x + h];
            red1[threadIdx.x] = red1[threadIdx.x] + red1[threadIdx.x + h];
        }
        __syncthreads();
    }
    if (threadIdx.x == 0) {
        *total0 = red0[0];
        *total1 = red1[0];
    }
}

size_t workspace_total(long long L) { return ((size_t)L * kRow * 8 + 255) & ~(size_t)255; }

}  // namespace

extern "C" {

int oplm_abi_version(void) { return OPLM_ABI_VERSION; }

const char* oplm_last_error(void) { return g_error; }

size_t oplm_workspace_bytes(long long L, int P) {
    if (P < 1 || L < P || L > (1LL << 40)) return 0;
    return workspace_total(L);
}

int oplm_refine(double* depth, const long long* track_offsets, int P, long long L, const double* intrinsic0, const double* intrinsic1,
                const double* mkpts0_c, const double* mkpts1_f, const long long* left_idx, const long long* right_idx,
                const double* angle_axis, int F, double lam0, double up, double down, double lam_min, double lam_max, double step_tol,
                int max_iters, int* iterations, int* rejects, int* status, double* lambda, double* initial_cost, double* final_cost,
                double* initial_residual, double* final_residual, double* residuals, void* workspace, size_t workspace_bytes,
                void* stream) {
    if (!depth || !track_offsets || !intrinsic0 || !intrinsic1 || !mkpts0_c || !mkpts1_f || !left_idx || !right_idx || !angle_axis ||
        !iterations || !rejects || !status || !lambda || !initial_cost || !final_cost || !initial_residual || !final_residual || !workspace)
        return bad_arg(__func__, "null pointer");
    if (P < 1 || L < P || F < 1 || L > (1LL << 40)) return bad_arg(__func__, "bad sizes");
    if (max_iters < 0 || max_iters > kMaxIters) return bad_arg(__func__, "max_iters outside [0, 2^20]");
    // written so that a NaN fails: a damping schedule that cannot grow, or a tolerance that is no number, would never end a track
    if (!(lam0 > 0.0 && lam_min > 0.0 && lam_max >= lam_min && lam_max < HUGE_VAL && up > 1.0 && up < HUGE_VAL && down > 0.0 &&
          down <= 1.0 && step_tol >= 0.0 && step_tol < HUGE_VAL))
        return bad_arg(__func__, "LM constants: lam0, lam_min > 0, lam_min <= lam_max, up > 1, 0 < down <= 1, step_tol >= 0, all finite");
    if (workspace_bytes < workspace_total(L)) return bad_arg(__func__, "workspace too small (oplm_workspace_bytes)");
    if (((uintptr_t)workspace & 255) || ((uintptr_t)residuals & 15)) return bad_arg(__func__, "workspace 256-byte, residuals 16-byte aligned");
    hipStream_t s = (hipStream_t)stream;
    LmArgs a{};
    a.in = FoldInputs{intrinsic0, intrinsic1, mkpts0_c, mkpts1_f, angle_axis, left_idx, right_idx, F};
    a.offs = track_offsets;
    a.depth = depth;
    a.rows = static_cast<double*>(workspace);
    a.iterations = iterations;
    a.rejects = rejects;
    a.status = status;
    a.lambda = lambda;
    a.cost0 = initial_cost;
    a.cost1 = final_cost;
    a.resid = residuals;
    a.lam0 = lam0;
    a.up = up;
    a.down = down;
    a.lam_min = lam_min;
    a.lam_max = lam_max;
    a.step_tol = step_tol;
    a.L = L;
    a.P = P;
    a.max_iters = max_iters;
    const long long want = ((long long)P + kThreads / 64 - 1) / (kThreads / 64);
    const unsigned grid = (unsigned)(want < kMaxBlocks ? want : kMaxBlocks);
    postopt_lm_kernel<<<grid, kThreads, 0, s>>>(a);
    CAPI_CHECK_LAUNCH();
    postopt_lm_totals_kernel<<<1, kThreads, 0, s>>>(initial_cost, final_cost, P, initial_residual, final_residual);
    CAPI_CHECK_LAUNCH();
    return 0;
}

}  // extern "C"
