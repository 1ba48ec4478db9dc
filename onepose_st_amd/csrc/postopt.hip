// The keypoint-free SfM post-optimisation's depth refinement (src/KeypointFreeSfM/post_optimization/optimizer/optimizer.py:221-236,
// first_order_solver.py:6-172, residual.py:6-78, residual_utils.py:3-52) and the two point updates of its caller
// (dataset/coarse_colmap_dataset.py:353-423), all in float64.
//
// The reference refines one depth per track with up to 1 000 autograd + Adam steps.  Here a prep kernel folds each residual row once:
// unprojection by K0^-1, the inverse of pose0 taken through pytorch3d's so3_exp_map / 3x3 inverse / so3_log_map, and the two
// AngleAxisRotatePoint rotations are linear in the depth d, so the homogeneous projection into frame 1 is h(d) = d * a + b (b[2] carries
// the reference's + 1e-4) and the residual is h[0:2] / h[2] - mkpts1_f.  One step kernel per Adam step then evaluates every row, sums
// gradient and loss per track in a fixed order (one wave per track, lane-strided rows, xor butterfly), updates the depth with torch's
// single-tensor Adam arithmetic, and reduces the loss to one number through per-workgroup partials and a last-arriving reducer, which
// also applies the early-stop rule and raises a device flag that turns every later step kernel into an immediate exit.  The host
// enqueues all steps with no synchronisation between them.
#include "tile.h"
#include "onepose_hip.h"
#include "postopt_fold.h"
#include "reduce_f64.h"
#include <math.h>
#include <stdint.h>

namespace {

constexpr int kStepThreads = 256;            // 4 waves, one track per wave at a time
constexpr int kStepMaxBlocks = 2048;         // wave w of the grid owns tracks w, w + 4 * grid, ... (fixed by P: deterministic sums)

struct PrepArgs {
    FoldInputs in;
    double* rows;                               // [L][kRow]
    long long L;
};

__global__ __launch_bounds__(256) void postopt_prep_kernel(PrepArgs p) {
    const long long r = (long long)blockIdx.x * 256 + threadIdx.x;
    if (r >= p.L) return;
    fold_row(p.in, r, p.rows + r * kRow);
}

struct StepArgs {
    const double* rows;                 // [L][kRow]
    const long long* offs;              // [P + 1] first row of every track
    double *depth, *m, *v;              // [P]
    const double* table;                // [max_steps][2]: step_size, bias_correction2 ** 0.5 (as Python computes them)
    double* partial;                    // [grid] per-workgroup loss
    unsigned* counter;                  // [max_steps] arrivals, zeroed per call
    unsigned* stop;                     // early-stop flag, zeroed per call
    double* loss;                       // [max_steps]
    int* steps_run;
    double* resid;                      // optional [L][2]: the residuals of the last evaluated depths
    double beta2, omb1, omb2, eps;      // omb1 = 1 - beta1, omb2 = 1 - beta2
    int P, max_steps;
};

__global__ __launch_bounds__(kStepThreads) void postopt_step_kernel(StepArgs a, int it) {
#pragma clang fp contract(off)
    __shared__ double red[kStepThreads];
    __shared__ int last;
    if (__hip_atomic_load(a.stop, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT)) return;     // stopped at an earlier step
    const int lane = threadIdx.x & 63, wv = threadIdx.x >> 6;
    const int nwaves = gridDim.x * (kStepThreads / 64);
    const double step_size = a.table[2 * it], bc2_sqrt = a.table[2 * it + 1];
    double lsum = 0.0;                                              // this wave's loss, tracks in order
    for (int p = blockIdx.x * (kStepThreads / 64) + wv; p < a.P; p += nwaves) {
        const long long r0 = a.offs[p], r1 = a.offs[p + 1];
        const double d = a.depth[p];
        double g = 0.0, l = 0.0;
        for (long long r = r0 + lane; r < r1; r += 64) {
            const double2* q = reinterpret_cast<const double2*>(a.rows + r * kRow);
            const double2 q0 = q[0], q1 = q[1], q2 = q[2], q3 = q[3];
            // q0 = (a0, a1), q1 = (a2, b0), q2 = (b1, b2 + 1e-4), q3 = mkpts1_f
            const double z = d * q1.x + q2.y;
            const double px = (d * q0.x + q1.y) / z, py = (d * q0.y + q2.x) / z;
            const double rx = px - q3.x, ry = py - q3.y;
            g += rx * ((q0.x - px * q1.x) / z) + ry * ((q0.y - py * q1.x) / z);    // d r / d d = (a - p * a2) / z
            l += (0.5 * rx) * rx + (0.5 * ry) * ry;
            if (a.resid) {
                a.resid[2 * r] = rx;
                a.resid[2 * r + 1] = ry;
            }
        }
        g = red64::wave_sum(g);
        l = red64::wave_sum(l);
        lsum += l;
        if (lane == 0) {
            // torch.optim.Adam, single tensor: exp_avg.lerp_(g, 1 - b1), exp_avg_sq.mul_(b2).addcmul_(g, g, 1 - b2),
            // param.addcdiv_(exp_avg, exp_avg_sq.sqrt() / bc2_sqrt + eps, -step_size) -- with the rounding of torch's CPU kernels
            const double m = fma(a.omb1, g - a.m[p], a.m[p]);
            const double v = fma(a.omb2 * g, g, a.v[p] * a.beta2);
            const double den = sqrt(v) / bc2_sqrt + a.eps;
            a.m[p] = m;
            a.v[p] = v;
            a.depth[p] = d + (-step_size * m) / den;
        }
    }
    // loss: per-workgroup partial, then the last workgroup to arrive sums all partials in block order (agent-scope release / acquire)
    if (lane == 0) red[wv] = lsum;
    __syncthreads();
    if (threadIdx.x == 0) {
        const double s = ((red[0] + red[1]) + red[2]) + red[3];
        __hip_atomic_store(reinterpret_cast<unsigned long long*>(a.partial) + blockIdx.x, (unsigned long long)__double_as_longlong(s),
                           __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
        asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
        __builtin_amdgcn_fence(__ATOMIC_RELEASE, "agent");
        asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
        const unsigned t = __hip_atomic_fetch_add(a.counter + it, 1u, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
        const int is_last = t == gridDim.x - 1;
        if (is_last) __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "agent");
        asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
        last = is_last;
    }
    __syncthreads();
    if (!last) return;
    double s = 0.0;
    for (int b = threadIdx.x; b < (int)gridDim.x; b += kStepThreads)
        s += __longlong_as_double((long long)__hip_atomic_load(reinterpret_cast<unsigned long long*>(a.partial) + b, __ATOMIC_RELAXED,
                                                               __HIP_MEMORY_SCOPE_AGENT));
    red[threadIdx.x] = s;
    __syncthreads();
    for (int h = kStepThreads / 2; h >= 1; h >>= 1) {
        if ((int)threadIdx.x < h) red[threadIdx.x] = red[threadIdx.x] + red[threadIdx.x + h];
        __syncthreads();
    }
    if (threadIdx.x == 0) {
        const double li = red[0];
        a.loss[it] = li;
        *a.steps_run = it + 1;
        if (it > 0) {
            // first_order_solver.py:149-162: stop once (l_{i-1} - l_i) / l_{i-1} < 1e-4 and i > 0.2 * max_steps (a NaN ratio never stops)
            const double prev = a.loss[it - 1];
            const double ratio = (prev - li) / prev;
            if (ratio < 0.0001 && (double)it > (double)a.max_steps * 0.2)
                __hip_atomic_store(a.stop, 1u, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
        }
    }
}

// general 4x4 inverse (np.linalg.inv of [[R, t], [0, 0, 0, 1]]), cofactor form
__device__ void inv4(const double* m, double* o) {
#pragma clang fp contract(off)
    double v[16];
    v[0] = m[5] * m[10] * m[15] - m[5] * m[11] * m[14] - m[9] * m[6] * m[15] + m[9] * m[7] * m[14] + m[13] * m[6] * m[11] - m[13] * m[7] * m[10];
    v[4] = -m[4] * m[10] * m[15] + m[4] * m[11] * m[14] + m[8] * m[6] * m[15] - m[8] * m[7] * m[14] - m[12] * m[6] * m[11] + m[12] * m[7] * m[10];
    v[8] = m[4] * m[9] * m[15] - m[4] * m[11] * m[13] - m[8] * m[5] * m[15] + m[8] * m[7] * m[13] + m[12] * m[5] * m[11] - m[12] * m[7] * m[9];
    v[12] = -m[4] * m[9] * m[14] + m[4] * m[10] * m[13] + m[8] * m[5] * m[14] - m[8] * m[6] * m[13] - m[12] * m[5] * m[10] + m[12] * m[6] * m[9];
    v[1] = -m[1] * m[10] * m[15] + m[1] * m[11] * m[14] + m[9] * m[2] * m[15] - m[9] * m[3] * m[14] - m[13] * m[2] * m[11] + m[13] * m[3] * m[10];
    v[5] = m[0] * m[10] * m[15] - m[0] * m[11] * m[14] - m[8] * m[2] * m[15] + m[8] * m[3] * m[14] + m[12] * m[2] * m[11] - m[12] * m[3] * m[10];
    v[9] = -m[0] * m[9] * m[15] + m[0] * m[11] * m[13] + m[8] * m[1] * m[15] - m[8] * m[3] * m[13] - m[12] * m[1] * m[11] + m[12] * m[3] * m[9];
    v[13] = m[0] * m[9] * m[14] - m[0] * m[10] * m[13] - m[8] * m[1] * m[14] + m[8] * m[2] * m[13] + m[12] * m[1] * m[10] - m[12] * m[2] * m[9];
    v[2] = m[1] * m[6] * m[15] - m[1] * m[7] * m[14] - m[5] * m[2] * m[15] + m[5] * m[3] * m[14] + m[13] * m[2] * m[7] - m[13] * m[3] * m[6];
    v[6] = -m[0] * m[6] * m[15] + m[0] * m[7] * m[14] + m[4] * m[2] * m[15] - m[4] * m[3] * m[14] - m[12] * m[2] * m[7] + m[12] * m[3] * m[6];
    v[10] = m[0] * m[5] * m[15] - m[0] * m[7] * m[13] - m[4] * m[1] * m[15] + m[4] * m[3] * m[13] + m[12] * m[1] * m[7] - m[12] * m[3] * m[5];
    v[14] = -m[0] * m[5] * m[14] + m[0] * m[6] * m[13] + m[4] * m[1] * m[14] - m[4] * m[2] * m[13] - m[12] * m[1] * m[6] + m[12] * m[2] * m[5];
    v[3] = -m[1] * m[6] * m[11] + m[1] * m[7] * m[10] + m[5] * m[2] * m[11] - m[5] * m[3] * m[10] - m[9] * m[2] * m[7] + m[9] * m[3] * m[6];
    v[7] = m[0] * m[6] * m[11] - m[0] * m[7] * m[10] - m[4] * m[2] * m[11] + m[4] * m[3] * m[10] + m[8] * m[2] * m[7] - m[8] * m[3] * m[6];
    v[11] = -m[0] * m[5] * m[11] + m[0] * m[7] * m[9] + m[4] * m[1] * m[11] - m[4] * m[3] * m[9] - m[8] * m[1] * m[7] + m[8] * m[3] * m[5];
    v[15] = m[0] * m[5] * m[10] - m[0] * m[6] * m[9] - m[4] * m[1] * m[10] + m[4] * m[2] * m[9] + m[8] * m[1] * m[6] - m[8] * m[2] * m[5];
    const double r = 1.0 / (m[0] * v[0] + m[1] * v[4] + m[2] * v[8] + m[3] * v[12]);
    for (int k = 0; k < 16; ++k) o[k] = v[k] * r;
}

struct PointArgs {
    const double *in, *depth;           // points_from_depth: keypoints [N][2], depth [N]; project: points [N][3], depth NULL
    const long long* fidx;              // [N]
    const double *K, *R, *t;            // [F][9], [F][9], [F][3]
    double* out;                        // [N][3] or [N][2]
    int N, F;
};

// coarse_colmap_dataset.py:372-380: inv(T) applied to K^-1 ([x, y, 1] * d)
__global__ __launch_bounds__(256) void postopt_points_kernel(PointArgs p) {
#pragma clang fp contract(off)
    const int n = blockIdx.x * 256 + threadIdx.x;
    if (n >= p.N) return;
    double* o = p.out + 3 * (long long)n;
    const long long f = p.fidx[n];
    if (f < 0 || f >= p.F) { o[0] = o[1] = o[2] = __builtin_nan(""); return; }
    double T[16], Ti[16], Ki[9], K[9];
    for (int i = 0; i < 3; ++i) {
        for (int j = 0; j < 3; ++j) T[4 * i + j] = p.R[9 * f + 3 * i + j];
        T[4 * i + 3] = p.t[3 * f + i];
    }
    T[12] = 0.0; T[13] = 0.0; T[14] = 0.0; T[15] = 1.0;
    inv4(T, Ti);
    for (int k = 0; k < 9; ++k) K[k] = p.K[9 * f + k];
    inv3(K, Ki);
    const double d = p.depth[n];
    const double kh[3] = {p.in[2 * (long long)n] * d, p.in[2 * (long long)n + 1] * d, 1.0 * d};
    double kc[3];
    mat3_vec(Ki, kh, kc);
    for (int i = 0; i < 3; ++i) o[i] = (Ti[4 * i] * kc[0] + Ti[4 * i + 1] * kc[1] + Ti[4 * i + 2] * kc[2]) + Ti[4 * i + 3];
}

// coarse_colmap_dataset.py:417-419: K (R X + t), xy / (z + 1e-4)
__global__ __launch_bounds__(256) void postopt_project_kernel(PointArgs p) {
#pragma clang fp contract(off)
    const int n = blockIdx.x * 256 + threadIdx.x;
    if (n >= p.N) return;
    double* o = p.out + 2 * (long long)n;
    const long long f = p.fidx[n];
    if (f < 0 || f >= p.F) { o[0] = o[1] = __builtin_nan(""); return; }
    const double X[3] = {p.in[3 * (long long)n], p.in[3 * (long long)n + 1], p.in[3 * (long long)n + 2]};
    double c[3], h[3];
    mat3_vec(p.R + 9 * f, X, c);
    for (int i = 0; i < 3; ++i) c[i] = c[i] + p.t[3 * f + i];
    mat3_vec(p.K + 9 * f, c, h);
    o[0] = h[0] / (h[2] + 1e-4);
    o[1] = h[1] / (h[2] + 1e-4);
}

struct Workspace {
    size_t ctl, rows, m, v, partial, total;     // byte offsets; ctl (stop flag + per-step counters) starts the block and is memset per call
};

__host__ Workspace workspace_layout(long long L, int P, int max_steps) {
    auto up = [](size_t x) { return (x + 255) & ~(size_t)255; };
    Workspace w{};
    w.ctl = 0;
    const size_t ctl_bytes = ((size_t)(4 + max_steps) * 4 + 15) & ~(size_t)15;
    w.rows = up(ctl_bytes);
    w.m = up(w.rows + (size_t)L * kRow * 8);
    w.v = up(w.m + (size_t)P * 8);
    w.partial = up(w.v + (size_t)P * 8);
    w.total = up(w.partial + (size_t)kStepMaxBlocks * 8);
    return w;
}

}  // namespace

extern "C" size_t ophip_postopt_workspace_bytes(long long L, int P, int max_steps) {
    if (L < 1 || P < 1 || max_steps < 1) return 0;
    return workspace_layout(L, P, max_steps).total;
}

extern "C" int ophip_postopt_refine(double* depth, const long long* track_offsets, int P, long long L, const double* intrinsic0,
                                    const double* intrinsic1, const double* mkpts0_c, const double* mkpts1_f, const long long* left_idx,
                                    const long long* right_idx, const double* angle_axis, int F, const double* step_table, int max_steps,
                                    double beta1, double beta2, double eps, double* loss, int* steps_run, double* residuals,
                                    void* workspace, size_t workspace_bytes, void* stream_) {
    if (!depth || !track_offsets || !intrinsic0 || !intrinsic1 || !mkpts0_c || !mkpts1_f || !left_idx || !right_idx || !angle_axis ||
        !step_table || !loss || !steps_run || !workspace)
        return ophip_bad_arg(__func__, "null pointer");
    if (P < 1 || L < P || F < 1 || max_steps < 1 || L > (1LL << 40)) return ophip_bad_arg(__func__, "bad sizes");
    const Workspace w = workspace_layout(L, P, max_steps);
    if (workspace_bytes < w.total) return ophip_bad_arg(__func__, "workspace too small (ophip_postopt_workspace_bytes)");
    if (((uintptr_t)workspace & 255) || ((uintptr_t)residuals & 15)) return ophip_bad_arg(__func__, "workspace 256-byte, residuals 16-byte aligned");
    hipStream_t stream = (hipStream_t)stream_;
    char* ws = static_cast<char*>(workspace);
    hipError_t e = hipMemsetAsync(ws + w.ctl, 0, w.rows - w.ctl, stream);
    if (e == hipSuccess) e = hipMemsetAsync(ws + w.m, 0, w.partial - w.m, stream);          // Adam moments m, v
    if (e == hipSuccess) e = hipMemsetAsync(steps_run, 0, sizeof(int), stream);
    if (e != hipSuccess) return ophip_fail(e, __func__);
    PrepArgs pa{{intrinsic0, intrinsic1, mkpts0_c, mkpts1_f, angle_axis, left_idx, right_idx, F}, reinterpret_cast<double*>(ws + w.rows), L};
    OPHIP_LAUNCH("postopt_prep", stream, postopt_prep_kernel, dim3((unsigned)((L + 255) / 256)), dim3(256), 0, stream, pa);
    OPHIP_CHECK_LAUNCH();
    StepArgs sa{};
    sa.rows = pa.rows;
    sa.offs = track_offsets;
    sa.depth = depth;
    sa.m = reinterpret_cast<double*>(ws + w.m);
    sa.v = reinterpret_cast<double*>(ws + w.v);
    sa.table = step_table;
    sa.partial = reinterpret_cast<double*>(ws + w.partial);
    sa.stop = reinterpret_cast<unsigned*>(ws + w.ctl);
    sa.counter = sa.stop + 4;
    sa.loss = loss;
    sa.steps_run = steps_run;
    sa.resid = residuals;
    sa.beta2 = beta2;
    sa.omb1 = 1.0 - beta1;
    sa.omb2 = 1.0 - beta2;
    sa.eps = eps;
    sa.P = P;
    sa.max_steps = max_steps;
    const int waves_per_block = kStepThreads / 64;
    const int grid = (int)(((long long)P + waves_per_block - 1) / waves_per_block < kStepMaxBlocks
                               ? ((long long)P + waves_per_block - 1) / waves_per_block : kStepMaxBlocks);
    for (int it = 0; it < max_steps; ++it) {
        OPHIP_LAUNCH("postopt_step", stream, postopt_step_kernel, dim3(grid), dim3(kStepThreads), 0, stream, sa, it);
        OPHIP_CHECK_LAUNCH();
    }
    return 0;
}

static int point_call(const char* fn, bool project, const double* in, const double* depth, const long long* frame_idx, int N,
                      const double* K, const double* R, const double* t, int F, double* out, void* stream_) {
    if (N < 0 || F < 1) return ophip_bad_arg(fn, "bad sizes");
    if (N == 0) return 0;
    if (!in || (!project && !depth) || !frame_idx || !K || !R || !t || !out) return ophip_bad_arg(fn, "null pointer");
    hipStream_t stream = (hipStream_t)stream_;
    PointArgs a{in, depth, frame_idx, K, R, t, out, N, F};
    if (project) OPHIP_LAUNCH("postopt_project", stream, postopt_project_kernel, dim3((unsigned)((N + 255) / 256)), dim3(256), 0, stream, a);
    else OPHIP_LAUNCH("postopt_points", stream, postopt_points_kernel, dim3((unsigned)((N + 255) / 256)), dim3(256), 0, stream, a);
    OPHIP_CHECK_LAUNCH();
    return 0;
}

extern "C" int ophip_postopt_points_from_depth(const double* keypoints, const double* depth, const long long* frame_idx, int N,
                                               const double* K, const double* R, const double* t, int F, double* points, void* stream) {
    return point_call(__func__, false, keypoints, depth, frame_idx, N, K, R, t, F, points, stream);
}

extern "C" int ophip_postopt_project_points(const double* points, const long long* frame_idx, int N, const double* K, const double* R,
                                            const double* t, int F, double* keypoints, void* stream) {
    return point_call(__func__, true, points, nullptr, frame_idx, N, K, R, t, F, keypoints, stream);
}
