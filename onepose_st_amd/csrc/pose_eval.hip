// Pose evaluation on the device (include/onepose_pose_eval.h): the cm-degree errors, ADD, ADD-S and the 2D projection error
// of a sequence of poses against their ground truth.  The header is the specification; everything is float64 in the written order.
//
// errors_kernel     one lane per frame: the flags, the cosine of the rotation error (no arc cosine here) and the translation error.
// add_kernel,       grid (blocks of 256 vertices, frames): a lane transforms its vertex under both poses, its term goes through the
// proj2d_kernel     block's fixed tree, lane 0 writes the block's partial.  No [F, V] table exists anywhere.
// adds_kernel       the same grid over the TARGET vertices: a lane keeps its target in registers; the predicted vertices are transformed
//                   once per workgroup, 256 at a time, into three double arrays in LDS and read back at a wave-uniform address (a
//                   broadcast: no bank conflicts); the running minimum is complete for a tile before the next one is staged; the last
//                   tile is masked by index.  256 * V pair evaluations per V transforms: the staging is 1 / 256 of the work.
// finish_kernel     one lane per frame adds its partials in ascending block order and divides by V.
// No atomics and no MFMA (its rounding is not the written order) anywhere in this file.
#include "capi_error.h"
#include "onepose_pose_eval.h"
#include "reduce_f64.h"
#include <math.h>

#pragma clang fp contract(off)

namespace {

using capi::bad_arg;
using capi::blocks_of;

constexpr int kThreads = OPEVL_BLOCK;
constexpr int kMaxGridY = 65535;
static_assert(kThreads == 256, "the header fixes the tree: it starts at stride 128");

struct Pose {
    double r[3][3], t[3];
};

__device__ __forceinline__ Pose load_pose(const double* __restrict__ p) {
    Pose q;
    for (int i = 0; i < 3; ++i) {
        for (int j = 0; j < 3; ++j) q.r[i][j] = p[4 * i + j];
        q.t[i] = p[4 * i + 3];
    }
    return q;
}

__device__ __forceinline__ void transform(const Pose& p, double x0, double x1, double x2, double out[3]) {
    for (int k = 0; k < 3; ++k) out[k] = ((p.r[k][0] * x0 + p.r[k][1] * x1) + p.r[k][2] * x2) + p.t[k];
}

__global__ __launch_bounds__(kThreads) void errors_kernel(const double* __restrict__ pred, int pred_stride, const double* __restrict__ gt,
                                                          int gt_stride, const int* __restrict__ status, int status_mask, int frames,
                                                          double unit_scale, double* __restrict__ rot_cos, double* __restrict__ t_err,
                                                          int* __restrict__ flags) {
    const int f = blockIdx.x * kThreads + threadIdx.x;
    if (f >= frames) return;
    const double* p = pred + (long long)f * pred_stride;
    const double* g = gt + (long long)f * gt_stride;
    int flag = (status != nullptr && (status[f] & status_mask)) ? OPEVL_NO_POSE : 0;
    bool finite = true;
    for (int k = 0; k < 12; ++k) finite = finite && isfinite(p[k]) && isfinite(g[k]);
    if (!finite) flag |= OPEVL_BAD_INPUT;
    flags[f] = flag;
    if (flag) {
        rot_cos[f] = __builtin_nan("");
        t_err[f] = __builtin_inf();
        return;
    }
    double trace = 0.0;
    for (int i = 0; i < 3; ++i)
        for (int j = 0; j < 3; ++j) trace = trace + p[4 * i + j] * g[4 * i + j];
    const double clamped = trace <= 3.0 ? trace : 3.0;
    rot_cos[f] = (clamped - 1.0) / 2.0;
    const double dx = p[3] - g[3], dy = p[7] - g[7], dz = p[11] - g[11];
    t_err[f] = unit_scale * sqrt((dx * dx + dy * dy) + dz * dz);
}

__global__ __launch_bounds__(kThreads) void add_kernel(const float* __restrict__ verts, int V, const double* __restrict__ pred, int pred_stride,
                                                       const double* __restrict__ gt, int gt_stride, const int* __restrict__ flags,
                                                       int frame0, int nblk, double* __restrict__ partials) {
    __shared__ double s[kThreads];
    const int tid = threadIdx.x, f = frame0 + blockIdx.y;
    if (flags != nullptr && flags[f]) return;               // uniform over the workgroup
    const int v = blockIdx.x * kThreads + tid;
    double term[1] = {0.0};                                 // the block's tree (header, "every mean") takes an array
    if (v < V) {
        const Pose P = load_pose(pred + (long long)f * pred_stride), G = load_pose(gt + (long long)f * gt_stride);
        const double x0 = verts[3 * v], x1 = verts[3 * v + 1], x2 = verts[3 * v + 2];
        double a[3], b[3];
        transform(P, x0, x1, x2, a);
        transform(G, x0, x1, x2, b);
        const double dx = a[0] - b[0], dy = a[1] - b[1], dz = a[2] - b[2];
        term[0] = sqrt((dx * dx + dy * dy) + dz * dz);
    }
    red64::block_sums<kThreads>(term, 1, s);
    if (tid == 0) partials[(long long)f * nblk + blockIdx.x] = term[0];
}

__global__ __launch_bounds__(kThreads) void proj2d_kernel(const float* __restrict__ verts, int V, const double* __restrict__ pred,
                                                          int pred_stride, const double* __restrict__ gt, int gt_stride,
                                                          const double* __restrict__ K, int k_shared, const int* __restrict__ flags,
                                                          int frame0, int nblk, double* __restrict__ partials) {
    __shared__ double s[kThreads];
    const int tid = threadIdx.x, f = frame0 + blockIdx.y;
    if (flags != nullptr && flags[f]) return;
    const int v = blockIdx.x * kThreads + tid;
    double term[1] = {0.0};                                 // the block's tree (header, "every mean") takes an array
    if (v < V) {
        const Pose P = load_pose(pred + (long long)f * pred_stride), G = load_pose(gt + (long long)f * gt_stride);
        const double* k = K + (k_shared ? 0 : (long long)f * 9);
        const double x0 = verts[3 * v], x1 = verts[3 * v + 1], x2 = verts[3 * v + 2];
        double a[3], b[3], ua[3], ub[3];
        transform(P, x0, x1, x2, a);
        transform(G, x0, x1, x2, b);
        for (int r = 0; r < 3; ++r) {
            ua[r] = (k[3 * r] * a[0] + k[3 * r + 1] * a[1]) + k[3 * r + 2] * a[2];
            ub[r] = (k[3 * r] * b[0] + k[3 * r + 1] * b[1]) + k[3 * r + 2] * b[2];
        }
        const double dx = ua[0] / ua[2] - ub[0] / ub[2], dy = ua[1] / ua[2] - ub[1] / ub[2];
        term[0] = sqrt(dx * dx + dy * dy);
    }
    red64::block_sums<kThreads>(term, 1, s);
    if (tid == 0) partials[(long long)f * nblk + blockIdx.x] = term[0];
}

__global__ __launch_bounds__(kThreads) void adds_kernel(const float* __restrict__ verts, int V, const double* __restrict__ pred, int pred_stride,
                                                        const double* __restrict__ gt, int gt_stride, const int* __restrict__ flags,
                                                        int frame0, int block0, int nblk, double* __restrict__ partials) {
    __shared__ double sx[kThreads], sy[kThreads], sz[kThreads];
    const int tid = threadIdx.x, f = frame0 + blockIdx.y, blk = block0 + blockIdx.x;
    if (flags != nullptr && flags[f]) return;               // uniform over the workgroup: the barriers below are safe
    const Pose P = load_pose(pred + (long long)f * pred_stride);
    const int j = blk * kThreads + tid;
    double tx = 0.0, ty = 0.0, tz = 0.0;
    if (j < V) {
        const Pose G = load_pose(gt + (long long)f * gt_stride);
        double b[3];
        transform(G, verts[3 * j], verts[3 * j + 1], verts[3 * j + 2], b);
        tx = b[0]; ty = b[1]; tz = b[2];
    }
    double m = __builtin_inf();
    for (int base = 0; base < V; base += kThreads) {
        const int i = base + tid;
        if (i < V) {
            double a[3];
            transform(P, verts[3 * i], verts[3 * i + 1], verts[3 * i + 2], a);
            sx[tid] = a[0]; sy[tid] = a[1]; sz[tid] = a[2];
        }
        __syncthreads();
        const int n = V - base < kThreads ? V - base : kThreads;         // the last tile is masked by index
        int q = 0;
        for (; q + 4 <= n; q += 4) {
#pragma unroll
            for (int u = 0; u < 4; ++u) {
                const double dx = sx[q + u] - tx, dy = sy[q + u] - ty, dz = sz[q + u] - tz;
                const double d2 = (dx * dx + dy * dy) + dz * dz;
                if (d2 < m) m = d2;
            }
        }
        for (; q < n; ++q) {
            const double dx = sx[q] - tx, dy = sy[q] - ty, dz = sz[q] - tz;
            const double d2 = (dx * dx + dy * dy) + dz * dz;
            if (d2 < m) m = d2;
        }
        __syncthreads();                                    // the tile is used up before the next one is staged
    }
    double term[1] = {j < V ? sqrt(m) : 0.0};
    red64::block_sums<kThreads>(term, 1, sx);
    if (tid == 0) partials[(long long)f * nblk + blk] = term[0];
}

__global__ __launch_bounds__(kThreads) void finish_kernel(const double* __restrict__ partials, const int* __restrict__ flags, int frames, int nblk,
                                                          int V, double* __restrict__ out) {
    const int f = blockIdx.x * kThreads + threadIdx.x;
    if (f >= frames) return;
    if (flags != nullptr && flags[f]) {
        out[f] = __builtin_inf();
        return;
    }
    double sum = 0.0;
    for (int b = 0; b < nblk; ++b) sum = sum + partials[(long long)f * nblk + b];
    out[f] = sum / (double)V;
}

const char* check_tables(const void* pred, int pred_stride, const void* gt, int gt_stride, int frames) {
    if (pred == nullptr || gt == nullptr) return "null pointer";
    if (frames < 1 || frames > OPEVL_MAX_FRAMES) return "frames outside [1, OPEVL_MAX_FRAMES]";
    if ((pred_stride != 12 && pred_stride != 16) || (gt_stride != 12 && gt_stride != 16)) return "pose stride: 12 or 16 doubles";
    return nullptr;
}

const char* check_model(const void* verts, int V, const void* partials, const void* out) {
    if (verts == nullptr || partials == nullptr || out == nullptr) return "null pointer";
    if (V < 1 || V > OPEVL_MAX_VERTICES) return "V outside [1, OPEVL_MAX_VERTICES]";
    return nullptr;
}

}  // namespace

extern "C" {

int opevl_abi_version(void) { return OPEVL_ABI_VERSION; }
const char* opevl_last_error(void) { return capi::g_error; }

int opevl_errors(const double* pose_pred, int pred_stride, const double* pose_gt, int gt_stride, const int* status, int status_mask,
                 int frames, double unit_scale, double* rot_cos, double* t_err, int* flags, void* stream) {
    if (rot_cos == nullptr || t_err == nullptr || flags == nullptr) return bad_arg(__func__, "null pointer");
    if (const char* what = check_tables(pose_pred, pred_stride, pose_gt, gt_stride, frames)) return bad_arg(__func__, what);
    if (!(isfinite(unit_scale) && unit_scale > 0)) return bad_arg(__func__, "unit_scale: finite and > 0");
    errors_kernel<<<blocks_of(frames, kThreads), kThreads, 0, (hipStream_t)stream>>>(pose_pred, pred_stride, pose_gt, gt_stride, status,
                                                                                      status_mask, frames, unit_scale, rot_cos, t_err, flags);
    CAPI_CHECK_LAUNCH();
    return 0;
}

int opevl_add(const float* verts, int V, const double* pose_pred, int pred_stride, const double* pose_gt, int gt_stride, const int* flags,
              int frames, double* partials, double* add_dist, void* stream) {
    if (const char* what = check_model(verts, V, partials, add_dist)) return bad_arg(__func__, what);
    if (const char* what = check_tables(pose_pred, pred_stride, pose_gt, gt_stride, frames)) return bad_arg(__func__, what);
    const int nblk = (int)blocks_of(V, kThreads);
    for (int f0 = 0; f0 < frames; f0 += kMaxGridY) {
        const int fc = frames - f0 < kMaxGridY ? frames - f0 : kMaxGridY;
        add_kernel<<<dim3(nblk, fc), kThreads, 0, (hipStream_t)stream>>>(verts, V, pose_pred, pred_stride, pose_gt, gt_stride, flags, f0, nblk,
                                                                        partials);
        CAPI_CHECK_LAUNCH();
    }
    finish_kernel<<<blocks_of(frames, kThreads), kThreads, 0, (hipStream_t)stream>>>(partials, flags, frames, nblk, V, add_dist);
    CAPI_CHECK_LAUNCH();
    return 0;
}

int opevl_adds(const float* verts, int V, const double* pose_pred, int pred_stride, const double* pose_gt, int gt_stride, const int* flags,
               int frames, long long pair_budget, double* partials, double* adds_dist, void* stream) {
    if (const char* what = check_model(verts, V, partials, adds_dist)) return bad_arg(__func__, what);
    if (const char* what = check_tables(pose_pred, pred_stride, pose_gt, gt_stride, frames)) return bad_arg(__func__, what);
    if (pair_budget == 0) pair_budget = OPEVL_MAX_PAIRS_PER_LAUNCH;
    const long long per_block = (long long)(V < kThreads ? V : kThreads) * V, per_frame = (long long)V * V;
    if (pair_budget < per_block || pair_budget > OPEVL_MAX_PAIRS_PER_LAUNCH)
        return bad_arg(__func__, "pair_budget outside [min(V, OPEVL_BLOCK) * V, OPEVL_MAX_PAIRS_PER_LAUNCH]");
    const int nblk = (int)blocks_of(V, kThreads);
    if (per_frame <= pair_budget) {                         // whole frames per launch
        long long chunk = pair_budget / per_frame;
        if (chunk > kMaxGridY) chunk = kMaxGridY;
        for (int f0 = 0; f0 < frames; f0 += (int)chunk) {
            const int fc = frames - f0 < chunk ? frames - f0 : (int)chunk;
            adds_kernel<<<dim3(nblk, fc), kThreads, 0, (hipStream_t)stream>>>(verts, V, pose_pred, pred_stride, pose_gt, gt_stride, flags, f0,
                                                                             0, nblk, partials);
            CAPI_CHECK_LAUNCH();
        }
    } else {                                                // the blocks of one frame per launch
        const long long chunk = pair_budget / ((long long)kThreads * V);
        for (int f0 = 0; f0 < frames; ++f0)
            for (int b0 = 0; b0 < nblk; b0 += (int)chunk) {
                const int bc = nblk - b0 < chunk ? nblk - b0 : (int)chunk;
                adds_kernel<<<dim3(bc, 1), kThreads, 0, (hipStream_t)stream>>>(verts, V, pose_pred, pred_stride, pose_gt, gt_stride, flags, f0,
                                                                              b0, nblk, partials);
                CAPI_CHECK_LAUNCH();
            }
    }
    finish_kernel<<<blocks_of(frames, kThreads), kThreads, 0, (hipStream_t)stream>>>(partials, flags, frames, nblk, V, adds_dist);
    CAPI_CHECK_LAUNCH();
    return 0;
}

int opevl_proj2d(const float* verts, int V, const double* pose_pred, int pred_stride, const double* pose_gt, int gt_stride, const double* K,
                 int k_shared, const int* flags, int frames, double* partials, double* proj2d, void* stream) {
    if (const char* what = check_model(verts, V, partials, proj2d)) return bad_arg(__func__, what);
    if (K == nullptr) return bad_arg(__func__, "null pointer");
    if (const char* what = check_tables(pose_pred, pred_stride, pose_gt, gt_stride, frames)) return bad_arg(__func__, what);
    const int nblk = (int)blocks_of(V, kThreads);
    for (int f0 = 0; f0 < frames; f0 += kMaxGridY) {
        const int fc = frames - f0 < kMaxGridY ? frames - f0 : kMaxGridY;
        proj2d_kernel<<<dim3(nblk, fc), kThreads, 0, (hipStream_t)stream>>>(verts, V, pose_pred, pred_stride, pose_gt, gt_stride, K, k_shared,
                                                                           flags, f0, nblk, partials);
        CAPI_CHECK_LAUNCH();
    }
    finish_kernel<<<blocks_of(frames, kThreads), kThreads, 0, (hipStream_t)stream>>>(partials, flags, frames, nblk, V, proj2d);
    CAPI_CHECK_LAUNCH();
    return 0;
}

}  // extern "C"
