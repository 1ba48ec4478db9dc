// The keypoint-free SfM's triangulation (include/onepose_sfm_triangulate.h): the reference shells out to COLMAP's
// point_triangulator (src/sfm_utils/triangulation.py:195-250); this file implements the project's own specification of that step.
//
//   components   hook_kernel: one thread per match row, lock-free union-find (the larger root is hooked under the smaller with one
//                compare-and-swap, retried on the new roots when it loses); flatten_kernel: every node walks to its root, which is the
//                smallest node of its component.  No workgroup waits for another; the labels do not depend on the order of the hooks.
//   prepare      camera_kernel: P = K [R | t] and the centre -R^T t per image; dir_kernel: the unit ray of every slot
//   round        round_kernel<64>: one wavefront per component of at most OPSTR_SHORT_TRACK candidates, its camera rows, keypoints,
//                rays and centres staged in LDS; round_kernel<256>: one workgroup per longer component, the same tables read from global
//                memory.  Both: one thread per two-view hypothesis, which walks all the component's elements (every lane reads the same
//                element: an LDS broadcast); the winner by one max-reduction of (inliers, earliest); refit, Gauss-Newton steps and costs
//                as per-thread partial sums in element order and a fixed tree over the threads in LDS; the exists-a-pair angle test
//                shared by the threads.  Float64 VALU and LDS reductions only; no atomics on floats, so two runs agree bit for bit.
// Sorting and segmenting the candidates by label between the rounds is the caller's (sfm_triangulate.py), with torch on the device.
//
// This file is compiled with -ffp-contract=off: every expression is evaluated in the written order.
#include <hip/hip_runtime.h>
#include <stdint.h>
#include "onepose_sfm_triangulate.h"
#include "capi_error.h"
#include "device_loop.h"
#include "reduce_f64.h"

using capi::bad_arg;
using capi::blocks_of;
using capi::fail;
using capi::g_error;
using red64::block_sums;

namespace {

constexpr int kThreads = 256;                     // 4 waves of 64
constexpr int kShort = OPSTR_SHORT_TRACK;         // one wavefront
constexpr int kCam = OPSTR_CAMERA_DOUBLES;
constexpr int kSums = 10;                         // the widest reduction: 6 + 3 normal-equation entries and the cost
constexpr int kElemDoubles = 21;                  // P 12, xy 2, dir 3, centre 3, one pad (an odd stride over the LDS banks)

// ---- components --------------------------------------------------------------------------------------------------------------------------
__device__ __forceinline__ int load_parent(const int* parent, int x) { return __hip_atomic_load(parent + x, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT); }

// parent[x] <= x always and only a root's entry ever changes, to a smaller node: the walk ends, at most U steps
__device__ __forceinline__ int find_root(const int* parent, int x) {
    for (;;) {
        const int p = load_parent(parent, x);
        if (p == x) return x;
        x = p;
    }
}

__global__ __launch_bounds__(kThreads) void hook_kernel(const long long* slot0, const long long* slot1, long long T, long long U, int* parent) {
    const long long r = (long long)blockIdx.x * kThreads + threadIdx.x;
    if (r >= T) return;
    const long long s0 = slot0[r], s1 = slot1[r];
    if (s0 < 0 || s0 >= U || s1 < 0 || s1 >= U) return;
    int a = (int)s0, b = (int)s1;
    for (;;) {                                    // lock-free: a lost compare-and-swap means another thread made progress
        a = find_root(parent, a);
        b = find_root(parent, b);
        if (a == b) return;
        if (a < b) { const int x = a; a = b; b = x; }
        if (atomicCAS(parent + a, a, b) == a) return;             // a, the larger root, now hangs under b
    }
}

__global__ __launch_bounds__(kThreads) void flatten_kernel(const int* parent, long long U, long long* labels) {
    const long long u = (long long)blockIdx.x * kThreads + threadIdx.x;
    if (u >= U) return;
    int x = (int)u;
    for (;;) {                                    // hook_kernel has ended: plain loads
        const int p = parent[x];
        if (p == x || p < 0 || p >= U) break;
        x = p;
    }
    labels[u] = x;
}

// ---- cameras and rays ----------------------------------------------------------------------------------------------------------------------
__global__ __launch_bounds__(kThreads) void camera_kernel(const double* K, const double* R, const double* t, int I, double* cameras) {
    const int i = blockIdx.x * kThreads + threadIdx.x;
    if (i >= I) return;
    const double *Ki = K + 9 * i, *Ri = R + 9 * i, *ti = t + 3 * i;
    double* c = cameras + (long long)kCam * i;
    for (int r = 0; r < 3; ++r) {
        for (int j = 0; j < 3; ++j) c[4 * r + j] = (Ki[3 * r] * Ri[j] + Ki[3 * r + 1] * Ri[3 + j]) + Ki[3 * r + 2] * Ri[6 + j];
        c[4 * r + 3] = (Ki[3 * r] * ti[0] + Ki[3 * r + 1] * ti[1]) + Ki[3 * r + 2] * ti[2];
    }
    for (int j = 0; j < 3; ++j) c[12 + j] = -((Ri[j] * ti[0] + Ri[3 + j] * ti[1]) + Ri[6 + j] * ti[2]);
    c[15] = 0.0;
}

__global__ __launch_bounds__(kThreads) void dir_kernel(const double* K, const double* R, const double* xys, const long long* slot_image, int I,
                                                       long long U, double* dirs) {
    const long long u = (long long)blockIdx.x * kThreads + threadIdx.x;
    if (u >= U) return;
    const long long i = slot_image[u];
    double d0 = 0.0, d1 = 0.0, d2 = 0.0;
    if (i >= 0 && i < I) {
        const double *Ki = K + 9 * i, *Ri = R + 9 * i;
        const double yn = (xys[2 * u + 1] - Ki[5]) / Ki[4];
        const double xn = ((xys[2 * u] - Ki[2]) - Ki[1] * yn) / Ki[0];
        d0 = (Ri[0] * xn + Ri[3] * yn) + Ri[6];
        d1 = (Ri[1] * xn + Ri[4] * yn) + Ri[7];
        d2 = (Ri[2] * xn + Ri[5] * yn) + Ri[8];
        const double n = sqrt((d0 * d0 + d1 * d1) + d2 * d2);
        d0 /= n;
        d1 /= n;
        d2 /= n;
    }
    dirs[3 * u] = d0;
    dirs[3 * u + 1] = d1;
    dirs[3 * u + 2] = d2;
}

// ---- one round -------------------------------------------------------------------------------------------------------------------------------
struct RoundTables {
    const long long *comp_offsets, *comp_label, *elem_slot, *slot_image;
    const double *xys, *cameras, *dirs;
    long long C, n_elems, U, point_base;
    int I, round, max_hypotheses, refine_steps;
    double max_err_sq, cos_min_angle;
    double* ws;                                   // [n_elems][4]: unit direction centre -> X and the inlier mark, of long components
    int* ok;
    double *xyz, *point_error;
    long long *min_slot, *assigned;
};

// the element tables of one component: staged in LDS (one wavefront) or read from global memory (one workgroup)
struct LdsElems {
    const double* e;                              // [L][kElemDoubles]
    const int* img;
    double* w;                                    // [L][4]
    __device__ __forceinline__ const double* P(int k) const { return e + kElemDoubles * k; }
    __device__ __forceinline__ const double* xy(int k) const { return e + kElemDoubles * k + 12; }
    __device__ __forceinline__ const double* dir(int k) const { return e + kElemDoubles * k + 14; }
    __device__ __forceinline__ const double* centre(int k) const { return e + kElemDoubles * k + 17; }
    __device__ __forceinline__ int image(int k) const { return img[k]; }
    __device__ __forceinline__ double* unit(int k) const { return w + 4 * k; }
};

struct GlobalElems {
    const long long *slots, *slot_image;          // slots: the component's own, [L]
    const double *xys, *cameras, *dirs;
    double* w;
    __device__ __forceinline__ const double* P(int k) const { return cameras + kCam * slot_image[slots[k]]; }
    __device__ __forceinline__ const double* xy(int k) const { return xys + 2 * slots[k]; }
    __device__ __forceinline__ const double* dir(int k) const { return dirs + 3 * slots[k]; }
    __device__ __forceinline__ const double* centre(int k) const { return cameras + kCam * slot_image[slots[k]] + 12; }
    __device__ __forceinline__ int image(int k) const { return (int)slot_image[slots[k]]; }
    __device__ __forceinline__ double* unit(int k) const { return w + 4 * k; }
};

// the n-th output of splitmix64 from `seed`, n = 0, 1, ...
__device__ __forceinline__ unsigned long long splitmix64(unsigned long long seed, unsigned long long n) {
    return devloop::mix64(seed + (n + 1ULL) * 0x9E3779B97F4A7C15ULL);
}

// q = P (X, 1): u = q0 / q2, v = q1 / q2, depth q2 (the last row of K is (0, 0, 1))
__device__ __forceinline__ void project(const double* P, const double* X, double* u, double* v, double* z) {
    const double q0 = ((P[0] * X[0] + P[1] * X[1]) + P[2] * X[2]) + P[3];
    const double q1 = ((P[4] * X[0] + P[5] * X[1]) + P[6] * X[2]) + P[7];
    const double q2 = ((P[8] * X[0] + P[9] * X[1]) + P[10] * X[2]) + P[11];
    *z = q2;
    *u = q0 / q2;
    *v = q1 / q2;
}

__device__ __forceinline__ bool is_inlier(const double* P, const double* xy, const double* X, double max_err_sq, double* err_sq) {
    double u, v, z;
    project(P, X, &u, &v, &z);
    const double du = u - xy[0], dv = v - xy[1];
    *err_sq = du * du + dv * dv;
    return z > 0.0 && *err_sq <= max_err_sq;
}

// x = A^-1 b for the symmetric A = (a00 a01 a02; . a11 a12; . . a22), by cofactors
__device__ __forceinline__ void solve_sym3(const double* a, const double* b, double* x) {
    const double a00 = a[0], a01 = a[1], a02 = a[2], a11 = a[3], a12 = a[4], a22 = a[5];
    const double c00 = a11 * a22 - a12 * a12, c01 = a02 * a12 - a01 * a22, c02 = a01 * a12 - a02 * a11;
    const double c11 = a00 * a22 - a02 * a02, c12 = a01 * a02 - a00 * a12, c22 = a00 * a11 - a01 * a01;
    const double det = (a00 * c00 + a01 * c01) + a02 * c02;
    x[0] = ((c00 * b[0] + c01 * b[1]) + c02 * b[2]) / det;
    x[1] = ((c01 * b[0] + c11 * b[1]) + c12 * b[2]) / det;
    x[2] = ((c02 * b[0] + c12 * b[1]) + c22 * b[2]) / det;
}

template <int NT>
__device__ __forceinline__ unsigned long long block_max(unsigned long long v, unsigned long long* red) {
    const int tid = threadIdx.x;
    __syncthreads();
    red[tid] = v;
    __syncthreads();
    for (int s = NT / 2; s > 0; s >>= 1) {
        if (tid < s) red[tid] = red[tid] > red[tid + s] ? red[tid] : red[tid + s];
        __syncthreads();
    }
    const unsigned long long r = red[0];
    __syncthreads();
    return r;
}

// the squared reprojection cost of X over the inliers of X0 (marked in unit(k)[3])
template <int NT, class Elems>
__device__ __forceinline__ double cost_of(const Elems& el, int L, const double* X, double* red) {
    double s[1] = {0.0};
    for (int k = threadIdx.x; k < L; k += NT) {
        if (el.unit(k)[3] == 0.0) continue;
        double u, v, z;
        project(el.P(k), X, &u, &v, &z);
        const double du = u - el.xy(k)[0], dv = v - el.xy(k)[1];
        s[0] = s[0] + (du * du + dv * dv);
    }
    block_sums<NT>(s, 1, red);
    return s[0];
}

// marks the inliers of X in unit(k)[3]; -> their number, the smallest element among them and whether they span two images
template <int NT, class Elems>
__device__ __forceinline__ int mark_inliers(const Elems& el, int L, const double* X, double max_err_sq, unsigned long long* red, int* first,
                                            bool* two_images, double* err_sum, double* dred) {
    int n = 0, mine = 0x7fffffff;
    double es[1] = {0.0};
    for (int k = threadIdx.x; k < L; k += NT) {
        double e2;
        const bool in = is_inlier(el.P(k), el.xy(k), X, max_err_sq, &e2);
        el.unit(k)[3] = in ? 1.0 : 0.0;
        if (in) {
            ++n;
            if (k < mine) mine = k;
            es[0] = es[0] + sqrt(e2);
        }
    }
    *first = 0x7fffffff - (int)block_max<NT>((unsigned long long)(0x7fffffff - mine), red);      // its barriers publish the marks
    double cnt[1] = {(double)n};                                  // exact: integers far below 2^53
    block_sums<NT>(cnt, 1, dred);
    const int count = (int)cnt[0];
    bool other = false;
    if (count > 0) {
        const int img0 = el.image(*first);
        for (int k = threadIdx.x; k < L; k += NT) other |= el.unit(k)[3] != 0.0 && el.image(k) != img0;
    }
    *two_images = __syncthreads_or(other) != 0;
    block_sums<NT>(es, 1, dred);
    *err_sum = es[0];
    return count;
}

template <int NT, class Elems>
__device__ void triangulate_component(const RoundTables& t, const Elems& el, long long c, int L, const long long* slots, double* dred,
                                      unsigned long long* ured, double* sX) {
    const int tid = threadIdx.x;
    // -- hypotheses: one per thread and pass --------------------------------------------------------------------------------------------
    const long long n_pairs = (long long)L * (L - 1) / 2;
    const bool all_pairs = n_pairs <= t.max_hypotheses;
    const int H = all_pairs ? (int)n_pairs : t.max_hypotheses;
    const unsigned long long seed = ((unsigned long long)t.comp_label[c] << 8) + (unsigned long long)t.round;
    unsigned long long best = 0;
    double bestX[3] = {0.0, 0.0, 0.0};
    for (int h = tid; h < H; h += NT) {
        int a, b;
        if (all_pairs) {                                          // (a, b), a < b, in lexicographic order
            int rem = h;
            a = 0;
            while (rem >= L - 1 - a) {
                rem -= L - 1 - a;
                ++a;
            }
            b = a + 1 + rem;
        } else {
            a = (int)(splitmix64(seed, 2ULL * h) % (unsigned long long)L);
            const int r = (int)(splitmix64(seed, 2ULL * h + 1) % (unsigned long long)(L - 1));
            b = r + (r >= a ? 1 : 0);
        }
        if (el.image(a) == el.image(b)) continue;
        const double *ca = el.centre(a), *da = el.dir(a), *cb = el.centre(b), *db = el.dir(b);
        const double n0 = da[1] * db[2] - da[2] * db[1], n1 = da[2] * db[0] - da[0] * db[2], n2 = da[0] * db[1] - da[1] * db[0];
        const double sin2 = (n0 * n0 + n1 * n1) + n2 * n2;
        if (sqrt(sin2) < OPSTR_PARALLEL_SIN) continue;
        const double w0 = ca[0] - cb[0], w1 = ca[1] - cb[1], w2 = ca[2] - cb[2];
        const double bb = (da[0] * db[0] + da[1] * db[1]) + da[2] * db[2];
        const double dw = (da[0] * w0 + da[1] * w1) + da[2] * w2;
        const double ew = (db[0] * w0 + db[1] * w1) + db[2] * w2;
        const double ta = (bb * ew - dw) / sin2, tb = (ew - bb * dw) / sin2;
        double X[3];
        for (int j = 0; j < 3; ++j) X[j] = 0.5 * ((ca[j] + ta * da[j]) + (cb[j] + tb * db[j]));
        int n = 0, img0 = -1;
        bool two = false;
        for (int k = 0; k < L; ++k) {                             // every lane reads the same element
            double e2;
            if (!is_inlier(el.P(k), el.xy(k), X, t.max_err_sq, &e2)) continue;
            ++n;
            const int img = el.image(k);
            if (img0 < 0) img0 = img;
            else two |= img != img0;
        }
        if (n < 2 || !two) continue;
        const unsigned long long key = ((unsigned long long)n << 32) | (unsigned long long)(0x7fffffff - h);    // among equals the earliest
        if (key > best) {
            best = key;
            bestX[0] = X[0];
            bestX[1] = X[1];
            bestX[2] = X[2];
        }
    }
    const unsigned long long win = block_max<NT>(best, ured);
    if (tid == 0) t.ok[c] = 0;
    if (win == 0) return;                                         // uniform: no hypothesis with 2 inliers from 2 images
    if (best == win) {                                            // the keys are distinct
        sX[0] = bestX[0];
        sX[1] = bestX[1];
        sX[2] = bestX[2];
    }
    __syncthreads();
    double X[3] = {sX[0], sX[1], sX[2]};
    // -- refit over the winner's inliers: the point closest to their rays ---------------------------------------------------------------------
    int first;
    bool two_images;
    double err_sum;
    int n_in = mark_inliers<NT>(el, L, X, t.max_err_sq, ured, &first, &two_images, &err_sum, dred);
    double s[kSums];
    for (int j = 0; j < kSums; ++j) s[j] = 0.0;
    for (int k = tid; k < L; k += NT) {
        if (el.unit(k)[3] == 0.0) continue;
        const double *d = el.dir(k), *cc = el.centre(k);
        const double dc = (d[0] * cc[0] + d[1] * cc[1]) + d[2] * cc[2];
        s[0] = s[0] + (1.0 - d[0] * d[0]);
        s[1] = s[1] + (0.0 - d[0] * d[1]);
        s[2] = s[2] + (0.0 - d[0] * d[2]);
        s[3] = s[3] + (1.0 - d[1] * d[1]);
        s[4] = s[4] + (0.0 - d[1] * d[2]);
        s[5] = s[5] + (1.0 - d[2] * d[2]);
        s[6] = s[6] + (cc[0] - d[0] * dc);
        s[7] = s[7] + (cc[1] - d[1] * dc);
        s[8] = s[8] + (cc[2] - d[2] * dc);
    }
    block_sums<NT>(s, 9, dred);
    double Xfit[3];
    solve_sym3(s, s + 6, Xfit);
    const double floor_cost = (double)n_in * OPSTR_COST_FLOOR;
    double cost_fit = cost_of<NT>(el, L, Xfit, dred);
    if (cost_fit < floor_cost) cost_fit = 0.0;
    // -- Gauss-Newton on the squared reprojection error of those inliers ----------------------------------------------------------------------
    X[0] = Xfit[0];
    X[1] = Xfit[1];
    X[2] = Xfit[2];
    for (int step = 0; step < t.refine_steps; ++step) {
        for (int j = 0; j < 9; ++j) s[j] = 0.0;
        for (int k = tid; k < L; k += NT) {
            if (el.unit(k)[3] == 0.0) continue;
            const double* P = el.P(k);
            double u, v, z;
            project(P, X, &u, &v, &z);
            const double ru = u - el.xy(k)[0], rv = v - el.xy(k)[1];
            double ju[3], jv[3];
            for (int j = 0; j < 3; ++j) {
                ju[j] = (P[j] - u * P[8 + j]) / z;
                jv[j] = (P[4 + j] - v * P[8 + j]) / z;
            }
            s[0] = s[0] + (ju[0] * ju[0] + jv[0] * jv[0]);
            s[1] = s[1] + (ju[0] * ju[1] + jv[0] * jv[1]);
            s[2] = s[2] + (ju[0] * ju[2] + jv[0] * jv[2]);
            s[3] = s[3] + (ju[1] * ju[1] + jv[1] * jv[1]);
            s[4] = s[4] + (ju[1] * ju[2] + jv[1] * jv[2]);
            s[5] = s[5] + (ju[2] * ju[2] + jv[2] * jv[2]);
            s[6] = s[6] + (ju[0] * ru + jv[0] * rv);
            s[7] = s[7] + (ju[1] * ru + jv[1] * rv);
            s[8] = s[8] + (ju[2] * ru + jv[2] * rv);
        }
        block_sums<NT>(s, 9, dred);
        double delta[3];
        solve_sym3(s, s + 6, delta);
        X[0] = X[0] - delta[0];
        X[1] = X[1] - delta[1];
        X[2] = X[2] - delta[2];
    }
    double cost_ref = cost_of<NT>(el, L, X, dred);
    if (cost_ref < floor_cost) cost_ref = 0.0;
    if (t.refine_steps < 1 || !(cost_ref < cost_fit)) {           // also when the steps left the finite numbers
        X[0] = Xfit[0];
        X[1] = Xfit[1];
        X[2] = Xfit[2];
    }
    // -- filter: the inliers of the final point, two images, one pair of rays at min_tri_angle or more ---------------------------------------
    n_in = mark_inliers<NT>(el, L, X, t.max_err_sq, ured, &first, &two_images, &err_sum, dred);
    if (n_in < 2 || !two_images) return;                          // uniform
    for (int k = tid; k < L; k += NT) {
        if (el.unit(k)[3] == 0.0) continue;
        const double* cc = el.centre(k);
        const double v0 = X[0] - cc[0], v1 = X[1] - cc[1], v2 = X[2] - cc[2];
        const double n = sqrt((v0 * v0 + v1 * v1) + v2 * v2);
        double* w = el.unit(k);
        w[0] = v0 / n;
        w[1] = v1 / n;
        w[2] = v2 / n;
    }
    __syncthreads();
    bool wide = false;
    for (int i = tid; i < L; i += NT) {
        const double* wi = el.unit(i);
        if (wi[3] == 0.0) continue;
        for (int j = i + 1; j < L; ++j) {
            const double* wj = el.unit(j);
            if (wj[3] == 0.0) continue;
            wide |= ((wi[0] * wj[0] + wi[1] * wj[1]) + wi[2] * wj[2]) <= t.cos_min_angle;
        }
    }
    if (!__syncthreads_or(wide)) return;
    for (int k = tid; k < L; k += NT)
        if (el.unit(k)[3] != 0.0) t.assigned[slots[k]] = t.point_base + c;
    if (tid == 0) {
        t.ok[c] = 1;
        t.xyz[3 * c] = X[0];
        t.xyz[3 * c + 1] = X[1];
        t.xyz[3 * c + 2] = X[2];
        t.point_error[c] = err_sum / (double)n_in;
        t.min_slot[c] = slots[first];
    }
}

// a component's element range, or false when the tables point outside
__device__ __forceinline__ bool component_range(const RoundTables& t, long long c, long long* e0, int* L) {
    if (c < 0 || c >= t.C) return false;
    const long long a = t.comp_offsets[c], b = t.comp_offsets[c + 1];
    if (a < 0 || b > t.n_elems || b < a || b - a > 0x3fffffff) return false;
    *e0 = a;
    *L = (int)(b - a);
    return true;
}

__global__ __launch_bounds__(kShort) void round_short_kernel(RoundTables t) {
    __shared__ double s_elem[kShort * kElemDoubles];
    __shared__ double s_unit[kShort * 4];
    __shared__ int s_img[kShort];
    __shared__ long long s_slot[kShort];
    __shared__ double s_red[kSums * kShort];
    __shared__ unsigned long long s_ured[kShort];
    __shared__ double s_X[3];
    const long long c = blockIdx.x;
    long long e0;
    int L;
    if (!component_range(t, c, &e0, &L)) return;
    if (L > kShort) return;                                       // the workgroup launch takes it
    if (L < 2) {
        if (threadIdx.x == 0) t.ok[c] = 0;
        return;
    }
    const int k = threadIdx.x;
    bool sound = true;
    if (k < L) {
        const long long slot = t.elem_slot[e0 + k];
        const long long img = (slot >= 0 && slot < t.U) ? t.slot_image[slot] : -1;
        sound = img >= 0 && img < t.I;
        s_slot[k] = sound ? slot : 0;
        s_img[k] = sound ? (int)img : 0;
        if (sound) {
            double* e = s_elem + kElemDoubles * k;
            const double* cam = t.cameras + kCam * img;
            for (int j = 0; j < 12; ++j) e[j] = cam[j];
            e[12] = t.xys[2 * slot];
            e[13] = t.xys[2 * slot + 1];
            for (int j = 0; j < 3; ++j) e[14 + j] = t.dirs[3 * slot + j];
            for (int j = 0; j < 3; ++j) e[17 + j] = cam[12 + j];
        }
        s_unit[4 * k + 3] = 0.0;
    }
    if (__syncthreads_or(!sound)) {
        if (threadIdx.x == 0) t.ok[c] = 0;
        return;
    }
    const LdsElems el{s_elem, s_img, s_unit};
    triangulate_component<kShort>(t, el, c, L, s_slot, s_red, s_ured, s_X);
}

__global__ __launch_bounds__(kThreads) void round_long_kernel(RoundTables t, const long long* long_comps, long long n_long) {
    __shared__ double s_red[kSums * kThreads];
    __shared__ unsigned long long s_ured[kThreads];
    __shared__ double s_X[3];
    if ((long long)blockIdx.x >= n_long) return;
    const long long c = long_comps[blockIdx.x];
    long long e0;
    int L;
    if (!component_range(t, c, &e0, &L)) return;
    if (L <= kShort) return;                                      // the wavefront launch took it
    bool sound = true;
    for (int k = threadIdx.x; k < L; k += kThreads) {
        const long long slot = t.elem_slot[e0 + k];
        const long long img = (slot >= 0 && slot < t.U) ? t.slot_image[slot] : -1;
        sound &= img >= 0 && img < t.I;
    }
    if (__syncthreads_or(!sound)) {
        if (threadIdx.x == 0) t.ok[c] = 0;
        return;
    }
    const GlobalElems el{t.elem_slot + e0, t.slot_image, t.xys, t.cameras, t.dirs, t.ws + 4 * e0};
    triangulate_component<kThreads>(t, el, c, L, t.elem_slot + e0, s_red, s_ured, s_X);
}

}  // namespace

extern "C" {

int opstr_abi_version(void) { return OPSTR_ABI_VERSION; }
const char* opstr_last_error(void) { return g_error; }

size_t opstr_workspace_bytes(long long n_elems) { return n_elems > 0 ? (size_t)n_elems * 4 * sizeof(double) : 0; }

int opstr_components(const long long* slot0, const long long* slot1, long long T, long long U, int* parent, long long* labels,
                     void* stream) {
    if (T < 0 || T > OPSTR_MAX_ITEMS || U < 1 || U > OPSTR_MAX_ITEMS) return bad_arg(__func__, "table sizes");
    if ((T > 0 && (!slot0 || !slot1)) || !parent || !labels) return bad_arg(__func__, "null pointer");
    hipStream_t s = (hipStream_t)stream;
    if (T > 0) hook_kernel<<<blocks_of(T, kThreads), kThreads, 0, s>>>(slot0, slot1, T, U, parent);
    flatten_kernel<<<blocks_of(U, kThreads), kThreads, 0, s>>>(parent, U, labels);
    CAPI_CHECK_LAUNCH();
    return 0;
}

int opstr_prepare(const double* K, const double* R, const double* t, const double* xys, const long long* slot_image, int I, long long U,
                  double* cameras, double* dirs, void* stream) {
    if (I < 1 || U < 1 || U > OPSTR_MAX_ITEMS) return bad_arg(__func__, "table sizes");
    if (!K || !R || !t || !xys || !slot_image || !cameras || !dirs) return bad_arg(__func__, "null pointer");
    hipStream_t s = (hipStream_t)stream;
    camera_kernel<<<blocks_of(I, kThreads), kThreads, 0, s>>>(K, R, t, I, cameras);
    dir_kernel<<<blocks_of(U, kThreads), kThreads, 0, s>>>(K, R, xys, slot_image, I, U, dirs);
    CAPI_CHECK_LAUNCH();
    return 0;
}

int opstr_round(const long long* comp_offsets, const long long* comp_label, const long long* elem_slot, const long long* long_comps,
                long long C, long long n_long, long long n_elems, const long long* slot_image, const double* xys, const double* cameras,
                const double* dirs, int I, long long U, int round, double max_reproj_error, double cos_min_tri_angle,
                int max_hypotheses, int refine_steps, long long point_base, void* workspace, size_t workspace_bytes, int* ok, double* xyz,
                double* point_error, long long* min_slot, long long* assigned, void* stream) {
    if (C < 1 || C > OPSTR_MAX_ITEMS || n_long < 0 || n_long > C || n_elems < 1 || n_elems > OPSTR_MAX_ITEMS || I < 1 || U < 1 ||
        U > OPSTR_MAX_ITEMS || point_base < 0)
        return bad_arg(__func__, "table sizes");
    if (round < 0 || round > OPSTR_MAX_ROUNDS || max_hypotheses < 1 || max_hypotheses > OPSTR_MAX_HYPOTHESES || refine_steps < 0 ||
        refine_steps > OPSTR_MAX_REFINE_STEPS || !(max_reproj_error >= 0.0) || !(cos_min_tri_angle >= -1.0 && cos_min_tri_angle <= 1.0))
        return bad_arg(__func__, "options");
    if (!comp_offsets || !comp_label || !elem_slot || (n_long > 0 && !long_comps) || !slot_image || !xys || !cameras || !dirs || !ok || !xyz ||
        !point_error || !min_slot || !assigned)
        return bad_arg(__func__, "null pointer");
    if (n_long > 0 && (!workspace || workspace_bytes < opstr_workspace_bytes(n_elems))) return bad_arg(__func__, "workspace too small");
    hipStream_t s = (hipStream_t)stream;
    const RoundTables t{comp_offsets, comp_label, elem_slot, slot_image, xys, cameras, dirs, C, n_elems, U, point_base, I, round,
                        max_hypotheses, refine_steps, max_reproj_error * max_reproj_error, cos_min_tri_angle, (double*)workspace, ok, xyz,
                        point_error, min_slot, assigned};
    round_short_kernel<<<(unsigned)C, kShort, 0, s>>>(t);
    if (n_long > 0) round_long_kernel<<<(unsigned)n_long, kThreads, 0, s>>>(t, long_comps, n_long);
    CAPI_CHECK_LAUNCH();
    return 0;
}

}  // extern "C"
