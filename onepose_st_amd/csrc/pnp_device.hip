// Device PnP (include/onepose_pnp_device.h): the pose of a frame from the matcher's device-side matches without a
// host round trip.  The arithmetic is the host solver's (csrc_host/pnp.cpp: p3p_poses, count_inliers, refine_lm, finish), statement by
// statement in float64; what differs is the sampler (counter-based, so scheduling cannot change a draw) and that every trial runs.
//
//   ranges, prep   ranges_kernel (device_loop.h): one thread per frame, two binary searches in b_ids; prep_kernel: one thread per row
//   sample         sample_kernel: one thread per (frame, trial), three splitmix64 draws without a rejection loop (draw3, device_loop.h)
//   p3p            p3p_kernel: one thread per (frame, trial): Grunert's quartic, Ferrari + three Newton steps, triangle alignment
//   score          score_kernel: one lane per hypothesis with the pose in registers; the frame's rows go through LDS in chunks of
//                  OPPNPD_SCORE_CHUNK and are read at a wave-uniform address; count and cost are per-lane sums in row order
//   select         select_partial_kernel: one workgroup per OPPNPD_SELECT_BLOCK hypotheses; select_final_kernel: one workgroup per
//                  frame over the partial bests, then the winner's inlier mask.  A total order, so the tree's shape cannot change the winner.
//   refine         refine_kernel: one workgroup per frame; normal equations and costs as per-thread partial sums in row order and a
//                  fixed tree over the threads in LDS; the 6 x 6 solve on thread 0
// No workgroup waits for another, every loop is bounded at compile time or by a table size, no atomics on floats: two runs agree bit
// for bit.  Compiled with contraction off: every expression is evaluated in the written order.
#include <hip/hip_runtime.h>
#include <math.h>
#include <stdint.h>
#include "onepose_pnp_device.h"
#include "capi_error.h"
#include "device_loop.h"
#include "reduce_f64.h"

using capi::bad_arg;
using capi::blocks_of;
using capi::fail;
using capi::g_error;
using devloop::align_up;
using devloop::block_best;
using devloop::clamped_count;
using devloop::draw3;
using devloop::mask_clear_kernel;
using devloop::ranges_kernel;
using devloop::row_range;

#pragma clang fp contract(off)

namespace {

constexpr int kThreads = 256;                     // 4 waves of 64
constexpr int kRow = OPPNPD_ROW_DOUBLES;
constexpr int kChunk = OPPNPD_SCORE_CHUNK;
constexpr int kSelBlock = OPPNPD_SELECT_BLOCK;
constexpr int kSums = 27;                         // 21 entries of the upper triangle of J^T J and 6 of the gradient
constexpr int kMinIn = OPPNPD_MIN_INLIERS;

struct Intr { double fx, sk, cx, fy, cy; };

__device__ __forceinline__ Intr load_intr(const double* K, int k_shared, int f) {
    const double* k = K + (k_shared ? 0 : (size_t)f * 9);
    return Intr{k[0], k[1], k[2], k[4], k[5]};
}

// count_inliers' expression (csrc_host/pnp.cpp): true when the row is an inlier; `add` = what the row adds to the truncated cost
__device__ __forceinline__ bool row_inlier(const double* ps, double x0, double x1, double x2, double pu, double pv, const Intr& I, double thr2,
                                           double& add) {
    const double xc = ps[0] * x0 + ps[1] * x1 + ps[2] * x2 + ps[3];
    const double yc = ps[4] * x0 + ps[5] * x1 + ps[6] * x2 + ps[7];
    const double zc = ps[8] * x0 + ps[9] * x1 + ps[10] * x2 + ps[11];
    bool in = false;
    add = thr2;
    if (zc > 1e-12) {
        const double xn = xc / zc, yn = yc / zc;
        const double du = I.fx * xn + I.sk * yn + I.cx - pu, dv = I.fy * yn + I.cy - pv;
        const double e2 = du * du + dv * dv;
        in = e2 < thr2;
        add = in ? e2 : thr2;
    }
    return in;
}

// ---- ranges, prep ------------------------------------------------------------------------------------------------------------------------
__global__ void prep_kernel(const float* pts2d, const float* pts3d, const int* count, int cap, const long long* b_ids, int F, const double* K,
                            int k_shared, double scale, double* rows) {
    const int i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= clamped_count(count, cap)) return;
    double* o = rows + (size_t)i * kRow;
    const long long f = b_ids ? b_ids[i] : 0;
    if (f < 0 || f >= F) {
        for (int d = 0; d < kRow; ++d) o[d] = 0.0;
        return;
    }
    const double* m = K + (k_shared ? 0 : (size_t)f * 9);
    // inv3 of the host solver
    const double det = m[0] * (m[4] * m[8] - m[5] * m[7]) - m[1] * (m[3] * m[8] - m[5] * m[6]) + m[2] * (m[3] * m[7] - m[4] * m[6]);
    const double id = 1.0 / det;
    const double k0 = (m[4] * m[8] - m[5] * m[7]) * id, k1 = (m[2] * m[7] - m[1] * m[8]) * id, k2 = (m[1] * m[5] - m[2] * m[4]) * id;
    const double k3 = (m[5] * m[6] - m[3] * m[8]) * id, k4 = (m[0] * m[8] - m[2] * m[6]) * id, k5 = (m[2] * m[3] - m[0] * m[5]) * id;
    const double k6 = (m[3] * m[7] - m[4] * m[6]) * id, k7 = (m[1] * m[6] - m[0] * m[7]) * id, k8 = (m[0] * m[4] - m[1] * m[3]) * id;
    const double u = pts2d[2 * (size_t)i], v = pts2d[2 * (size_t)i + 1];
    const double w = k6 * u + k7 * v + k8;
    o[0] = scale * (double)pts3d[3 * (size_t)i]; o[1] = scale * (double)pts3d[3 * (size_t)i + 1]; o[2] = scale * (double)pts3d[3 * (size_t)i + 2];
    o[3] = u; o[4] = v;
    o[5] = (k0 * u + k1 * v + k2) / w;
    o[6] = (k3 * u + k4 * v + k5) / w;
    o[7] = 0.0;
}

// ---- sample ------------------------------------------------------------------------------------------------------------------------------
__global__ void sample_kernel(const int* ranges, int cap, int F, int trials, uint64_t seed, int* samples) {
    const int t = blockIdx.x * blockDim.x + threadIdx.x, f = blockIdx.y;
    if (t >= trials) return;
    int begin, end;
    row_range(ranges, f, cap, begin, end);
    const int n = end - begin;
    int* o = samples + ((size_t)f * trials + t) * 3;
    if (n < kMinIn) { o[0] = o[1] = o[2] = -1; return; }
    int a, b, c;
    draw3(seed, f, t, n, a, b, c);
    o[0] = a; o[1] = b; o[2] = c;
}

// ---- p3p ---------------------------------------------------------------------------------------------------------------------------------
// largest real root of z^3 + A z^2 + B z + C
__device__ double cubic_largest_root(double A, double B, double C) {
    const double a3 = A / 3.0;
    const double P = B - A * a3, Q = 2.0 * a3 * a3 * a3 - a3 * B + C;
    const double disc = 0.25 * Q * Q + P * P * P / 27.0;
    double w;
    if (disc > 0.0) {
        const double sq = sqrt(disc);
        w = cbrt(-0.5 * Q + sq) + cbrt(-0.5 * Q - sq);
    } else {
        const double m = 2.0 * sqrt(-P / 3.0);
        double arg = m > 0.0 ? 3.0 * Q / (P * m) : 0.0;
        arg = arg < -1.0 ? -1.0 : (arg > 1.0 ? 1.0 : arg);
        w = m * cos(acos(arg) / 3.0);
    }
    double z = w - a3;
    for (int it = 0; it < 3; ++it) {
        const double f = ((z + A) * z + B) * z + C, df = (3.0 * z + 2.0 * A) * z + B;
        if (fabs(df) < 1e-300) break;
        z -= f / df;
    }
    return z;
}

// real roots of c4 x^4 + ... + c0 (Ferrari, three Newton steps on the original polynomial); y0 .. y3 in the host's order
__device__ int quartic_real_roots(const double* c, double& r0, double& r1, double& r2, double& r3) {
    if (!(fabs(c[4]) > 1e-14 * (fabs(c[3]) + fabs(c[2]) + fabs(c[1]) + fabs(c[0]) + 1e-300))) return 0;
    const double a = c[3] / c[4], b = c[2] / c[4], cc = c[1] / c[4], d = c[0] / c[4];
    const double a2 = a * a;
    const double p = b - 0.375 * a2, q = cc - 0.5 * a * b + 0.125 * a2 * a, r = d - 0.25 * a * cc + 0.0625 * a2 * b - (3.0 / 256.0) * a2 * a2;
    double y0 = 0.0, y1 = 0.0, y2 = 0.0, y3 = 0.0;
    int n = 0;
    auto push = [&](double v) {
        if (n == 0) y0 = v; else if (n == 1) y1 = v; else if (n == 2) y2 = v; else y3 = v;
        ++n;
    };
    const double scale = fabs(p) + sqrt(fabs(r)) + 1e-300;
    if (fabs(q) < 1e-12 * scale * sqrt(scale)) {                 // biquadratic
        double disc = p * p - 4.0 * r;
        if (disc < 0.0) { if (disc > -1e-12 * scale * scale) disc = 0.0; else return 0; }
        const double sq = sqrt(disc);
        const double w0 = 0.5 * (-p + sq), w1 = 0.5 * (-p - sq);
        if (!(w0 < 0.0)) { const double s = sqrt(w0); push(s); push(-s); }
        if (!(w1 < 0.0)) { const double s = sqrt(w1); push(s); push(-s); }
    } else {
        const double z = cubic_largest_root(2.0 * p, p * p - 4.0 * r, -q * q);
        if (!(z > 0.0)) return 0;
        const double s = sqrt(z), t1 = 0.5 * (p + z - q / s), t2 = 0.5 * (p + z + q / s);
        const double tol = 1e-10 * (z + fabs(t1) + fabs(t2));
        double d1 = z - 4.0 * t1, d2 = z - 4.0 * t2;
        if (d1 > -tol) { d1 = sqrt(d1 > 0.0 ? d1 : 0.0); push(0.5 * (-s + d1)); push(0.5 * (-s - d1)); }
        if (d2 > -tol) { d2 = sqrt(d2 > 0.0 ? d2 : 0.0); push(0.5 * (s + d2)); push(0.5 * (s - d2)); }
    }
    auto polish = [&](double y) {
        double x = y - 0.25 * a;
        bool live = true;
        for (int it = 0; it < 3; ++it) {
            const double f = (((c[4] * x + c[3]) * x + c[2]) * x + c[1]) * x + c[0];
            const double df = ((4.0 * c[4] * x + 3.0 * c[3]) * x + 2.0 * c[2]) * x + c[1];
            live = live && fabs(df) >= 1e-300;
            if (live) x -= f / df;
        }
        return x;
    };
    r0 = polish(y0); r1 = polish(y1); r2 = polish(y2); r3 = polish(y3);
    return n;
}

__global__ __launch_bounds__(kThreads) void p3p_kernel(const double* rows, const int* ranges, const int* samples, int cap, int F, int trials,
                                                       double* hyps, int* nsol) {
    const int t = blockIdx.x * blockDim.x + threadIdx.x, f = blockIdx.y;
    if (t >= trials) return;
    double* out = hyps + ((size_t)f * trials + t) * 48;
    const double nan = __longlong_as_double(0x7FF8000000000000ll);
    int begin, end;
    row_range(ranges, f, cap, begin, end);
    const int n = end - begin;
    const int* s = samples + ((size_t)f * trials + t) * 3;
    const int i0 = s[0], i1 = s[1], i2 = s[2];
    int written = 0;
    const bool usable = n >= kMinIn && i0 >= 0 && i0 < n && i1 >= 0 && i1 < n && i2 >= 0 && i2 < n;
    if (usable) {
        double X[3][3], fb[3][3];
        const int idx[3] = {i0, i1, i2};
        for (int i = 0; i < 3; ++i) {
            const double* r = rows + (size_t)(begin + idx[i]) * kRow;
            X[i][0] = r[0]; X[i][1] = r[1]; X[i][2] = r[2];
            const double rx = r[5], ry = r[6];
            const double inv = 1.0 / sqrt(rx * rx + ry * ry + 1.0);
            fb[i][0] = rx * inv; fb[i][1] = ry * inv; fb[i][2] = inv;
        }
        auto dot = [](const double* a, const double* b) { return a[0] * b[0] + a[1] * b[1] + a[2] * b[2]; };
        auto d2 = [](const double* a, const double* b) {
            return (a[0] - b[0]) * (a[0] - b[0]) + (a[1] - b[1]) * (a[1] - b[1]) + (a[2] - b[2]) * (a[2] - b[2]);
        };
        const double ca = dot(fb[1], fb[2]), cb = dot(fb[0], fb[2]), cg = dot(fb[0], fb[1]);
        const double a2 = d2(X[1], X[2]), b2 = d2(X[0], X[2]), c2 = d2(X[0], X[1]);
        bool ok = a2 > 0.0 && b2 > 0.0 && c2 > 0.0;
        // triangle_frame of the world points: EP[i * 3 + k] = component i of axis k
        double EP[9];
        if (ok) {
            double e1[3] = {X[1][0] - X[0][0], X[1][1] - X[0][1], X[1][2] - X[0][2]}, w[3] = {X[2][0] - X[0][0], X[2][1] - X[0][1], X[2][2] - X[0][2]};
            const double n1 = sqrt(e1[0] * e1[0] + e1[1] * e1[1] + e1[2] * e1[2]);
            ok = n1 > 1e-300;
            if (ok) {
                for (int i = 0; i < 3; ++i) e1[i] /= n1;
                double e3[3] = {e1[1] * w[2] - e1[2] * w[1], e1[2] * w[0] - e1[0] * w[2], e1[0] * w[1] - e1[1] * w[0]};
                const double n3 = sqrt(e3[0] * e3[0] + e3[1] * e3[1] + e3[2] * e3[2]);
                const double nw = sqrt(w[0] * w[0] + w[1] * w[1] + w[2] * w[2]);
                ok = n3 > 1e-9 * nw && nw > 0.0;
                if (ok) {
                    for (int i = 0; i < 3; ++i) e3[i] /= n3;
                    const double e2[3] = {e3[1] * e1[2] - e3[2] * e1[1], e3[2] * e1[0] - e3[0] * e1[2], e3[0] * e1[1] - e3[1] * e1[0]};
                    for (int i = 0; i < 3; ++i) { EP[i * 3] = e1[i]; EP[i * 3 + 1] = e2[i]; EP[i * 3 + 2] = e3[i]; }
                }
            }
        }
        if (ok) {
            const double p = (a2 - c2) / b2, k = c2 / b2;
            const double N[3] = {p + 1.0, -2.0 * p * cb, p - 1.0}, D[2] = {2.0 * cg, -2.0 * ca}, E[3] = {1.0, -2.0 * cb, 1.0};
            const double D2[3] = {D[0] * D[0], 2.0 * D[0] * D[1], D[1] * D[1]};
            double c[5] = {D2[0], D2[1], D2[2], 0.0, 0.0};
#pragma unroll
            for (int i = 0; i < 3; ++i)
#pragma unroll
                for (int j = 0; j < 3; ++j) c[i + j] += N[i] * N[j] - k * E[i] * D2[j];
#pragma unroll
            for (int i = 0; i < 3; ++i)
#pragma unroll
                for (int j = 0; j < 2; ++j) c[i + j] -= 2.0 * cg * N[i] * D[j];
            double vs0 = 0.0, vs1 = 0.0, vs2 = 0.0, vs3 = 0.0;
            const int nr = quartic_real_roots(c, vs0, vs1, vs2, vs3);
            for (int ri = 0; ri < nr && ri < 4; ++ri) {
                const double v = ri == 0 ? vs0 : (ri == 1 ? vs1 : (ri == 2 ? vs2 : vs3));
                bool good = v > 0.0 && isfinite(v);
                for (int rj = 0; rj < ri; ++rj) {
                    const double o = rj == 0 ? vs0 : (rj == 1 ? vs1 : vs2);
                    good = good && !(fabs(o - v) < 1e-9 * (1.0 + fabs(v)));      // a double root counted once
                }
                const double den = D[0] + D[1] * v;
                good = good && fabs(den) >= 1e-12;
                const double u = (N[0] + (N[1] + N[2] * v) * v) / (good ? den : 1.0);
                good = good && u > 0.0;
                const double q = 1.0 + u * u - (2.0 * cg) * u;
                good = good && q > 1e-300;
                const double s1 = sqrt(c2 / (good ? q : 1.0));
                const double sd[3] = {s1, u * s1, v * s1};
                double Cc[3][3];
                for (int i = 0; i < 3; ++i)
                    for (int d = 0; d < 3; ++d) Cc[i][d] = sd[i] * fb[i][d];
                double e1[3] = {Cc[1][0] - Cc[0][0], Cc[1][1] - Cc[0][1], Cc[1][2] - Cc[0][2]}, w[3] = {Cc[2][0] - Cc[0][0], Cc[2][1] - Cc[0][1], Cc[2][2] - Cc[0][2]};
                const double n1 = sqrt(e1[0] * e1[0] + e1[1] * e1[1] + e1[2] * e1[2]);
                good = good && n1 > 1e-300;
                const double in1 = 1.0 / (good ? n1 : 1.0);
                for (int i = 0; i < 3; ++i) e1[i] *= in1;
                double e3[3] = {e1[1] * w[2] - e1[2] * w[1], e1[2] * w[0] - e1[0] * w[2], e1[0] * w[1] - e1[1] * w[0]};
                const double n3 = sqrt(e3[0] * e3[0] + e3[1] * e3[1] + e3[2] * e3[2]);
                const double nw = sqrt(w[0] * w[0] + w[1] * w[1] + w[2] * w[2]);
                good = good && n3 > 1e-9 * nw && nw > 0.0;
                const double in3 = 1.0 / (good ? n3 : 1.0);
                for (int i = 0; i < 3; ++i) e3[i] *= in3;
                const double e2[3] = {e3[1] * e1[2] - e3[2] * e1[1], e3[2] * e1[0] - e3[0] * e1[2], e3[0] * e1[1] - e3[1] * e1[0]};
                double ps[12];
                double fin_sum = 0.0;
                for (int i = 0; i < 3; ++i) {
                    for (int j = 0; j < 3; ++j) ps[i * 4 + j] = e1[i] * EP[j * 3] + e2[i] * EP[j * 3 + 1] + e3[i] * EP[j * 3 + 2];
                    ps[i * 4 + 3] = Cc[0][i] - (ps[i * 4] * X[0][0] + ps[i * 4 + 1] * X[0][1] + ps[i * 4 + 2] * X[0][2]);
                    for (int j = 0; j < 4; ++j) fin_sum += fabs(ps[i * 4 + j]);
                }
                good = good && fin_sum < 1e300;                           // every entry finite
                if (good && written < 4) {
                    for (int e = 0; e < 12; ++e) out[written * 12 + e] = ps[e];
                    ++written;
                }
            }
        }
    }
    for (int e = written * 12; e < 48; ++e) out[e] = nan;
    nsol[(size_t)f * trials + t] = written;
}

// ---- score -------------------------------------------------------------------------------------------------------------------------------
__global__ __launch_bounds__(kThreads) void score_kernel(const double* rows, const int* ranges, const double* K, int k_shared, const double* hyps,
                                                         int cap, int F, int H, double thr2, int* cnt_out, double* cost_out) {
    __shared__ double sh[kChunk][5];
    const int h = blockIdx.x * kThreads + threadIdx.x, f = blockIdx.y;
    int begin, end;
    row_range(ranges, f, cap, begin, end);
    const Intr I = load_intr(K, k_shared, f);
    double ps[12];
    bool finite = h < H;
    for (int e = 0; e < 12; ++e) {
        ps[e] = h < H ? hyps[((size_t)f * H + h) * 12 + e] : 0.0;
        finite = finite && isfinite(ps[e]);
    }
    int cnt = 0;
    double cost = 0.0;
    for (int c0 = begin; c0 < end; c0 += kChunk) {
        const int len = end - c0 < kChunk ? end - c0 : kChunk;
        __syncthreads();
        if ((int)threadIdx.x < len) {
            const double* r = rows + (size_t)(c0 + threadIdx.x) * kRow;
            for (int d = 0; d < 5; ++d) sh[threadIdx.x][d] = r[d];
        }
        __syncthreads();
        if (finite) {
            for (int j = 0; j < len; ++j) {
                double add;
                cnt += row_inlier(ps, sh[j][0], sh[j][1], sh[j][2], sh[j][3], sh[j][4], I, thr2, add) ? 1 : 0;
                cost += add;
            }
        }
    }
    if (h < H) {
        cnt_out[(size_t)f * H + h] = finite ? cnt : 0;
        cost_out[(size_t)f * H + h] = finite ? cost : __longlong_as_double(0x7FF0000000000000ll);
    }
}

// ---- select ------------------------------------------------------------------------------------------------------------------------------
struct Best { int cnt; int idx; double cost; };       // 16 bytes: an entry of the partial table

__device__ __forceinline__ bool better(const Best& a, const Best& b) {      // a before b in the total order; idx < 0: no candidate
    if (a.idx < 0) return false;
    if (b.idx < 0) return true;
    if (a.cnt != b.cnt) return a.cnt > b.cnt;
    if (a.cost < b.cost) return true;
    if (b.cost < a.cost) return false;
    return a.idx < b.idx;
}

__global__ __launch_bounds__(kThreads) void select_partial_kernel(const int* cnt, const double* cost, int F, int H, int nblk, Best* partial) {
    __shared__ Best sh[kThreads];
    const int f = blockIdx.y, blk = blockIdx.x;
    Best mine{0, -1, 0.0};
    for (int j = 0; j < kSelBlock / kThreads; ++j) {
        const int h = blk * kSelBlock + j * kThreads + threadIdx.x;
        if (h >= H) continue;
        const Best c{cnt[(size_t)f * H + h], h, cost[(size_t)f * H + h]};
        if (c.cnt > 0 && better(c, mine)) mine = c;
    }
    const Best r = block_best<kThreads>(mine, sh);
    if (threadIdx.x == 0) partial[(size_t)f * nblk + blk] = r;
}

__global__ __launch_bounds__(kThreads) void select_final_kernel(const Best* partial, int nblk, const double* rows, const int* ranges, const double* K,
                                                                int k_shared, const double* hyps, int cap, int F, int H, double thr2, double confidence,
                                                                int trials, int* best, int* n_inliers, int* status, unsigned char* mask) {
    __shared__ Best sh[kThreads];
    const int f = blockIdx.x;
    Best mine{0, -1, 0.0};
    for (int b = threadIdx.x; b < nblk; b += kThreads) {          // ascending blocks per thread; the order is total, so any tree gives the same winner
        const Best c = partial[(size_t)f * nblk + b];
        if (c.idx >= 0 && c.idx < H && better(c, mine)) mine = c;
    }
    const Best r = block_best<kThreads>(mine, sh);
    int begin, end;
    row_range(ranges, f, cap, begin, end);
    const int n = end - begin;
    const int won = r.idx >= 0 ? r.cnt : 0;
    if (threadIdx.x == 0) {
        int st = won < kMinIn ? OPPNPD_STATUS_NO_POSE : 0;
        if (n >= kMinIn) {                                        // needed_for of the host solver
            const double w = (double)won / (double)n, pw = w * w * w;
            double needed;
            if (pw > 1.0 - 1e-12) needed = 1.0;
            else if (pw > 1e-12) {
                needed = ceil(log(1.0 - confidence) / log(1.0 - pw));
                if (!(needed < (double)OPPNPD_MAX_NEEDED)) needed = (double)OPPNPD_MAX_NEEDED;
            } else needed = (double)OPPNPD_MAX_NEEDED;
            if (needed > (double)trials) st |= OPPNPD_STATUS_NEEDS_MORE;
        }
        best[f] = r.idx;
        n_inliers[f] = won;
        status[f] = st;
    }
    if (r.idx < 0) return;                                        // (the mask was cleared before this launch)
    const Intr I = load_intr(K, k_shared, f);
    double ps[12];
    for (int e = 0; e < 12; ++e) ps[e] = hyps[((size_t)f * H + r.idx) * 12 + e];
    for (int i = begin + threadIdx.x; i < end; i += kThreads) {
        const double* x = rows + (size_t)i * kRow;
        double add;
        mask[i] = row_inlier(ps, x[0], x[1], x[2], x[3], x[4], I, thr2, add) ? 1 : 0;
    }
}

// ---- refine ------------------------------------------------------------------------------------------------------------------------------
// refine_lm's cost on the masked rows of [begin, end): per-thread partials in row order, then the tree
__device__ __forceinline__ double lm_cost(const double* ps, const double* rows, const unsigned char* mask, int begin, int end, const Intr& I, double* red) {
    double c[1] = {0.0};
    for (int i = begin + threadIdx.x; i < end; i += kThreads) {
        if (!mask[i]) continue;
        const double* x = rows + (size_t)i * kRow;
        const double xc = ps[0] * x[0] + ps[1] * x[1] + ps[2] * x[2] + ps[3];
        const double yc = ps[4] * x[0] + ps[5] * x[1] + ps[6] * x[2] + ps[7];
        const double zc = ps[8] * x[0] + ps[9] * x[1] + ps[10] * x[2] + ps[11];
        const bool front = zc > 1e-12;
        const double izc = 1.0 / (front ? zc : 1.0);
        const double xn = xc * izc, yn = yc * izc;
        const double du = I.fx * xn + I.sk * yn + I.cx - x[3], dv = I.fy * yn + I.cy - x[4];
        c[0] += front ? du * du + dv * dv : 1e12;
    }
    red64::block_sums<kThreads>(c, 1, red);
    return c[0];
}

__global__ __launch_bounds__(kThreads) void refine_kernel(const double* rows, const int* ranges, const double* K, int k_shared, const double* hyps,
                                                          const int* best, int cap, int F, int H, double thr2, double scale, double* pose_out,
                                                          int* n_inliers, int* status, unsigned char* mask) {
    __shared__ double red[kSums][kThreads];
    __shared__ double sh_pose[12], sh_np[12], sh_M[6][7], sh_H[36], sh_g[6];
    __shared__ int sh_ok, sh_cnt, sh_changed;
    const int f = blockIdx.x, tid = threadIdx.x;
    int begin, end;
    row_range(ranges, f, cap, begin, end);
    const int n = end - begin;
    const int b = best[f];
    const int keep_bits = status[f] & OPPNPD_STATUS_NEEDS_MORE;
    const Intr I = load_intr(K, k_shared, f);
    bool have = b >= 0 && b < H && n >= kMinIn && n_inliers[f] >= kMinIn;
    int cnt = 0;
    if (have) {
        if (tid < 12) sh_pose[tid] = hyps[((size_t)f * H + b) * 12 + tid];
        __syncthreads();
        for (int round = 0; round < OPPNPD_LM_ROUNDS; ++round) {
            // ---- refine_lm: every thread holds the same lambda / cur / flags, computed from shared values
            double lambda = 1e-3;
            double cur = lm_cost(sh_pose, rows, mask, begin, end, I, red[0]);
            bool done = false;
            for (int it = 0; it < OPPNPD_LM_ITERS && !done; ++it) {
                double acc[kSums];
#pragma unroll
                for (int e = 0; e < kSums; ++e) acc[e] = 0.0;
                for (int i = begin + tid; i < end; i += kThreads) {
                    if (!mask[i]) continue;
                    const double* x = rows + (size_t)i * kRow;
                    const double pc0 = sh_pose[0] * x[0] + sh_pose[1] * x[1] + sh_pose[2] * x[2] + sh_pose[3];
                    const double pc1 = sh_pose[4] * x[0] + sh_pose[5] * x[1] + sh_pose[6] * x[2] + sh_pose[7];
                    const double pc2 = sh_pose[8] * x[0] + sh_pose[9] * x[1] + sh_pose[10] * x[2] + sh_pose[11];
                    if (!(pc2 > 1e-12)) continue;                 // behind the camera: weight 0, contributes nothing
                    const double iz = 1.0 / pc2, xn = pc0 * iz, yn = pc1 * iz;
                    const double ru = I.fx * xn + I.sk * yn + I.cx - x[3], rv = I.fy * yn + I.cy - x[4];
                    const double Ju[3] = {I.fx * iz, I.sk * iz, -(I.fx * xn + I.sk * yn) * iz};
                    const double Jv[3] = {0.0, I.fy * iz, -I.fy * yn * iz};
                    const double q[3] = {pc0 - sh_pose[3], pc1 - sh_pose[7], pc2 - sh_pose[11]};
                    double ju[6], jv[6];
                    ju[0] = -Ju[1] * q[2] + Ju[2] * q[1]; ju[1] = Ju[0] * q[2] - Ju[2] * q[0]; ju[2] = -Ju[0] * q[1] + Ju[1] * q[0];
                    jv[0] = -Jv[1] * q[2] + Jv[2] * q[1]; jv[1] = Jv[0] * q[2] - Jv[2] * q[0]; jv[2] = -Jv[0] * q[1] + Jv[1] * q[0];
#pragma unroll
                    for (int k = 0; k < 3; ++k) { ju[3 + k] = Ju[k]; jv[3 + k] = Jv[k]; }
                    int e = 0;
#pragma unroll
                    for (int a = 0; a < 6; ++a) {
                        acc[21 + a] -= ju[a] * ru + jv[a] * rv;
#pragma unroll
                        for (int b2 = a; b2 < 6; ++b2) acc[e++] += ju[a] * ju[b2] + jv[a] * jv[b2];
                    }
                }
#pragma unroll
                for (int e = 0; e < kSums; ++e) red[e][tid] = acc[e];
                __syncthreads();
                for (int s = kThreads / 2; s > 0; s >>= 1) {
                    if (tid < s)
#pragma unroll
                        for (int e = 0; e < kSums; ++e) red[e][tid] = red[e][tid] + red[e][tid + s];
                    __syncthreads();
                }
                if (tid == 0) {
                    int e = 0;
                    for (int a = 0; a < 6; ++a) {
                        sh_g[a] = red[21 + a][0];
                        for (int b2 = a; b2 < 6; ++b2) { sh_H[a * 6 + b2] = red[e][0]; sh_H[b2 * 6 + a] = red[e][0]; ++e; }
                    }
                }
                __syncthreads();
                bool improved = false;
                for (int tries = 0; tries < OPPNPD_LM_TRIES && !improved; ++tries) {
                    if (tid == 0) {
                        // solve6: Gaussian elimination with partial pivoting on H with its diagonal scaled by 1 + lambda
                        for (int i = 0; i < 6; ++i) {
                            for (int j = 0; j < 6; ++j) sh_M[i][j] = i == j ? sh_H[i * 6 + j] * (1.0 + lambda) : sh_H[i * 6 + j];
                            sh_M[i][6] = sh_g[i];
                        }
                        bool ok = true;
                        for (int c = 0; c < 6 && ok; ++c) {
                            int piv = c;
                            for (int r = c + 1; r < 6; ++r) if (fabs(sh_M[r][c]) > fabs(sh_M[piv][c])) piv = r;
                            if (fabs(sh_M[piv][c]) < 1e-300) { ok = false; break; }
                            if (piv != c) for (int j = 0; j < 7; ++j) { const double tmp = sh_M[c][j]; sh_M[c][j] = sh_M[piv][j]; sh_M[piv][j] = tmp; }
                            for (int r = c + 1; r < 6; ++r) {
                                const double fac = sh_M[r][c] / sh_M[c][c];
                                for (int j = c; j < 7; ++j) sh_M[r][j] -= fac * sh_M[c][j];
                            }
                        }
                        if (ok) {
                            double dx[6];
                            for (int i = 5; i >= 0; --i) {
                                double s = sh_M[i][6];
                                for (int j = i + 1; j < 6; ++j) s -= sh_M[i][j] * dx[j];
                                dx[i] = s / sh_M[i][i];
                            }
                            // rodrigues
                            const double th = sqrt(dx[0] * dx[0] + dx[1] * dx[1] + dx[2] * dx[2]);
                            const double ra = th < 1e-12 ? 1.0 - th * th / 6.0 : sin(th) / th;
                            const double rb = th < 1e-12 ? 0.5 - th * th / 24.0 : (1.0 - cos(th)) / (th * th);
                            const double Kx[9] = {0, -dx[2], dx[1], dx[2], 0, -dx[0], -dx[1], dx[0], 0};
                            double dR[9];
                            for (int i = 0; i < 3; ++i)
                                for (int j = 0; j < 3; ++j) {
                                    double k2 = 0.0;
                                    for (int k = 0; k < 3; ++k) k2 += Kx[i * 3 + k] * Kx[k * 3 + j];
                                    dR[i * 3 + j] = (i == j ? 1.0 : 0.0) + ra * Kx[i * 3 + j] + rb * k2;
                                }
                            for (int r = 0; r < 3; ++r) {
                                for (int c = 0; c < 3; ++c) sh_np[r * 4 + c] = dR[r * 3] * sh_pose[c] + dR[r * 3 + 1] * sh_pose[4 + c] + dR[r * 3 + 2] * sh_pose[8 + c];
                                sh_np[r * 4 + 3] = sh_pose[r * 4 + 3] + dx[3 + r];
                            }
                        }
                        sh_ok = ok ? 1 : 0;
                    }
                    __syncthreads();
                    const bool ok = sh_ok != 0;
                    if (!ok) { lambda *= 10.0; __syncthreads(); continue; }
                    const double nc = lm_cost(sh_np, rows, mask, begin, end, I, red[0]);
                    if (nc < cur) {
                        if (tid < 12) sh_pose[tid] = sh_np[tid];
                        const double rel = (cur - nc) / (cur + 1e-300);
                        cur = nc;
                        lambda = lambda > 1e-9 ? lambda * 0.3 : lambda;
                        improved = true;
                        if (rel < 1e-12) done = true;
                    } else {
                        lambda *= 10.0;
                    }
                    __syncthreads();
                }
                if (!improved) done = true;
            }
            // ---- the inlier set under the refined pose
            if (tid == 0) { sh_cnt = 0; sh_changed = 0; }
            __syncthreads();
            int my_cnt = 0, my_changed = 0;
            for (int i = begin + tid; i < end; i += kThreads) {
                const double* x = rows + (size_t)i * kRow;
                double add;
                const unsigned char in = row_inlier(sh_pose, x[0], x[1], x[2], x[3], x[4], I, thr2, add) ? 1 : 0;
                my_changed |= (mask[i] != 0) != (in != 0);
                mask[i] = in;
                my_cnt += in;
            }
            if (my_cnt) atomicAdd(&sh_cnt, my_cnt);               // integers: the order of the additions does not matter
            if (my_changed) atomicOr(&sh_changed, 1);
            __syncthreads();
            cnt = sh_cnt;
            const bool changed = sh_changed != 0;
            __syncthreads();
            if (cnt < kMinIn || !changed) break;
        }
        have = cnt >= kMinIn;
    }
    if (!have) {
        for (int i = begin + tid; i < end; i += kThreads) mask[i] = 0;
        if (tid < 12) pose_out[(size_t)f * 12 + tid] = (tid == 0 || tid == 5 || tid == 10) ? 1.0 : 0.0;
        if (tid == 0) { n_inliers[f] = 0; status[f] = keep_bits | OPPNPD_STATUS_NO_POSE; }
        return;
    }
    if (tid < 12) pose_out[(size_t)f * 12 + tid] = (tid & 3) == 3 ? sh_pose[tid] / scale : sh_pose[tid];
    if (tid == 0) { n_inliers[f] = cnt; status[f] = keep_bits; }
}

// ---- argument checks ---------------------------------------------------------------------------------------------------------------------
bool sizes_ok(int cap, int F) { return cap >= 1 && cap <= OPPNPD_MAX_ROWS && F >= 1 && F <= OPPNPD_MAX_FRAMES; }
bool hyps_ok(int F, long long H) { return H >= 1 && H <= 4ll * OPPNPD_MAX_TRIALS && (long long)F * H <= (1ll << 26); }
bool thr_ok(double e) { return isfinite(e) && e > 0.0; }

struct Layout { size_t ranges, rows, samples, hyps, nsol, cnt, cost, partial, best, total; };

Layout layout_of(int cap, int F, int trials) {
    Layout L;
    const size_t H = 4 * (size_t)trials, nblk = (H + kSelBlock - 1) / kSelBlock;
    size_t o = 0;
    L.ranges = o; o = align_up(o + sizeof(int) * 2 * F);
    L.rows = o; o = align_up(o + sizeof(double) * kRow * (size_t)cap);
    L.samples = o; o = align_up(o + sizeof(int) * 3 * (size_t)F * trials);
    L.hyps = o; o = align_up(o + sizeof(double) * 12 * (size_t)F * H);
    L.nsol = o; o = align_up(o + sizeof(int) * (size_t)F * trials);
    L.cnt = o; o = align_up(o + sizeof(int) * (size_t)F * H);
    L.cost = o; o = align_up(o + sizeof(double) * (size_t)F * H);
    L.partial = o; o = align_up(o + sizeof(Best) * (size_t)F * nblk);
    L.best = o; o = align_up(o + sizeof(int) * F);
    L.total = o;
    return L;
}

}  // namespace

extern "C" {

int oppnpd_abi_version(void) { return OPPNPD_ABI_VERSION; }
const char* oppnpd_last_error(void) { return g_error; }

size_t oppnpd_workspace_bytes(int cap, int F, int trials) {
    if (!sizes_ok(cap, F) || trials < 1 || trials > OPPNPD_MAX_TRIALS || !hyps_ok(F, 4ll * trials)) return 0;
    return layout_of(cap, F, trials).total;
}

int oppnpd_ranges(const long long* b_ids, const int* count, int cap, int F, int* ranges, void* stream) {
    if (!sizes_ok(cap, F)) return bad_arg(__func__, "table sizes");
    if (!count || !ranges) return bad_arg(__func__, "null pointer");
    if (!b_ids && F != 1) return bad_arg(__func__, "b_ids = NULL means one frame");
    ranges_kernel<kThreads><<<blocks_of(F, kThreads), kThreads, 0, (hipStream_t)stream>>>(b_ids, count, cap, F, ranges);
    CAPI_CHECK_LAUNCH();
    return 0;
}

int oppnpd_prep(const float* pts2d, const float* pts3d, const int* count, int cap, const long long* b_ids, int F, const double* K, int k_shared,
                double scale, double* rows, void* stream) {
    if (!sizes_ok(cap, F)) return bad_arg(__func__, "table sizes");
    if (!pts2d || !pts3d || !count || !K || !rows) return bad_arg(__func__, "null pointer");
    if (!b_ids && F != 1) return bad_arg(__func__, "b_ids = NULL means one frame");
    if (!(isfinite(scale) && scale > 0.0)) return bad_arg(__func__, "scale: a finite number > 0");
    prep_kernel<<<blocks_of(cap, kThreads), kThreads, 0, (hipStream_t)stream>>>(pts2d, pts3d, count, cap, b_ids, F, K, k_shared, scale, rows);
    CAPI_CHECK_LAUNCH();
    return 0;
}

int oppnpd_sample(const int* ranges, int F, int trials, unsigned long long seed, int* samples, void* stream) {
    if (F < 1 || F > OPPNPD_MAX_FRAMES || trials < 1 || trials > OPPNPD_MAX_TRIALS || !hyps_ok(F, 4ll * trials)) return bad_arg(__func__, "table sizes");
    if (!ranges || !samples) return bad_arg(__func__, "null pointer");
    sample_kernel<<<dim3(blocks_of(trials, kThreads), F), kThreads, 0, (hipStream_t)stream>>>(ranges, OPPNPD_MAX_ROWS, F, trials, (uint64_t)seed, samples);
    CAPI_CHECK_LAUNCH();
    return 0;
}

int oppnpd_p3p(const double* rows, const int* ranges, const int* samples, int cap, int F, int trials, double* hyps, int* nsol, void* stream) {
    if (!sizes_ok(cap, F) || trials < 1 || trials > OPPNPD_MAX_TRIALS || !hyps_ok(F, 4ll * trials)) return bad_arg(__func__, "table sizes");
    if (!rows || !ranges || !samples || !hyps || !nsol) return bad_arg(__func__, "null pointer");
    p3p_kernel<<<dim3(blocks_of(trials, kThreads), F), kThreads, 0, (hipStream_t)stream>>>(rows, ranges, samples, cap, F, trials, hyps, nsol);
    CAPI_CHECK_LAUNCH();
    return 0;
}

int oppnpd_score(const double* rows, const int* ranges, const double* K, int k_shared, const double* hyps, int cap, int F, int H,
                 double reproj_err_px, int* cnt, double* cost, void* stream) {
    if (!sizes_ok(cap, F) || !hyps_ok(F, H)) return bad_arg(__func__, "table sizes");
    if (!rows || !ranges || !K || !hyps || !cnt || !cost) return bad_arg(__func__, "null pointer");
    if (!thr_ok(reproj_err_px)) return bad_arg(__func__, "reproj_err_px: a finite number > 0");
    score_kernel<<<dim3(blocks_of(H, kThreads), F), kThreads, 0, (hipStream_t)stream>>>(rows, ranges, K, k_shared, hyps, cap, F, H,
                                                                                      reproj_err_px * reproj_err_px, cnt, cost);
    CAPI_CHECK_LAUNCH();
    return 0;
}

int oppnpd_select(const int* cnt, const double* cost, const double* rows, const int* ranges, const int* count, const double* K, int k_shared,
                  const double* hyps, int cap, int F, int H, double reproj_err_px, double confidence, int trials, void* partial, int* best,
                  int* n_inliers, int* status, unsigned char* inlier_mask, void* stream) {
    if (!sizes_ok(cap, F) || !hyps_ok(F, H) || trials < 1 || trials > OPPNPD_MAX_TRIALS) return bad_arg(__func__, "table sizes");
    if (!cnt || !cost || !rows || !ranges || !count || !K || !hyps || !partial || !best || !n_inliers || !status || !inlier_mask)
        return bad_arg(__func__, "null pointer");
    if (!thr_ok(reproj_err_px)) return bad_arg(__func__, "reproj_err_px: a finite number > 0");
    if (!(confidence > 0.0 && confidence < 1.0)) return bad_arg(__func__, "confidence: in (0, 1)");
    const int nblk = (int)blocks_of(H, kSelBlock);
    hipStream_t S = (hipStream_t)stream;
    select_partial_kernel<<<dim3(nblk, F), kThreads, 0, S>>>(cnt, cost, F, H, nblk, (Best*)partial);
    CAPI_CHECK_LAUNCH();
    mask_clear_kernel<kThreads><<<blocks_of(cap, kThreads), kThreads, 0, S>>>(count, cap, inlier_mask);
    CAPI_CHECK_LAUNCH();
    select_final_kernel<<<F, kThreads, 0, S>>>((const Best*)partial, nblk, rows, ranges, K, k_shared, hyps, cap, F, H, reproj_err_px * reproj_err_px,
                                               confidence, trials, best, n_inliers, status, inlier_mask);
    CAPI_CHECK_LAUNCH();
    return 0;
}

int oppnpd_refine(const double* rows, const int* ranges, const double* K, int k_shared, const double* hyps, const int* best, int cap, int F, int H,
                  double reproj_err_px, double scale, double* pose, int* n_inliers, int* status, unsigned char* inlier_mask, void* stream) {
    if (!sizes_ok(cap, F) || !hyps_ok(F, H)) return bad_arg(__func__, "table sizes");
    if (!rows || !ranges || !K || !hyps || !best || !pose || !n_inliers || !status || !inlier_mask) return bad_arg(__func__, "null pointer");
    if (!thr_ok(reproj_err_px)) return bad_arg(__func__, "reproj_err_px: a finite number > 0");
    if (!(isfinite(scale) && scale > 0.0)) return bad_arg(__func__, "scale: a finite number > 0");
    refine_kernel<<<F, kThreads, 0, (hipStream_t)stream>>>(rows, ranges, K, k_shared, hyps, best, cap, F, H, reproj_err_px * reproj_err_px, scale, pose,
                                                           n_inliers, status, inlier_mask);
    CAPI_CHECK_LAUNCH();
    return 0;
}

int oppnpd_solve(const float* pts2d, const float* pts3d, const int* count, int cap, const long long* b_ids, int F, const double* K, int k_shared,
                 double scale, double reproj_err_px, double confidence, int trials, unsigned long long seed, void* workspace,
                 size_t workspace_bytes, double* pose, int* n_inliers, int* status, unsigned char* inlier_mask, void* stream) {
    // every argument before any launch
    if (!sizes_ok(cap, F) || trials < 1 || trials > OPPNPD_MAX_TRIALS || !hyps_ok(F, 4ll * trials)) return bad_arg(__func__, "table sizes");
    if (!pts2d || !pts3d || !count || !K || !workspace || !pose || !n_inliers || !status || !inlier_mask) return bad_arg(__func__, "null pointer");
    if (!b_ids && F != 1) return bad_arg(__func__, "b_ids = NULL means one frame");
    if (!(isfinite(scale) && scale > 0.0)) return bad_arg(__func__, "scale: a finite number > 0");
    if (!thr_ok(reproj_err_px)) return bad_arg(__func__, "reproj_err_px: a finite number > 0");
    if (!(confidence > 0.0 && confidence < 1.0)) return bad_arg(__func__, "confidence: in (0, 1)");
    const Layout L = layout_of(cap, F, trials);
    if (workspace_bytes < L.total) return bad_arg(__func__, "workspace too small (oppnpd_workspace_bytes)");
    char* ws = (char*)workspace;
    int* ranges = (int*)(ws + L.ranges);
    double* rows = (double*)(ws + L.rows);
    int* samples = (int*)(ws + L.samples);
    double* hyps = (double*)(ws + L.hyps);
    int* nsol = (int*)(ws + L.nsol);
    int* cnt = (int*)(ws + L.cnt);
    double* cost = (double*)(ws + L.cost);
    int* best = (int*)(ws + L.best);
    const int H = 4 * trials;
    int rc;
    if ((rc = oppnpd_ranges(b_ids, count, cap, F, ranges, stream)) != 0) return rc;
    if ((rc = oppnpd_prep(pts2d, pts3d, count, cap, b_ids, F, K, k_shared, scale, rows, stream)) != 0) return rc;
    if ((rc = oppnpd_sample(ranges, F, trials, seed, samples, stream)) != 0) return rc;
    if ((rc = oppnpd_p3p(rows, ranges, samples, cap, F, trials, hyps, nsol, stream)) != 0) return rc;
    if ((rc = oppnpd_score(rows, ranges, K, k_shared, hyps, cap, F, H, reproj_err_px, cnt, cost, stream)) != 0) return rc;
    if ((rc = oppnpd_select(cnt, cost, rows, ranges, count, K, k_shared, hyps, cap, F, H, reproj_err_px, confidence, trials, ws + L.partial, best,
                            n_inliers, status, inlier_mask, stream)) != 0) return rc;
    return oppnpd_refine(rows, ranges, K, k_shared, hyps, best, cap, F, H, reproj_err_px, scale, pose, n_inliers, status, inlier_mask, stream);
}

}  // extern "C"
