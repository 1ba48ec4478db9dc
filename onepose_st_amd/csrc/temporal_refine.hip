// The temporal pose refinement (include/onepose_temporal.h): the float32 image pyramid, the pyramidal translation-only
// Lucas-Kanade tracker with its forward-backward check, and the two table kernels (collect, inject) around it.  The header is the
// specification; everything per point is float64 in the written order.
//
// pyr_down_kernel   one launch per level: a workgroup loads the (2 * 16 + 4) x (2 * 64 + 4) neighbourhood of its 16 x 64 outputs into LDS
//                   (indices clamped: the replicated border), runs the vertical pass on the kept rows into a second LDS tile and the
//                   horizontal pass on the kept columns out of it.  The level above is read once (halo aside), this level written once.
// track_kernel      256 threads, one wave per point.  Lane l owns the window elements l, l + 64, ...: at most 16 at window 31, their
//                   template and both gradients stay in registers over all iterations of a level.  The target is sampled straight from
//                   the float32 pyramid in global memory (a 31 x 31 neighbourhood moves with d, and its 4 KB sit in L1/L2 after the first
//                   iteration; no LDS staging).  The sums go through the xor butterfly of postopt_step_kernel, after which every lane holds
//                   the same number, so the whole level / iteration / forward-backward control flow is wave-uniform.
// collect_kernel,   one workgroup each: rows in chunks of 256, ballot + prefix inside the chunk, a running base across chunks: the
// inject_source_    position of a row never depends on timing.  inject is one launch for the frame's own rows and one per source, each
// kernel            starting at the count the launch before it left.  No atomics anywhere in this file.
#include "capi_error.h"
#include "device_loop.h"
#include "reduce_f64.h"
#include "onepose_temporal.h"
#include <math.h>
#include <stdint.h>

#pragma clang fp contract(off)

namespace {

using capi::bad_arg;
using capi::blocks_of;
using capi::fail;
using capi::g_error;
using devloop::clamped_count;
using red64::uniform;
using red64::wave_sum;

constexpr int kThreads = 256;
constexpr int kTileW = 64, kTileH = 16;                             // outputs of one pyr_down workgroup
constexpr int kInW = 2 * kTileW + 4, kInH = 2 * kTileH + 4;         // their inputs, with the two-element halo
constexpr int kPerLane = (OPTMP_MAX_WINDOW * OPTMP_MAX_WINDOW + 63) / 64;   // 16

// ---- the pyramid's layout (header, entry 1): the same function on both sides ---------------------------------------------------------------
__host__ __device__ __forceinline__ void level_geometry(int H, int W, int l, int& h, int& w, long long& off_floats) {
    h = H; w = W; off_floats = 0;
    for (int i = 0; i < l; ++i) {
        off_floats += ((long long)h * w + 63) & ~63LL;              // 256 bytes = 64 floats
        h = (h + 1) >> 1; w = (w + 1) >> 1;
    }
}

size_t pyramid_total(int H, int W, int levels) {
    if (levels < 1 || levels > OPTMP_MAX_LEVELS || H < 2 || W < 2 || H > OPTMP_MAX_SIDE || W > OPTMP_MAX_SIDE) return 0;
    int h, w; long long off;
    level_geometry(H, W, levels - 1, h, w, off);
    if (h < 2 || w < 2) return 0;
    level_geometry(H, W, levels, h, w, off);
    return (size_t)off * 4;
}

// four pixels per thread: one 4-byte load and one 16-byte store where the frame pointer allows it (Aligned), bytes otherwise and at the tail
template <bool Aligned>
__global__ __launch_bounds__(kThreads) void pyr_level0_kernel(const unsigned char* __restrict__ frame, long long n, float* __restrict__ out) {
    const long long i = ((long long)blockIdx.x * kThreads + threadIdx.x) * 4;
    if (Aligned && i + 3 < n) {
        const uchar4 v = *reinterpret_cast<const uchar4*>(frame + i);
        *reinterpret_cast<float4*>(out + i) = make_float4((float)v.x, (float)v.y, (float)v.z, (float)v.w);
        return;
    }
    for (long long k = i; k < i + 4 && k < n; ++k) out[k] = (float)frame[k];
}

__device__ __forceinline__ float tap5(float a0, float a1, float a2, float a3, float a4) {
    return (((a0 + a4) + 4.0f * (a1 + a3)) + 6.0f * a2) * 0.0625f;
}

__global__ __launch_bounds__(kThreads) void pyr_down_kernel(const float* __restrict__ in, int h, int w, float* __restrict__ out, int oh, int ow) {
    __shared__ float tin[kInH][kInW + 1];
    __shared__ float tv[kTileH][kInW + 1];
    const int tid = threadIdx.x, ox0 = blockIdx.x * kTileW, oy0 = blockIdx.y * kTileH;
    for (int i = tid; i < kInH * kInW; i += kThreads) {
        const int r = i / kInW, c = i - r * kInW;
        int y = 2 * oy0 + r - 2, x = 2 * ox0 + c - 2;
        y = y < 0 ? 0 : (y > h - 1 ? h - 1 : y);
        x = x < 0 ? 0 : (x > w - 1 ? w - 1 : x);
        tin[r][c] = in[(long long)y * w + x];
    }
    __syncthreads();
    for (int i = tid; i < kTileH * kInW; i += kThreads) {           // the vertical pass at the kept rows 2 (oy0 + r)
        const int r = i / kInW, c = i - r * kInW;
        tv[r][c] = tap5(tin[2 * r][c], tin[2 * r + 1][c], tin[2 * r + 2][c], tin[2 * r + 3][c], tin[2 * r + 4][c]);
    }
    __syncthreads();
    for (int i = tid; i < kTileH * kTileW; i += kThreads) {         // the horizontal pass at the kept columns 2 (ox0 + c)
        const int r = i / kTileW, c = i - r * kTileW;
        const int oy = oy0 + r, ox = ox0 + c;
        if (oy < oh && ox < ow)
            out[(long long)oy * ow + ox] = tap5(tv[r][2 * c], tv[r][2 * c + 1], tv[r][2 * c + 2], tv[r][2 * c + 3], tv[r][2 * c + 4]);
    }
}

// ---- the tracker ----------------------------------------------------------------------------------------------------------------------------
struct TrackArgs {
    const float *src, *dst;
    const double *pts, *guess, *pose, *K;
    const float* pts_3d;
    const int* count;
    double *out_pts, *fb_error;
    int *flags, *iterations;
    double scale, eps2, min_eig, fb_threshold;
    int cap, H, W, levels, window, max_iters;
};

__device__ __forceinline__ double quiet_nan() { return __longlong_as_double(0x7ff8000000000000LL); }

__device__ __forceinline__ bool finite2(double x, double y) { return fabs(x) < HUGE_VAL && fabs(y) < HUGE_VAL; }   // false for NaN

__device__ __forceinline__ bool inside(double x, double y, int W, int H) {                                          // false for NaN
    return x >= 0.0 && x <= (double)(W - 1) && y >= 0.0 && y <= (double)(H - 1);
}

// a float64 index into [0, hi]; NaN -> 0; never converts a value outside the int range
__device__ __forceinline__ int clamp_index(double v, int hi) { return !(v >= 0.0) ? 0 : (v > (double)hi ? hi : (int)v); }

__device__ __forceinline__ double sample(const float* __restrict__ I, int w, int h, double x, double y) {
    const double x0 = floor(x), y0 = floor(y);
    const double fx = x - x0, fy = y - y0;
    const int xa = clamp_index(x0, w - 1), xb = clamp_index(x0 + 1.0, w - 1);
    const int ya = clamp_index(y0, h - 1), yb = clamp_index(y0 + 1.0, h - 1);
    const double a = (double)I[ya * w + xa], b = (double)I[ya * w + xb], c = (double)I[yb * w + xa], d = (double)I[yb * w + xb];
    const double top = a + fx * (b - a), bot = c + fx * (d - c);
    return top + fy * (bot - top);
}

// track(S, D, p, g) of the header; every lane of the wave calls it with the same arguments and returns the same values
__device__ __forceinline__ int track_point(const TrackArgs& a, const float* __restrict__ S, const float* __restrict__ D, double px, double py,
                                           double gx0, double gy0, int lane, double& qx, double& qy, int& iters) {
    qx = qy = quiet_nan();
    iters = 0;
    if (!finite2(px, py) || !finite2(gx0, gy0) || !inside(px, py, a.W, a.H)) return OPTMP_BAD_INPUT;
    const int window = a.window, half = window >> 1, n_el = window * window;
    const double top = (double)(1 << (a.levels - 1));
    double dx = (gx0 - px) / top, dy = (gy0 - py) / top;
    int flags = 0;
    int offs[kPerLane];                                             // this lane's window offsets, (oy + half) << 8 | (ox + half)
#pragma unroll
    for (int j = 0; j < kPerLane; ++j) {
        const int k = lane + 64 * j, r = k / window;
        offs[j] = (r << 8) | (k - r * window);
    }
    for (int l = a.levels - 1; l >= 0; --l) {
        int h, w; long long off;
        level_geometry(a.H, a.W, l, h, w, off);
        const float* __restrict__ Sl = S + off;
        const float* __restrict__ Dl = D + off;
        const double s = (double)(1 << l);
        const double plx = px / s, ply = py / s;
        double T[kPerLane], Gx[kPerLane], Gy[kPerLane];
        double sxx = 0.0, sxy = 0.0, syy = 0.0;
#pragma unroll
        for (int j = 0; j < kPerLane; ++j) {
            const int k = lane + 64 * j;
            T[j] = Gx[j] = Gy[j] = 0.0;
            if (k < n_el) {
                const double x = plx + (double)((offs[j] & 255) - half), y = ply + (double)((offs[j] >> 8) - half);
                T[j] = sample(Sl, w, h, x, y);
                Gx[j] = 0.5 * (sample(Sl, w, h, x + 1.0, y) - sample(Sl, w, h, x - 1.0, y));
                Gy[j] = 0.5 * (sample(Sl, w, h, x, y + 1.0) - sample(Sl, w, h, x, y - 1.0));
                sxx += Gx[j] * Gx[j];
                sxy += Gx[j] * Gy[j];
                syy += Gy[j] * Gy[j];
            }
        }
        const double Gxx = uniform(wave_sum(sxx)), Gxy = uniform(wave_sum(sxy)), Gyy = uniform(wave_sum(syy));
        const double det = Gxx * Gyy - Gxy * Gxy;
        const double min_eig = ((Gxx + Gyy) - sqrt((Gxx - Gyy) * (Gxx - Gyy) + 4.0 * (Gxy * Gxy))) / (2.0 * (double)n_el);
        if (!(det > 0.0) || !(min_eig >= a.min_eig)) return flags | OPTMP_DEGENERATE;
        bool converged = false;
        for (int it = 0; it < a.max_iters; ++it) {
            const double cx = plx + dx, cy = ply + dy;
            double bx = 0.0, by = 0.0;
#pragma unroll
            for (int j = 0; j < kPerLane; ++j) {
                const int k = lane + 64 * j;
                if (k < n_el) {
                    const double e = T[j] - sample(Dl, w, h, cx + (double)((offs[j] & 255) - half), cy + (double)((offs[j] >> 8) - half));
                    bx += e * Gx[j];
                    by += e * Gy[j];
                }
            }
            bx = uniform(wave_sum(bx));
            by = uniform(wave_sum(by));
            const double ddx = (Gyy * bx - Gxy * by) / det, ddy = (Gxx * by - Gxy * bx) / det;
            dx = dx + ddx;
            dy = dy + ddy;
            ++iters;
            if (ddx * ddx + ddy * ddy < a.eps2) { converged = true; break; }
        }
        if (l == 0 && !converged) flags |= OPTMP_FLAG_MAX_ITERS;
        if (!inside(px + s * dx, py + s * dy, a.W, a.H)) return flags | OPTMP_OUT_OF_IMAGE;
        if (l > 0) { dx = 2.0 * dx; dy = 2.0 * dy; }
    }
    qx = px + dx;
    qy = py + dy;
    return flags;
}

__global__ __launch_bounds__(kThreads) void track_kernel(TrackArgs a) {
    const int lane = threadIdx.x & 63;
    const int row = __builtin_amdgcn_readfirstlane((int)(blockIdx.x * (kThreads / 64) + (threadIdx.x >> 6)));
    if (row >= clamped_count(a.count, a.cap)) return;
    const double px = a.pts[2 * row], py = a.pts[2 * row + 1];
    double gx = px, gy = py;
    if (a.guess) { gx = a.guess[2 * row]; gy = a.guess[2 * row + 1]; }
    if (a.pts_3d) {
        const double X0 = a.scale * (double)a.pts_3d[3 * row], X1 = a.scale * (double)a.pts_3d[3 * row + 1], X2 = a.scale * (double)a.pts_3d[3 * row + 2];
        double cam[3], u[3];
        for (int i = 0; i < 3; ++i) cam[i] = ((a.pose[4 * i] * X0 + a.pose[4 * i + 1] * X1) + a.pose[4 * i + 2] * X2) + a.scale * a.pose[4 * i + 3];
        for (int i = 0; i < 3; ++i) u[i] = (a.K[3 * i] * cam[0] + a.K[3 * i + 1] * cam[1]) + a.K[3 * i + 2] * cam[2];
        const double ux = u[0] / u[2], uy = u[1] / u[2];
        if (cam[2] > 1e-12 && finite2(ux, uy) && inside(ux, uy, a.W, a.H)) { gx = ux; gy = uy; }
    }
    double qx, qy, fbe = quiet_nan();
    int iters;
    int flags = track_point(a, a.src, a.dst, px, py, gx, gy, lane, qx, qy, iters);
    if (!(flags & OPTMP_LOST) && a.fb_threshold >= 0.0) {
        double bx, by;
        int back_iters;
        const int back = track_point(a, a.dst, a.src, qx, qy, qx - (gx - px), qy - (gy - py), lane, bx, by, back_iters);
        if (back & OPTMP_LOST) {
            flags |= OPTMP_FB_FAIL;
        } else {
            const double ex = bx - px, ey = by - py;
            fbe = sqrt(ex * ex + ey * ey);
            if (!(fbe <= a.fb_threshold)) flags |= OPTMP_FB_FAIL;
        }
    }
    if (lane == 0) {
        a.out_pts[2 * row] = qx;
        a.out_pts[2 * row + 1] = qy;
        a.flags[row] = flags;
        a.iterations[row] = iters;
        a.fb_error[row] = fbe;
    }
}

// ---- collect and inject -------------------------------------------------------------------------------------------------------------------
// the position of the calling thread's row among the selected rows of this chunk of 256, and the chunk's total; wsum: 4 ints of LDS
__device__ __forceinline__ int chunk_position(bool selected, int* wsum, int& total) {
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const unsigned long long m = __ballot(selected);
    __syncthreads();                                                // the previous chunk's readers are done with wsum
    if (lane == 0) wsum[wave] = __popcll(m);
    __syncthreads();
    int before = 0;
    for (int v = 0; v < wave; ++v) before += wsum[v];
    total = (wsum[0] + wsum[1]) + (wsum[2] + wsum[3]);
    return before + __popcll(m & ((1ull << lane) - 1ull));
}

__global__ __launch_bounds__(kThreads) void collect_kernel(const float* __restrict__ pts_2d, const float* __restrict__ pts_3d,
                                                           const int* __restrict__ count, int cap, const unsigned char* __restrict__ mask,
                                                           const double* __restrict__ trans, double* __restrict__ pts_orig,
                                                           float* __restrict__ out_3d, int* __restrict__ out_count) {
    __shared__ int wsum[kThreads / 64];
    const int n = clamped_count(count, cap);
    const double m00 = trans[0], m01 = trans[1], m02 = trans[2], m10 = trans[3], m11 = trans[4], m12 = trans[5], m20 = trans[6], m21 = trans[7],
                 m22 = trans[8];
    const double c0 = m11 * m22 - m12 * m21, c1 = m12 * m20 - m10 * m22, c2 = m10 * m21 - m11 * m20;
    const double det = (m00 * c0 + m01 * c1) + m02 * c2;
    const double n00 = c0 / det, n01 = (m02 * m21 - m01 * m22) / det, n02 = (m01 * m12 - m02 * m11) / det;
    const double n10 = c1 / det, n11 = (m00 * m22 - m02 * m20) / det, n12 = (m02 * m10 - m00 * m12) / det;
    const double n20 = c2 / det, n21 = (m01 * m20 - m00 * m21) / det, n22 = (m00 * m11 - m01 * m10) / det;
    int base = 0;
    for (int r0 = 0; r0 < cap; r0 += kThreads) {                    // sized by the capacity: the trip count is the same for every thread
        const int row = r0 + (int)threadIdx.x;
        const bool sel = row < n && (!mask || mask[row] != 0);
        int total;
        const int pos = base + chunk_position(sel, wsum, total);
        if (sel) {
            const double x = (double)pts_2d[2 * row], y = (double)pts_2d[2 * row + 1];
            const double h0 = (n00 * x + n01 * y) + n02, h1 = (n10 * x + n11 * y) + n12, h2 = (n20 * x + n21 * y) + n22;
            pts_orig[2 * pos] = h0 / h2;
            pts_orig[2 * pos + 1] = h1 / h2;
            out_3d[3 * pos] = pts_3d[3 * row]; out_3d[3 * pos + 1] = pts_3d[3 * row + 1]; out_3d[3 * pos + 2] = pts_3d[3 * row + 2];
        }
        base += total;
    }
    if (threadIdx.x == 0) *out_count = base;
}

// rows [0, own) of the injected table and the count behind them
__global__ __launch_bounds__(kThreads) void inject_own_kernel(const float* __restrict__ own_2d, const float* __restrict__ own_3d,
                                                              const int* __restrict__ own_count, int cap_own, float* __restrict__ out_2d,
                                                              float* __restrict__ out_3d, int* __restrict__ out_count) {
    const int own = clamped_count(own_count, cap_own);
    for (int row = blockIdx.x * kThreads + threadIdx.x; row < own; row += gridDim.x * kThreads) {
        out_2d[2 * row] = own_2d[2 * row]; out_2d[2 * row + 1] = own_2d[2 * row + 1];
        out_3d[3 * row] = own_3d[3 * row]; out_3d[3 * row + 1] = own_3d[3 * row + 1]; out_3d[3 * row + 2] = own_3d[3 * row + 2];
    }
    if (blockIdx.x == 0 && threadIdx.x == 0) *out_count = own;
}

// one source's unflagged rows behind the count the launch before this one left (the same stream orders them); one workgroup
__global__ __launch_bounds__(kThreads) void inject_source_kernel(const double* __restrict__ pts, const float* __restrict__ p3,
                                                                 const int* __restrict__ flags, const int* __restrict__ count, int cap,
                                                                 const double* __restrict__ trans, float* __restrict__ out_2d,
                                                                 float* __restrict__ out_3d, int* out_count, int cap_total) {
    __shared__ int wsum[kThreads / 64];
    double m[9];
    for (int i = 0; i < 9; ++i) m[i] = trans[i];
    const int n = clamped_count(count, cap);
    int base = clamped_count(out_count, cap_total);
    for (int r0 = 0; r0 < cap; r0 += kThreads) {                    // sized by the capacity: the trip count is the same for every thread
        const int row = r0 + (int)threadIdx.x;
        const bool sel = row < n && !(flags[row] & OPTMP_LOST);
        int total;
        const int pos = base + chunk_position(sel, wsum, total);
        if (sel && pos < cap_total) {
            const double x = pts[2 * row], y = pts[2 * row + 1];
            const double h0 = (m[0] * x + m[1] * y) + m[2], h1 = (m[3] * x + m[4] * y) + m[5], h2 = (m[6] * x + m[7] * y) + m[8];
            out_2d[2 * pos] = (float)(h0 / h2);
            out_2d[2 * pos + 1] = (float)(h1 / h2);
            out_3d[3 * pos] = p3[3 * row]; out_3d[3 * pos + 1] = p3[3 * row + 1]; out_3d[3 * pos + 2] = p3[3 * row + 2];
        }
        base += total;
    }
    __syncthreads();                                                // every thread has read the old count
    if (threadIdx.x == 0) *out_count = base < cap_total ? base : cap_total;
}

bool finite_host(double v) { return v - v == 0.0; }

}  // namespace

extern "C" {

int optmp_abi_version(void) { return OPTMP_ABI_VERSION; }

const char* optmp_last_error(void) { return g_error; }

size_t optmp_pyramid_bytes(int H, int W, int levels) { return pyramid_total(H, W, levels); }

int optmp_pyramid(const unsigned char* frame, int H, int W, int levels, void* pyramid, size_t pyramid_bytes, void* stream) {
    if (!frame || !pyramid) return bad_arg(__func__, "null pointer");
    const size_t need = pyramid_total(H, W, levels);
    if (need == 0) return bad_arg(__func__, "levels in [1, 6], H and W in [2, 16384], the smallest level at least 2 x 2");
    if (pyramid_bytes < need) return bad_arg(__func__, "pyramid too small (optmp_pyramid_bytes)");
    if ((uintptr_t)pyramid & 255) return bad_arg(__func__, "pyramid 256-byte aligned");
    hipStream_t s = (hipStream_t)stream;
    float* base = static_cast<float*>(pyramid);
    const long long n0 = (long long)H * W;
    if ((uintptr_t)frame & 3)
        pyr_level0_kernel<false><<<blocks_of(n0, 4 * kThreads), kThreads, 0, s>>>(frame, n0, base);
    else
        pyr_level0_kernel<true><<<blocks_of(n0, 4 * kThreads), kThreads, 0, s>>>(frame, n0, base);
    CAPI_CHECK_LAUNCH();
    for (int l = 1; l < levels; ++l) {
        int h, w, oh, ow; long long off, ooff;
        level_geometry(H, W, l - 1, h, w, off);
        level_geometry(H, W, l, oh, ow, ooff);
        pyr_down_kernel<<<dim3(blocks_of(ow, kTileW), blocks_of(oh, kTileH)), kThreads, 0, s>>>(base + off, h, w, base + ooff, oh, ow);
        CAPI_CHECK_LAUNCH();
    }
    return 0;
}

int optmp_track(const void* src, const void* dst, int H, int W, int levels, const double* pts, const int* count, int cap,
                const double* guess, const float* pts_3d, const double* pose, const double* K, double scale, int window, int max_iters,
                double eps, double min_eig_threshold, double fb_threshold, double* out_pts, int* flags, int* iterations, double* fb_error,
                void* stream) {
    if (!src || !dst || !pts || !out_pts || !flags || !iterations || !fb_error) return bad_arg(__func__, "null pointer");
    if (pyramid_total(H, W, levels) == 0) return bad_arg(__func__, "levels in [1, 6], H and W in [2, 16384], the smallest level at least 2 x 2");
    if (cap < 1 || cap > OPTMP_MAX_ROWS) return bad_arg(__func__, "cap outside [1, 2^20]");
    if (window < OPTMP_MIN_WINDOW || window > OPTMP_MAX_WINDOW || !(window & 1)) return bad_arg(__func__, "window: odd, in [3, 31]");
    if (max_iters < 1 || max_iters > OPTMP_MAX_ITERS) return bad_arg(__func__, "max_iters outside [1, 1000]");
    if (!(eps > 0.0 && finite_host(eps) && min_eig_threshold >= 0.0 && finite_host(min_eig_threshold)) || fb_threshold != fb_threshold)
        return bad_arg(__func__, "eps > 0, min_eig_threshold >= 0, both finite; fb_threshold a number (negative: no check)");
    if ((pts_3d != nullptr) != (pose != nullptr) || (pts_3d != nullptr) != (K != nullptr))
        return bad_arg(__func__, "pts_3d, pose and K: all three or none");
    if (!(scale > 0.0 && finite_host(scale))) return bad_arg(__func__, "scale: a finite number > 0");
    if (((uintptr_t)src & 255) || ((uintptr_t)dst & 255)) return bad_arg(__func__, "pyramids 256-byte aligned");
    TrackArgs a{};
    a.src = static_cast<const float*>(src);
    a.dst = static_cast<const float*>(dst);
    a.pts = pts; a.guess = guess; a.pose = pose; a.K = K; a.pts_3d = pts_3d; a.count = count;
    a.out_pts = out_pts; a.fb_error = fb_error; a.flags = flags; a.iterations = iterations;
    a.scale = scale; a.eps2 = eps * eps; a.min_eig = min_eig_threshold; a.fb_threshold = fb_threshold;
    a.cap = cap; a.H = H; a.W = W; a.levels = levels; a.window = window; a.max_iters = max_iters;
    track_kernel<<<blocks_of(cap, kThreads / 64), kThreads, 0, (hipStream_t)stream>>>(a);
    CAPI_CHECK_LAUNCH();
    return 0;
}

int optmp_collect(const float* pts_2d, const float* pts_3d, const int* count, int cap, const unsigned char* mask, const double* trans,
                  double* pts_orig, float* out_3d, int* out_count, void* stream) {
    if (!pts_2d || !pts_3d || !trans || !pts_orig || !out_3d || !out_count) return bad_arg(__func__, "null pointer");
    if (cap < 1 || cap > OPTMP_MAX_ROWS) return bad_arg(__func__, "cap outside [1, 2^20]");
    collect_kernel<<<1, kThreads, 0, (hipStream_t)stream>>>(pts_2d, pts_3d, count, cap, mask, trans, pts_orig, out_3d, out_count);
    CAPI_CHECK_LAUNCH();
    return 0;
}

int optmp_inject(const float* own_2d, const float* own_3d, const int* own_count, int cap_own, const void** src_pts, const void** src_3d,
                 const void** src_flags, const void** src_count, const int* src_cap, int n_sources, const double* trans, float* out_2d,
                 float* out_3d, int* out_count, int cap_total, void* stream) {
    if (!own_2d || !own_3d || !trans || !out_2d || !out_3d || !out_count) return bad_arg(__func__, "null pointer");
    if (n_sources < 0 || n_sources > OPTMP_MAX_SOURCES) return bad_arg(__func__, "n_sources outside [0, 8]");
    if (n_sources > 0 && (!src_pts || !src_3d || !src_flags || !src_count || !src_cap)) return bad_arg(__func__, "null source table");
    if (cap_own < 1 || cap_own > OPTMP_MAX_ROWS || cap_total < cap_own || cap_total > OPTMP_MAX_ROWS)
        return bad_arg(__func__, "1 <= cap_own <= cap_total <= 2^20");
    for (int s = 0; s < n_sources; ++s) {
        if (!src_pts[s] || !src_3d[s] || !src_flags[s]) return bad_arg(__func__, "null pointer in a source");
        if (src_cap[s] < 1 || src_cap[s] > OPTMP_MAX_ROWS) return bad_arg(__func__, "source capacity outside [1, 2^20]");
    }
    hipStream_t st = (hipStream_t)stream;
    const unsigned own_blocks = blocks_of(cap_own, kThreads);
    inject_own_kernel<<<own_blocks < 64 ? own_blocks : 64, kThreads, 0, st>>>(own_2d, own_3d, own_count, cap_own, out_2d, out_3d, out_count);
    CAPI_CHECK_LAUNCH();
    for (int s = 0; s < n_sources; ++s) {
        inject_source_kernel<<<1, kThreads, 0, st>>>(static_cast<const double*>(src_pts[s]), static_cast<const float*>(src_3d[s]),
                                                     static_cast<const int*>(src_flags[s]), static_cast<const int*>(src_count[s]), src_cap[s],
                                                     trans, out_2d, out_3d, out_count, cap_total);
        CAPI_CHECK_LAUNCH();
    }
    return 0;
}

}  // extern "C"
