// Device detection (include/onepose_detect.h): the detector's vote from the LoFTR matcher's device-side matches
// without a host round trip.  The arithmetic is the host estimator's (csrc_host/pnp.cpp: affine_from3, affine_inliers and the normal
// equations of oppnp_estimate_affine2d), statement by statement in float64; what differs is the sampler (counter-based, so scheduling
// cannot change a draw) and that every trial runs.
//
//   ranges    ranges_kernel (device_loop.h, as the sampler and the crop geometry): one thread per view, two binary searches in b_ids
//   score     score_kernel: one workgroup per (view, 256 trials); a thread draws its trial's three rows, forms the affinity in registers
//             and walks the view's rows, staged through LDS in chunks of OPDET_SCORE_CHUNK (16 bytes a row) and read at a wave-uniform
//             address; the count is a per-thread integer
//   select    mask_clear_kernel, then select_kernel: one workgroup per view; (count descending, trial ascending) is a total order, so
//             the tree's shape cannot change the winner; the winner's affinity again from its sample, and its mask
//   fit, box  fit_box_kernel: one workgroup per view; twelve sums as per-thread partials in row order, added in thread order by twelve
//             threads; the 3 x 3 solve, the corners and the box on thread 0
//   vote      vote_kernel: one workgroup; the winner under (inliers descending, view ascending), its box and crop_geometry's pair
// No workgroup waits for another, every loop is bounded by a table size, no atomics: two runs agree bit for bit.  Compiled with
// contraction off: every expression is evaluated in the written order.
#include <hip/hip_runtime.h>
#include <math.h>
#include <stdint.h>
#include "onepose_detect.h"
#include "onepose_track.h"
#include "capi_error.h"
#include "device_loop.h"

using capi::bad_arg;
using capi::blocks_of;
using capi::g_error;
using devloop::align_up;
using devloop::block_best;
using devloop::draw3;
using devloop::fits_int32;
using devloop::geometry_entry;
using devloop::mask_clear_kernel;
using devloop::ranges_kernel;
using devloop::row_range;

#pragma clang fp contract(off)

namespace {

constexpr int kThreads = 256;                     // 4 waves of 64
constexpr int kChunk = OPDET_SCORE_CHUNK;
constexpr int kSums = 12;                         // xx, xy, x, yy, y, 1; xu, yu, u; xv, yv, v
static_assert(kChunk == kThreads, "a thread stages one row of a chunk");

__device__ __forceinline__ int trial_floor(int min_matches) { return min_matches > 3 ? min_matches : 3; }

// affine_from3 of the host estimator on rows r0, r1, r2 (indices into the row table, checked by the caller)
__device__ __forceinline__ bool affine_from3(const float* __restrict__ s, const float* __restrict__ d, int r0, int r1, int r2, double* A) {
    const double x0 = s[2 * (size_t)r0], y0 = s[2 * (size_t)r0 + 1], x1 = s[2 * (size_t)r1], y1 = s[2 * (size_t)r1 + 1];
    const double x2 = s[2 * (size_t)r2], y2 = s[2 * (size_t)r2 + 1];
    const double det = (x1 - x0) * (y2 - y0) - (x2 - x0) * (y1 - y0);
    const double scale = fabs(x1 - x0) + fabs(y1 - y0) + fabs(x2 - x0) + fabs(y2 - y0);
    if (!(fabs(det) > 1e-9 * scale * scale) || !(scale > 0.0)) return false;
#pragma unroll
    for (int r = 0; r < 2; ++r) {
        const double u0 = d[2 * (size_t)r0 + r], u1 = d[2 * (size_t)r1 + r], u2 = d[2 * (size_t)r2 + r];
        const double a = ((u1 - u0) * (y2 - y0) - (u2 - u0) * (y1 - y0)) / det;
        const double b = ((x1 - x0) * (u2 - u0) - (x2 - x0) * (u1 - u0)) / det;
        A[3 * r] = a; A[3 * r + 1] = b; A[3 * r + 2] = u0 - a * x0 - b * y0;
    }
    return true;
}

// affine_inliers' expression
__device__ __forceinline__ bool row_inlier(const double* A, double x, double y, double u, double v, double thr2) {
    const double ex = A[0] * x + A[1] * y + A[2] - u, ey = A[3] * x + A[4] * y + A[5] - v;
    return ex * ex + ey * ey < thr2;
}

// ---- sample, hypothesis, score -----------------------------------------------------------------------------------------------------------
__global__ __launch_bounds__(kThreads) void score_kernel(const float* __restrict__ mk0, const float* __restrict__ mk1, const int* __restrict__ ranges,
                                                         int cap, int V, int trials, int min_matches, double thr2, uint64_t seed,
                                                         int* __restrict__ samples, int* __restrict__ cnt_out) {
    __shared__ float4 sh[kChunk];
    const int t = blockIdx.x * kThreads + threadIdx.x, v = blockIdx.y;
    int begin, end;
    row_range(ranges, v, cap, begin, end);
    const int n = end - begin;
    const size_t slot = (size_t)v * trials + t;
    if (n < trial_floor(min_matches)) {           // the whole workgroup leaves: no trials in this view
        if (t < trials) {
            samples[3 * slot] = -1; samples[3 * slot + 1] = -1; samples[3 * slot + 2] = -1;
            cnt_out[slot] = 0;
        }
        return;
    }
    double A[6] = {0.0, 0.0, 0.0, 0.0, 0.0, 0.0};
    bool ok = false;
    if (t < trials) {
        int a, b, c;
        draw3(seed, v, t, n, a, b, c);
        samples[3 * slot] = a; samples[3 * slot + 1] = b; samples[3 * slot + 2] = c;
        ok = affine_from3(mk0, mk1, begin + a, begin + b, begin + c, A);
    }
    int cnt = 0;
    for (int c0 = begin; c0 < end; c0 += kChunk) {
        const int len = end - c0 < kChunk ? end - c0 : kChunk;
        __syncthreads();
        if ((int)threadIdx.x < len) {
            const size_t r = (size_t)(c0 + threadIdx.x);
            sh[threadIdx.x] = make_float4(mk0[2 * r], mk0[2 * r + 1], mk1[2 * r], mk1[2 * r + 1]);
        }
        __syncthreads();
        if (ok) {
            for (int j = 0; j < len; ++j) {
                const float4 p = sh[j];
                cnt += row_inlier(A, (double)p.x, (double)p.y, (double)p.z, (double)p.w, thr2) ? 1 : 0;
            }
        }
    }
    if (t < trials) cnt_out[slot] = cnt;
}

// ---- select ------------------------------------------------------------------------------------------------------------------------------
struct Best { int cnt; int idx; };                // idx < 0: no candidate

__device__ __forceinline__ bool better(const Best& a, const Best& b) {      // a before b in the total order
    if (a.idx < 0) return false;
    if (b.idx < 0) return true;
    if (a.cnt != b.cnt) return a.cnt > b.cnt;
    return a.idx < b.idx;
}

__global__ __launch_bounds__(kThreads) void select_kernel(const float* __restrict__ mk0, const float* __restrict__ mk1, const int* __restrict__ ranges,
                                                          const int* __restrict__ samples, const int* __restrict__ cnt, int cap, int V, int trials,
                                                          int min_matches, double thr2, double confidence, int* __restrict__ best,
                                                          int* __restrict__ n_inliers, int* __restrict__ status, unsigned char* __restrict__ mask) {
    __shared__ Best sh[kThreads];
    const int v = blockIdx.x;
    int begin, end;
    row_range(ranges, v, cap, begin, end);
    const int n = end - begin;
    const bool ran = n >= trial_floor(min_matches);
    Best mine{0, -1};
    if (ran) {
        for (int t = threadIdx.x; t < trials; t += kThreads) {    // ascending trials per thread
            const Best c{cnt[(size_t)v * trials + t], t};
            if (c.cnt > 0 && better(c, mine)) mine = c;
        }
    }
    const Best r = block_best<kThreads>(mine, sh);
    const int won = r.idx < 0 ? 0 : (r.cnt > n ? n : r.cnt);
    if (threadIdx.x == 0) {
        int st = (n < min_matches || won < 3) ? OPDET_STATUS_NO_MODEL : 0;
        if (ran) {                                                // the stop formula of oppnp_estimate_affine2d
            const double w = (double)won / (double)n, pw = w * w * w;
            bool more = true;
            if (pw > 1.0 - 1e-12) more = trials < 1;
            else if (pw > 1e-12) more = ceil(log(1.0 - confidence) / log(1.0 - pw)) > (double)trials;
            if (more) st |= OPDET_STATUS_NEEDS_MORE;
        }
        best[v] = r.idx;
        n_inliers[v] = won;
        status[v] = st;
    }
    if (r.idx < 0) return;                                        // (the mask was cleared before this launch)
    const int* s = samples + ((size_t)v * trials + r.idx) * 3;
    const int i0 = s[0], i1 = s[1], i2 = s[2];
    double A[6];
    bool ok = i0 >= 0 && i0 < n && i1 >= 0 && i1 < n && i2 >= 0 && i2 < n;
    ok = ok && affine_from3(mk0, mk1, begin + i0, begin + i1, begin + i2, A);
    if (!ok) return;
    for (int i = begin + threadIdx.x; i < end; i += kThreads)
        mask[i] = row_inlier(A, (double)mk0[2 * (size_t)i], (double)mk0[2 * (size_t)i + 1], (double)mk1[2 * (size_t)i], (double)mk1[2 * (size_t)i + 1], thr2) ? 1 : 0;
}

// ---- fit, box ----------------------------------------------------------------------------------------------------------------------------
__device__ __forceinline__ void centre_box(int H, int W, int* b) {
    b[0] = W / 2 - 500; b[1] = H / 2 - 500; b[2] = W / 2 + 500; b[3] = H / 2 + 500;
}

__global__ __launch_bounds__(kThreads) void fit_box_kernel(const float* __restrict__ mk0, const float* __restrict__ mk1, const int* __restrict__ ranges,
                                                           const int* __restrict__ view_hw, int cap, int V, int H, int W, int* __restrict__ n_inliers,
                                                           int* __restrict__ status, unsigned char* __restrict__ mask, double* __restrict__ affine,
                                                           int* __restrict__ boxes) {
    __shared__ double part[kSums][kThreads];
    __shared__ double sums[kSums];
    __shared__ int sh_model;
    const int v = blockIdx.x, tid = threadIdx.x;
    int begin, end;
    row_range(ranges, v, cap, begin, end);
    const int st_in = status[v];
    const bool model = !(st_in & OPDET_STATUS_NO_MODEL) && n_inliers[v] >= 3;
    double acc[kSums];
#pragma unroll
    for (int e = 0; e < kSums; ++e) acc[e] = 0.0;
    if (model) {
        for (int i = begin + tid; i < end; i += kThreads) {       // view-local rows tid, tid + 256, ...
            if (!mask[i]) continue;
            const double x = mk0[2 * (size_t)i], y = mk0[2 * (size_t)i + 1], u = mk1[2 * (size_t)i], w = mk1[2 * (size_t)i + 1];
            acc[0] += x * x; acc[1] += x * y; acc[2] += x * 1.0; acc[3] += y * y; acc[4] += y * 1.0; acc[5] += 1.0 * 1.0;
            acc[6] += x * u; acc[7] += y * u; acc[8] += 1.0 * u;
            acc[9] += x * w; acc[10] += y * w; acc[11] += 1.0 * w;
        }
    }
#pragma unroll
    for (int e = 0; e < kSums; ++e) part[e][tid] = acc[e];
    __syncthreads();
    if (tid < kSums) {                                            // the partials in thread order
        double s = 0.0;
        for (int l = 0; l < kThreads; ++l) s += part[tid][l];
        sums[tid] = s;
    }
    __syncthreads();
    if (tid == 0) {
        double A[6] = {1.0, 0.0, 0.0, 0.0, 1.0, 0.0};
        int b[4];
        bool ok = model;
        if (ok) {
            const double S[9] = {sums[0], sums[1], sums[2], sums[1], sums[3], sums[4], sums[2], sums[4], sums[5]};
            const double* bu = sums + 6;
            const double* bv = sums + 9;
            const double det = S[0] * (S[4] * S[8] - S[5] * S[7]) - S[1] * (S[3] * S[8] - S[5] * S[6]) + S[2] * (S[3] * S[7] - S[4] * S[6]);
            ok = !(fabs(det) < 1e-12);
            if (ok) {
                const double id = 1.0 / det;
                const double Si[9] = {(S[4] * S[8] - S[5] * S[7]) * id, (S[2] * S[7] - S[1] * S[8]) * id, (S[1] * S[5] - S[2] * S[4]) * id,
                                      (S[5] * S[6] - S[3] * S[8]) * id, (S[0] * S[8] - S[2] * S[6]) * id, (S[2] * S[3] - S[0] * S[5]) * id,
                                      (S[3] * S[7] - S[4] * S[6]) * id, (S[1] * S[6] - S[0] * S[7]) * id, (S[0] * S[4] - S[1] * S[3]) * id};
                double F[6];
#pragma unroll
                for (int a = 0; a < 3; ++a) {
                    F[a] = Si[a * 3] * bu[0] + Si[a * 3 + 1] * bu[1] + Si[a * 3 + 2] * bu[2];
                    F[3 + a] = Si[a * 3] * bv[0] + Si[a * 3 + 1] * bv[1] + Si[a * 3 + 2] * bv[2];
                }
                const double Hv = (double)view_hw[2 * v], Wv = (double)view_hw[2 * v + 1];
                const double cx[4] = {0.0, Wv, 0.0, Wv}, cy[4] = {0.0, 0.0, Hv, Hv};
                double px[4], py[4];
#pragma unroll
                for (int c = 0; c < 4; ++c) {
                    px[c] = F[0] * cx[c] + F[1] * cy[c] + F[2];
                    py[c] = F[3] * cx[c] + F[4] * cy[c] + F[5];
                    ok = ok && fits_int32(px[c]) && fits_int32(py[c]);
                }
                if (ok) {                                         // every coordinate fits, so the conversions are defined
                    int x0 = (int)px[0], y0 = (int)py[0], x1 = x0, y1 = y0;
#pragma unroll
                    for (int c = 1; c < 4; ++c) {
                        const int qx = (int)px[c], qy = (int)py[c];
                        x0 = qx < x0 ? qx : x0; x1 = qx > x1 ? qx : x1;
                        y0 = qy < y0 ? qy : y0; y1 = qy > y1 ? qy : y1;
                    }
                    b[0] = x0; b[1] = y0; b[2] = x1; b[3] = y1;
#pragma unroll
                    for (int e = 0; e < 6; ++e) A[e] = F[e];
                }
            }
        }
        if (!ok) {
            centre_box(H, W, b);
            n_inliers[v] = 0;
            status[v] = st_in | OPDET_STATUS_NO_MODEL;
        }
        for (int e = 0; e < 6; ++e) affine[(size_t)v * 6 + e] = A[e];
        for (int e = 0; e < 4; ++e) boxes[4 * v + e] = b[e];
        sh_model = ok ? 1 : 0;
    }
    __syncthreads();
    if (!sh_model)
        for (int i = begin + tid; i < end; i += kThreads) mask[i] = 0;
}

// ---- vote --------------------------------------------------------------------------------------------------------------------------------
__global__ __launch_bounds__(kThreads) void vote_kernel(const int* __restrict__ boxes, const int* __restrict__ n_inliers, int* __restrict__ status, int V,
                                                        int H, int W, const double* __restrict__ K, int S, int* __restrict__ winner,
                                                        int* __restrict__ box, int* __restrict__ flag, double* __restrict__ K_crop,
                                                        double* __restrict__ trans) {
    __shared__ Best sh[kThreads];
    __shared__ int sbox[4];
    const int tid = threadIdx.x;
    const Best mine = tid < V ? Best{n_inliers[tid], tid} : Best{0, -1};      // V <= OPDET_MAX_VIEWS = the workgroup's threads
    const Best r = block_best<kThreads>(mine, sh);
    if (tid == 0) {
        const int w = r.idx < 0 || r.idx >= V ? 0 : r.idx;
        int b[4] = {boxes[4 * w], boxes[4 * w + 1], boxes[4 * w + 2], boxes[4 * w + 3]};
        if (b[2] <= b[0] || b[3] <= b[1]) {
            centre_box(H, W, b);
            status[w] |= OPDET_STATUS_DEGENERATE;
        }
        *winner = w;
        for (int e = 0; e < 4; ++e) { sbox[e] = b[e]; box[e] = b[e]; }
        *flag = 0;
    }
    __syncthreads();
    if (tid < 9) geometry_entry(sbox, K, S, tid, K_crop, trans);
}

// ---- argument checks ---------------------------------------------------------------------------------------------------------------------
static_assert(OPDET_MAX_VIEWS <= kThreads, "the vote is one workgroup with a thread per view");

bool sizes_ok(int cap, int V) { return cap >= 1 && cap <= OPDET_MAX_ROWS && V >= 1 && V <= OPDET_MAX_VIEWS; }
bool trials_ok(int trials) { return trials >= 1 && trials <= OPDET_MAX_TRIALS; }
bool thr_ok(double e) { return isfinite(e) && e > 0.0; }
bool frame_ok(int H, int W) { return H >= 1 && H <= OPDET_MAX_SIDE && W >= 1 && W <= OPDET_MAX_SIDE; }

struct Layout { size_t ranges, samples, cnt, best, total; };

Layout layout_of(int V, int trials) {
    Layout L;
    size_t o = 0;
    L.ranges = o; o = align_up(o + sizeof(int) * 2 * V);
    L.samples = o; o = align_up(o + sizeof(int) * 3 * (size_t)V * trials);
    L.cnt = o; o = align_up(o + sizeof(int) * (size_t)V * trials);
    L.best = o; o = align_up(o + sizeof(int) * V);
    L.total = o;
    return L;
}

}  // namespace

extern "C" {

int opdet_abi_version(void) { return OPDET_ABI_VERSION; }
const char* opdet_last_error(void) { return g_error; }

size_t opdet_workspace_bytes(int cap, int V, int trials) {
    if (!sizes_ok(cap, V) || !trials_ok(trials)) return 0;
    return layout_of(V, trials).total;
}

int opdet_ranges(const long long* b_ids, const int* count, int cap, int V, int* ranges, void* stream) {
    if (!sizes_ok(cap, V)) return bad_arg(__func__, "table sizes");
    if (!b_ids || !ranges) return bad_arg(__func__, "null pointer");
    ranges_kernel<kThreads><<<blocks_of(V, kThreads), kThreads, 0, (hipStream_t)stream>>>(b_ids, count, cap, V, ranges);
    CAPI_CHECK_LAUNCH();
    return 0;
}

int opdet_score(const float* mk0, const float* mk1, const int* ranges, int cap, int V, int trials, int min_matches, double reproj_thr,
                unsigned long long seed, int* samples, int* cnt, void* stream) {
    if (!sizes_ok(cap, V)) return bad_arg(__func__, "table sizes");
    if (!trials_ok(trials)) return bad_arg(__func__, "trials outside [1, OPDET_MAX_TRIALS]");
    if (!mk0 || !mk1 || !ranges || !samples || !cnt) return bad_arg(__func__, "null pointer");
    if (min_matches < 0) return bad_arg(__func__, "min_matches < 0");
    if (!thr_ok(reproj_thr)) return bad_arg(__func__, "reproj_thr: a finite number > 0");
    score_kernel<<<dim3(blocks_of(trials, kThreads), V), kThreads, 0, (hipStream_t)stream>>>(mk0, mk1, ranges, cap, V, trials, min_matches,
                                                                                           reproj_thr * reproj_thr, (uint64_t)seed, samples, cnt);
    CAPI_CHECK_LAUNCH();
    return 0;
}

int opdet_select(const float* mk0, const float* mk1, const int* ranges, const int* count, const int* samples, const int* cnt, int cap, int V,
                 int trials, int min_matches, double reproj_thr, double confidence, int* best, int* n_inliers, int* status,
                 unsigned char* inlier_mask, void* stream) {
    if (!sizes_ok(cap, V)) return bad_arg(__func__, "table sizes");
    if (!trials_ok(trials)) return bad_arg(__func__, "trials outside [1, OPDET_MAX_TRIALS]");
    if (!mk0 || !mk1 || !ranges || !samples || !cnt || !best || !n_inliers || !status || !inlier_mask) return bad_arg(__func__, "null pointer");
    if (min_matches < 0) return bad_arg(__func__, "min_matches < 0");
    if (!thr_ok(reproj_thr)) return bad_arg(__func__, "reproj_thr: a finite number > 0");
    if (!(confidence > 0.0 && confidence < 1.0)) return bad_arg(__func__, "confidence: in (0, 1)");
    hipStream_t S = (hipStream_t)stream;
    mask_clear_kernel<kThreads><<<blocks_of(cap, kThreads), kThreads, 0, S>>>(count, cap, inlier_mask);
    CAPI_CHECK_LAUNCH();
    select_kernel<<<V, kThreads, 0, S>>>(mk0, mk1, ranges, samples, cnt, cap, V, trials, min_matches, reproj_thr * reproj_thr, confidence, best,
                                         n_inliers, status, inlier_mask);
    CAPI_CHECK_LAUNCH();
    return 0;
}

int opdet_fit_box(const float* mk0, const float* mk1, const int* ranges, const int* view_hw, int cap, int V, int H, int W, int* n_inliers,
                  int* status, unsigned char* inlier_mask, double* affine, int* boxes, void* stream) {
    if (!sizes_ok(cap, V)) return bad_arg(__func__, "table sizes");
    if (!frame_ok(H, W)) return bad_arg(__func__, "query size outside [1, OPDET_MAX_SIDE]");
    if (!mk0 || !mk1 || !ranges || !view_hw || !n_inliers || !status || !inlier_mask || !affine || !boxes) return bad_arg(__func__, "null pointer");
    fit_box_kernel<<<V, kThreads, 0, (hipStream_t)stream>>>(mk0, mk1, ranges, view_hw, cap, V, H, W, n_inliers, status, inlier_mask, affine, boxes);
    CAPI_CHECK_LAUNCH();
    return 0;
}

int opdet_vote(const int* boxes, const int* n_inliers, int* status, int V, int H, int W, const double* K, int S, int* winner, int* box,
               int* flag, double* K_crop, double* trans, void* stream) {
    if (V < 1 || V > OPDET_MAX_VIEWS) return bad_arg(__func__, "table sizes");
    if (!frame_ok(H, W)) return bad_arg(__func__, "query size outside [1, OPDET_MAX_SIDE]");
    if (S < 1 || S > OPTRK_MAX_CROP) return bad_arg(__func__, "crop size S outside [1, OPTRK_MAX_CROP]");
    if (!boxes || !n_inliers || !status || !K || !winner || !box || !flag || !K_crop || !trans) return bad_arg(__func__, "null pointer");
    vote_kernel<<<1, kThreads, 0, (hipStream_t)stream>>>(boxes, n_inliers, status, V, H, W, K, S, winner, box, flag, K_crop, trans);
    CAPI_CHECK_LAUNCH();
    return 0;
}

int opdet_detect(const float* mk0, const float* mk1, const long long* b_ids, const int* count, int cap, int V, const int* view_hw, int H, int W,
                 const double* K, int S, int min_matches, double reproj_thr, double confidence, int trials, unsigned long long seed,
                 void* workspace, size_t workspace_bytes, int* boxes, int* n_inliers, double* affine, int* status, unsigned char* inlier_mask,
                 int* winner, int* box, int* flag, double* K_crop, double* trans, void* stream) {
    // every argument before any launch
    if (!sizes_ok(cap, V)) return bad_arg(__func__, "table sizes");
    if (!trials_ok(trials)) return bad_arg(__func__, "trials outside [1, OPDET_MAX_TRIALS]");
    if (!frame_ok(H, W)) return bad_arg(__func__, "query size outside [1, OPDET_MAX_SIDE]");
    if (S < 1 || S > OPTRK_MAX_CROP) return bad_arg(__func__, "crop size S outside [1, OPTRK_MAX_CROP]");
    if (!mk0 || !mk1 || !b_ids || !view_hw || !K || !workspace || !boxes || !n_inliers || !affine || !status || !inlier_mask || !winner || !box ||
        !flag || !K_crop || !trans)
        return bad_arg(__func__, "null pointer");
    if (min_matches < 0) return bad_arg(__func__, "min_matches < 0");
    if (!thr_ok(reproj_thr)) return bad_arg(__func__, "reproj_thr: a finite number > 0");
    if (!(confidence > 0.0 && confidence < 1.0)) return bad_arg(__func__, "confidence: in (0, 1)");
    const Layout L = layout_of(V, trials);
    if (workspace_bytes < L.total) return bad_arg(__func__, "workspace too small (opdet_workspace_bytes)");
    char* ws = (char*)workspace;
    int* ranges = (int*)(ws + L.ranges);
    int* samples = (int*)(ws + L.samples);
    int* cnt = (int*)(ws + L.cnt);
    int* best = (int*)(ws + L.best);
    int rc;
    if ((rc = opdet_ranges(b_ids, count, cap, V, ranges, stream)) != 0) return rc;
    if ((rc = opdet_score(mk0, mk1, ranges, cap, V, trials, min_matches, reproj_thr, seed, samples, cnt, stream)) != 0) return rc;
    if ((rc = opdet_select(mk0, mk1, ranges, count, samples, cnt, cap, V, trials, min_matches, reproj_thr, confidence, best, n_inliers, status,
                           inlier_mask, stream)) != 0) return rc;
    if ((rc = opdet_fit_box(mk0, mk1, ranges, view_hw, cap, V, H, W, n_inliers, status, inlier_mask, affine, boxes, stream)) != 0) return rc;
    return opdet_vote(boxes, n_inliers, status, V, H, W, K, S, winner, box, flag, K_crop, trans, stream);
}

}  // extern "C"
