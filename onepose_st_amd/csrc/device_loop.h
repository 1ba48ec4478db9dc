// What several satellite libraries must compute alike, written once.  It began as the shared code of the device frame loop
// (pnp_device.hip, track_box.hip, detect_affine.hip), whose specification asks for bit-identical behaviour in three places; this header
// is the single copy of each, and other libraries take from it what they would otherwise restate (temporal_refine.hip: clamped_count;
// sfm_triangulate.hip: mix64):
//
//   the sampler        onepose_detect.h defines detection's draws as onepose_pnp_device.h's with the view in place of the frame: mix64, draw3
//   the crop geometry  the state detection writes is bit-equal to optrk_box_set's (onepose_track.h, crop_geometry): geometry_entry, fits_int32
//   the range rule     a group's rows are the [begin, end) of its id in an ascending b_ids, cut at the clamped count, and every reader
//                      forces a range into the row table before it indexes with it: ranges_kernel, clamped_count, row_range
//
// and of the helpers the pnp and detection pipelines share beside them (block_best, mask_clear_kernel, align_up).  The two kernels are
// templates over the workgroup size they are launched with, so a library holds them only where it launches them.  Contraction is off here
// as in every file that includes this: each expression is evaluated in the written order.
#pragma once
#include <hip/hip_runtime.h>
#include <stddef.h>
#include <stdint.h>

#pragma clang fp contract(off)

namespace devloop {

// ---- the range rule ----------------------------------------------------------------------------------------------------------------------
// [begin, end) of group g (a frame, a view), forced into the row table whatever the ranges table holds
__device__ __forceinline__ void row_range(const int* ranges, int g, int cap, int& begin, int& end) {
    int b = ranges[2 * g], e = ranges[2 * g + 1];
    b = b < 0 ? 0 : (b > cap ? cap : b);
    e = e < b ? b : (e > cap ? cap : e);
    begin = b; end = e;
}

// count = NULL: every row of the table
__device__ __forceinline__ int clamped_count(const int* count, int cap) {
    const int n = count ? *count : cap;
    return n < 0 ? 0 : (n > cap ? cap : n);
}

// one thread per group; b_ids = NULL: one group holding every row (G == 1 is checked before the launch)
template <int Threads>
__global__ __launch_bounds__(Threads) void ranges_kernel(const long long* __restrict__ b_ids, const int* __restrict__ count, int cap, int G,
                                                         int* __restrict__ ranges) {
    const int g = blockIdx.x * blockDim.x + threadIdx.x;
    if (g >= G) return;
    const int n = clamped_count(count, cap);
    if (!b_ids) {
        ranges[2 * g] = 0; ranges[2 * g + 1] = g == 0 ? n : 0;
        return;
    }
    int res[2];
    for (int s = 0; s < 2; ++s) {                 // the first row whose id is >= g + s
        const long long key = (long long)g + s;
        int lo = 0, hi = n;
        for (int it = 0; it < 32 && lo < hi; ++it) {
            const int mid = lo + (hi - lo) / 2;
            if (b_ids[mid] < key) lo = mid + 1; else hi = mid;
        }
        res[s] = lo;
    }
    ranges[2 * g] = res[0]; ranges[2 * g + 1] = res[1] < res[0] ? res[0] : res[1];
}

template <int Threads>
__global__ __launch_bounds__(Threads) void mask_clear_kernel(const int* __restrict__ count, int cap, unsigned char* __restrict__ mask) {
    const int i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i < clamped_count(count, cap)) mask[i] = 0;
}

// ---- the sampler -------------------------------------------------------------------------------------------------------------------------
__device__ __forceinline__ uint64_t mix64(uint64_t z) {
    z ^= z >> 30; z *= 0xBF58476D1CE4E5B9ull;
    z ^= z >> 27; z *= 0x94D049BB133111EBull;
    z ^= z >> 31;
    return z;
}

// three distinct rows in [0, n), n >= 3, of trial `trial` of group `id`: counter-based, no rejection loop
__device__ __forceinline__ void draw3(uint64_t seed, int id, int trial, int n, int& a, int& b, int& c) {
    const uint64_t base = (((uint64_t)id << 32) | (uint64_t)trial) * 4ull;
    const uint64_t G = 0x9E3779B97F4A7C15ull;
    a = (int)(mix64(seed + G * (base + 1ull)) % (uint64_t)n);
    b = (int)(mix64(seed + G * (base + 2ull)) % (uint64_t)(n - 1));
    if (b >= a) ++b;
    c = (int)(mix64(seed + G * (base + 3ull)) % (uint64_t)(n - 2));
    const int lo = a < b ? a : b, hi = a < b ? b : a;
    if (c >= lo) ++c;
    if (c >= hi) ++c;
}

// ---- the crop geometry -------------------------------------------------------------------------------------------------------------------
// true when v truncates toward zero to an int32 (false for NaN and the infinities)
__device__ __forceinline__ bool fits_int32(double v) { return v > -2147483649.0 && v < 2147483648.0; }

// crop_geometry's expression (include/onepose_track.h): entry e = 3 i + j of trans and of K_crop = trans K for box b
__device__ __forceinline__ void geometry_entry(const int* b, const double* __restrict__ K, int S, int e, double* __restrict__ K_crop,
                                               double* __restrict__ trans) {
    const double x0 = (double)b[0], y0 = (double)b[1], x1 = (double)b[2], y1 = (double)b[3];
    const double wb = x1 - x0, hb = y1 - y0;
    const double s = (double)S / wb;
    const int i = e / 3, j = e - 3 * i;
    double t0, t1, t2;
    if (i == 0) {
        t0 = s; t1 = 0.0; t2 = -s * x0;
    } else if (i == 1) {
        t0 = 0.0; t1 = s; t2 = 0.5 * (double)S - s * (y0 + 0.5 * hb);
    } else {
        t0 = 0.0; t1 = 0.0; t2 = 1.0;
    }
    trans[e] = j == 0 ? t0 : (j == 1 ? t1 : t2);
    K_crop[e] = ((t0 * K[j]) + (t1 * K[3 + j])) + (t2 * K[6 + j]);
}

// ---- shared helpers ----------------------------------------------------------------------------------------------------------------------
// the first of a workgroup's candidates under the file's own `bool better(const Best&, const Best&)` (a total order, so the tree's shape
// cannot change the winner); sh: Threads entries of LDS; every thread gets the result
template <int Threads, typename Best>
__device__ __forceinline__ Best block_best(Best mine, Best* sh) {
    sh[threadIdx.x] = mine;
    __syncthreads();
    for (int s = Threads / 2; s > 0; s >>= 1) {
        if ((int)threadIdx.x < s && better(sh[threadIdx.x + s], sh[threadIdx.x])) sh[threadIdx.x] = sh[threadIdx.x + s];
        __syncthreads();
    }
    const Best r = sh[0];
    __syncthreads();
    return r;
}

// workspace offsets: multiples of 256 bytes
inline size_t align_up(size_t x) { return (x + 255) & ~(size_t)255; }

}  // namespace devloop
