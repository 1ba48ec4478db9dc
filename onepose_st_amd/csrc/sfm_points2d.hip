// The keypoint-free SfM's coarse-match merge (src/KeypointFreeSfM/coarse_match/coarse_match.py:141-186, non-Ray branch): every pair's
// matches become one keypoint list per image (utils.py:20-61 Match2Pts2D, coarse_match_worker.py:87-111 points2D_worker with
// utils.py:5-18 agg_groupby_2d "sum"), index pairs into those lists (coarse_match_worker.py:119-155 update_matches) and float32
// keypoints / scores (:163-183 transform_points2D).
//
// Observation o = 2 t + side of row t is (image of that side, int(x), int(y), mconf[t]).  A pair never holds one image twice, so o
// ascending is the reference's occurrence order within every image.  The pipeline, integer-only apart from one float64 sum per key:
//   expand     key = image << 42 | (int(x) + 2^20) << 21 | (int(y) + 2^20), value = o
//   sort 1     stable LSD radix sort of (key, value), 8 bits a pass, only the passes the key width needs.  A pass is three launches:
//              per-tile digit histograms, one exclusive scan per digit over the tiles, and a stable scatter whose in-tile ranks come
//              from 64-lane __ballot matches.  No workgroup waits on another.
//   segment    heads of equal-key runs -> per-tile head counts -> one scan (its total U is the host's one read-back) -> unique ids
//   sum        one lane per unique key adds its run's mconf in float64 in run order (= occurrence order: the sort is stable)
//   sort 2     unique ids by the score's bits (descending), then stably by image: equal scores keep the (x, y) order of sort 1
//   emit       keypoints / float32 scores in rank order, per-image offsets, and match_ids [T][2] = rank of each observation's key
#include "tile.h"
#include "onepose_hip.h"
#include <stdint.h>

namespace {

constexpr int kThreads = 256;                     // 4 waves of 64
constexpr int kItems = 16;                        // elements per thread and tile
constexpr int kTile = kThreads * kItems;          // 4096 elements per tile
constexpr int kRadix = 256;                       // 8-bit digits
constexpr int kCoordBits = 21;                    // int(x) + 2^20 in [0, 2^21)
constexpr long long kCoordBias = 1LL << 20;
constexpr int kImageShift = 2 * kCoordBits;       // 42
constexpr unsigned long long kCoordMask = (1ULL << kCoordBits) - 1;
static_assert(kThreads == kRadix, "thread d of a scatter workgroup owns digit d");

// exclusive scan of one int per thread over the workgroup (kThreads); *total = the workgroup's sum.  lds: kThreads / 64 + 1 ints.
__device__ __forceinline__ int block_excl_scan(int v, int* lds, int* total) {
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    int incl = v;
    for (int d = 1; d < 64; d <<= 1) {
        const int up = __shfl_up(incl, d, 64);
        if (lane >= d) incl += up;
    }
    if (lane == 63) lds[wave] = incl;
    __syncthreads();
    int before = 0, sum = 0;
    for (int w = 0; w < kThreads / 64; ++w) {
        const int s = lds[w];
        if (w < wave) before += s;
        sum += s;
    }
    __syncthreads();                              // lds is reused by the caller's next scan
    *total = sum;
    return before + incl - v;
}

// ---- expand ----------------------------------------------------------------------------------------------------------------------------
__global__ __launch_bounds__(kThreads) void p2d_expand_kernel(const float* mk0, const float* mk1, const long long* offsets,
                                                               const long long* images, int P, long long n, unsigned long long* keys,
                                                               unsigned* vals) {
    const long long o = (long long)blockIdx.x * kThreads + threadIdx.x;
    if (o >= n) return;
    const long long t = o >> 1;
    const int side = (int)(o & 1);
    int lo = 0, hi = P - 1;                       // the last pair p with offsets[p] <= t (empty pairs share their offset)
    while (lo < hi) {
        const int mid = (lo + hi + 1) >> 1;
        if (offsets[mid] <= t) lo = mid;
        else hi = mid - 1;
    }
    const unsigned long long img = (unsigned long long)images[2 * (long long)lo + side];
    const float* mk = side ? mk1 : mk0;
    const long long x = (long long)(int)mk[2 * t], y = (long long)(int)mk[2 * t + 1];      // C conversion: truncation toward zero
    keys[o] = (img << kImageShift) | ((unsigned long long)(x + kCoordBias) << kCoordBits) | (unsigned long long)(y + kCoordBias);
    vals[o] = (unsigned)o;
}

// ---- one LSD radix pass ----------------------------------------------------------------------------------------------------------------
// hist[d * ntiles + tile] = how many of the tile's keys have digit d
__global__ __launch_bounds__(kThreads) void p2d_radix_hist_kernel(const unsigned long long* keys, long long n, int shift, int ntiles,
                                                                   int* hist) {
    __shared__ int h[kRadix];
    h[threadIdx.x] = 0;
    __syncthreads();
    const long long base = (long long)blockIdx.x * kTile;
    for (int it = 0; it < kItems; ++it) {
        const long long i = base + it * kThreads + threadIdx.x;
        if (i < n) atomicAdd(&h[(keys[i] >> shift) & (kRadix - 1)], 1);
    }
    __syncthreads();
    hist[(long long)threadIdx.x * ntiles + blockIdx.x] = h[threadIdx.x];
}

// workgroup d: hist[d][0 .. ntiles) -> exclusive prefix in place, digit_total[d] = the digit's count
__global__ __launch_bounds__(kThreads) void p2d_radix_scan_kernel(int* hist, int ntiles, int* digit_total) {
    __shared__ int lds[kThreads / 64 + 1];
    int* row = hist + (long long)blockIdx.x * ntiles;
    int carry = 0;
    for (int b = 0; b < ntiles; b += kThreads) {
        const int i = b + threadIdx.x;
        const int v = i < ntiles ? row[i] : 0;
        int tot;
        const int ex = block_excl_scan(v, lds, &tot);
        if (i < ntiles) row[i] = carry + ex;
        carry += tot;
    }
    if (threadIdx.x == 0) digit_total[blockIdx.x] = carry;
}

// stable scatter: element i of the tile goes to (keys before it with a smaller digit anywhere) + (keys with its digit in earlier tiles) +
// (keys with its digit earlier in this tile).  The tile is walked in chunks of kThreads in element order; within a chunk each wave
// matches its lanes' digits with 8 ballots, and the 4 waves' counts are combined in wave order.
__global__ __launch_bounds__(kThreads) void p2d_radix_scatter_kernel(const unsigned long long* keys_in, const unsigned* vals_in,
                                                                      unsigned long long* keys_out, unsigned* vals_out, long long n, int shift,
                                                                      int ntiles, const int* hist, const int* digit_total) {
    __shared__ int base[kRadix];
    __shared__ int cnt[kThreads / 64][kRadix];
    __shared__ int lds[kThreads / 64 + 1];
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    {
        int tot;
        const int ex = block_excl_scan(digit_total[tid], lds, &tot);
        base[tid] = ex + hist[(long long)tid * ntiles + blockIdx.x];
    }
    const unsigned long long lt = (1ULL << lane) - 1ULL;
    const long long tile0 = (long long)blockIdx.x * kTile;
    for (int it = 0; it < kItems; ++it) {
        if (tile0 + (long long)it * kThreads >= n) break;                      // uniform over the workgroup
        for (int w = 0; w < kThreads / 64; ++w) cnt[w][tid] = 0;
        __syncthreads();
        const long long i = tile0 + (long long)it * kThreads + tid;
        const bool valid = i < n;
        unsigned long long key = 0;
        unsigned val = 0;
        int d = 0;
        if (valid) {
            key = keys_in[i];
            val = vals_in[i];
            d = (int)((key >> shift) & (kRadix - 1));
        }
        unsigned long long match = __ballot(valid);
        for (int b = 0; b < 8; ++b) {
            const bool bit = (d >> b) & 1;
            const unsigned long long m = __ballot(valid && bit);
            match &= bit ? m : ~m;
        }
        const int rank = __popcll(match & lt);
        if (valid && rank == 0) cnt[wave][d] = __popcll(match);              // the lowest lane of each digit group
        __syncthreads();
        int run = base[tid];
        for (int w = 0; w < kThreads / 64; ++w) {                             // thread tid owns digit tid
            const int c = cnt[w][tid];
            cnt[w][tid] = run;
            run += c;
        }
        __syncthreads();
        if (valid) {
            const int dst = cnt[wave][d] + rank;
            keys_out[dst] = key;
            vals_out[dst] = val;
        }
        base[tid] = run;                                                      // read again only after the next chunk's first barrier
        __syncthreads();
    }
}

// ---- segments of equal keys ------------------------------------------------------------------------------------------------------------
__device__ __forceinline__ int is_head(const unsigned long long* keys, long long i, long long n) {
    return i < n && (i == 0 || keys[i] != keys[i - 1]) ? 1 : 0;
}

__global__ __launch_bounds__(kThreads) void p2d_head_count_kernel(const unsigned long long* keys, long long n, int* tile_count) {
    __shared__ int lds[kThreads / 64 + 1];
    const long long tile0 = (long long)blockIdx.x * kTile;
    int c = 0;
    for (int it = 0; it < kItems; ++it) c += is_head(keys, tile0 + (long long)it * kThreads + threadIdx.x, n);
    int tot;
    block_excl_scan(c, lds, &tot);
    if (threadIdx.x == 0) tile_count[blockIdx.x] = tot;
}

// one workgroup: exclusive prefix of count[0 .. m) in place, *total = the sum
__global__ __launch_bounds__(kThreads) void p2d_scan_one_kernel(int* count, int m, int* total) {
    __shared__ int lds[kThreads / 64 + 1];
    int carry = 0;
    for (int b = 0; b < m; b += kThreads) {
        const int i = b + threadIdx.x;
        const int v = i < m ? count[i] : 0;
        int tot;
        const int ex = block_excl_scan(v, lds, &tot);
        if (i < m) count[i] = carry + ex;
        carry += tot;
    }
    if (threadIdx.x == 0) *total = carry;
}

// unique id of every sorted element (heads before it, inclusive, minus one): ustart[u] = position of head u, ukey[u] = its key,
// obs_uid[observation] = u
__global__ __launch_bounds__(kThreads) void p2d_segment_kernel(const unsigned long long* keys, const unsigned* vals, long long n,
                                                                const int* tile_offset, int* ustart, unsigned long long* ukey, int* obs_uid) {
    __shared__ int lds[kThreads / 64 + 1];
    const long long tile0 = (long long)blockIdx.x * kTile;
    int carry = tile_offset[blockIdx.x];
    for (int it = 0; it < kItems; ++it) {
        if (tile0 + (long long)it * kThreads >= n) break;                      // uniform
        const long long i = tile0 + (long long)it * kThreads + threadIdx.x;
        const int h = is_head(keys, i, n);
        int tot;
        const int ex = block_excl_scan(h, lds, &tot);
        if (i < n) {
            const int u = carry + ex + h - 1;
            if (h) {
                ustart[u] = (int)i;
                ukey[u] = keys[i];
            }
            obs_uid[vals[i]] = u;
        }
        carry += tot;
    }
}

// ---- scores ----------------------------------------------------------------------------------------------------------------------------
// run u: sum of its observations' mconf, float64, in run order (np.bincount's sequential accumulation); skey = the bits ordered so that
// ascending skey = descending score; img_count[image] += 1 (integer)
__global__ __launch_bounds__(kThreads) void p2d_score_kernel(const int* ustart, const unsigned long long* ukey, int U, long long n,
                                                              const unsigned* vals, const float* mconf, double* score,
                                                              unsigned long long* skey, unsigned* uval, int* img_count, int I) {
    const int u = blockIdx.x * kThreads + threadIdx.x;
    if (u >= U) return;
    const long long s0 = ustart[u], s1 = u + 1 < U ? (long long)ustart[u + 1] : n;
    double s = 0.0;
    for (long long i = s0; i < s1; ++i) s = s + (double)mconf[vals[i] >> 1];
    score[u] = s;
    if (s == 0.0) s = 0.0;                                                    // -0.0 and +0.0 compare equal in the reference's sort
    unsigned long long b = (unsigned long long)__double_as_longlong(s);
    b = (b >> 63) ? ~b : (b | (1ULL << 63));                                  // ascending b = ascending score
    skey[u] = ~b;
    uval[u] = (unsigned)u;
    const unsigned long long img = ukey[u] >> kImageShift;
    if (img < (unsigned long long)I) atomicAdd(&img_count[img], 1);          // the host validates; a bad index never writes past
}

__global__ __launch_bounds__(kThreads) void p2d_image_key_kernel(const unsigned* uval, const unsigned long long* ukey, int U,
                                                                  unsigned long long* keys) {
    const int p = blockIdx.x * kThreads + threadIdx.x;
    if (p < U) keys[p] = ukey[uval[p]] >> kImageShift;
}

// one workgroup: kpt_offsets[0 .. I] (int64) from the per-image counts
__global__ __launch_bounds__(kThreads) void p2d_image_offsets_kernel(const int* img_count, int I, long long* kpt_offsets) {
    __shared__ int lds[kThreads / 64 + 1];
    long long carry = 0;
    for (int b = 0; b < I; b += kThreads) {
        const int i = b + threadIdx.x;
        const int v = i < I ? img_count[i] : 0;
        int tot;
        const int ex = block_excl_scan(v, lds, &tot);
        if (i < I) kpt_offsets[i] = carry + ex;
        carry += tot;
    }
    if (threadIdx.x == 0) kpt_offsets[I] = carry;
}

// position p of the ranked list: keypoint, float32 score, and the key's rank within its image
__global__ __launch_bounds__(kThreads) void p2d_emit_kernel(const unsigned* order, const unsigned long long* ukey, const double* score,
                                                             const long long* kpt_offsets, int U, int I, float* keypoints, float* scores,
                                                             int* rank) {
    const int p = blockIdx.x * kThreads + threadIdx.x;
    if (p >= U) return;
    const unsigned u = order[p];
    const unsigned long long k = ukey[u];
    const unsigned long long img = k >> kImageShift;
    keypoints[2 * (long long)p] = (float)((long long)((k >> kCoordBits) & kCoordMask) - kCoordBias);
    keypoints[2 * (long long)p + 1] = (float)((long long)(k & kCoordMask) - kCoordBias);
    scores[p] = (float)score[u];
    rank[u] = img < (unsigned long long)I ? (int)(p - kpt_offsets[img]) : -1;
}

__global__ __launch_bounds__(kThreads) void p2d_match_ids_kernel(const int* obs_uid, const int* rank, long long n, long long* match_ids) {
    const long long o = (long long)blockIdx.x * kThreads + threadIdx.x;
    if (o < n) match_ids[o] = rank[obs_uid[o]];
}

// ---- workspace ---------------------------------------------------------------------------------------------------------------------------
struct Workspace {
    size_t keys_a, keys_b, vals_a, vals_b, hist, digit_total, tile_count, ustart, ukey, obs_uid, score, rank, img_count, ctl, total;
};

inline long long tiles_of(long long n) { return (n + kTile - 1) / kTile; }

__host__ Workspace workspace_layout(long long T, int I) {
    auto up = [](size_t x) { return (x + 255) & ~(size_t)255; };
    const size_t n = (size_t)(2 * T), nt = (size_t)tiles_of(2 * T);
    Workspace w{};
    size_t o = 0;
    w.keys_a = o; o = up(o + n * 8);
    w.keys_b = o; o = up(o + n * 8);
    w.vals_a = o; o = up(o + n * 4);
    w.vals_b = o; o = up(o + n * 4);
    w.hist = o; o = up(o + (size_t)kRadix * nt * 4);
    w.digit_total = o; o = up(o + (size_t)kRadix * 4);
    w.tile_count = o; o = up(o + nt * 4);
    w.ustart = o; o = up(o + n * 4);
    w.ukey = o; o = up(o + n * 8);
    w.obs_uid = o; o = up(o + n * 4);
    w.score = o; o = up(o + n * 8);
    w.rank = o; o = up(o + n * 4);
    w.img_count = o; o = up(o + (size_t)I * 4);
    w.ctl = o; o = up(o + 16);
    w.total = o;
    return w;
}

inline bool sizes_ok(long long T, int I) { return T >= 1 && T <= OPHIP_SFM_POINTS2D_MAX_ROWS && I >= 1 && I <= OPHIP_SFM_POINTS2D_MAX_IMAGES; }

inline int bit_length(unsigned long long v) {
    int b = 0;
    while (v) { ++b; v >>= 1; }
    return b;
}

// stable sort of (keys, vals) at a / b by bits [0, bits): the result ends in a when the pass count is even, else in b; -> 1 if it is in b
int radix_sort(const char* fn, unsigned long long* ka, unsigned* va, unsigned long long* kb, unsigned* vb, long long n, int bits, int* hist,
               int* digit_total, hipStream_t stream, int* in_b) {
    const int nt = (int)tiles_of(n);
    int cur = 0;
    for (int shift = 0; shift < bits; shift += 8) {
        unsigned long long* ki = cur ? kb : ka;
        unsigned long long* ko = cur ? ka : kb;
        unsigned* vi = cur ? vb : va;
        unsigned* vo = cur ? va : vb;
        OPHIP_LAUNCH("sfm_p2d_radix_hist", stream, p2d_radix_hist_kernel, dim3(nt), dim3(kThreads), 0, stream, ki, n, shift, nt, hist);
        OPHIP_LAUNCH("sfm_p2d_radix_scan", stream, p2d_radix_scan_kernel, dim3(kRadix), dim3(kThreads), 0, stream, hist, nt, digit_total);
        OPHIP_LAUNCH("sfm_p2d_radix_scatter", stream, p2d_radix_scatter_kernel, dim3(nt), dim3(kThreads), 0, stream, ki, vi, ko, vo, n, shift,
                     nt, hist, digit_total);
        hipError_t e = hipGetLastError();
        if (e != hipSuccess) return ophip_fail(e, fn);
        cur ^= 1;
    }
    *in_b = cur;
    return 0;
}

}  // namespace

extern "C" size_t ophip_sfm_points2d_workspace_bytes(long long T, int I) {
    if (!sizes_ok(T, I)) return 0;
    return workspace_layout(T, I).total;
}

extern "C" int ophip_sfm_points2d_group(const float* mkpts0, const float* mkpts1, const long long* pair_offsets, const long long* pair_images,
                                        int P, long long T, int I, void* workspace, size_t workspace_bytes, int* unique_count, void* stream_) {
    if (!mkpts0 || !mkpts1 || !pair_offsets || !pair_images || !workspace || !unique_count) return ophip_bad_arg(__func__, "null pointer");
    if (!sizes_ok(T, I) || P < 1) return ophip_bad_arg(__func__, "bad sizes");
    const Workspace w = workspace_layout(T, I);
    if (workspace_bytes < w.total) return ophip_bad_arg(__func__, "workspace too small (ophip_sfm_points2d_workspace_bytes)");
    if ((uintptr_t)workspace & 255) return ophip_bad_arg(__func__, "workspace 256-byte aligned");
    hipStream_t stream = (hipStream_t)stream_;
    char* ws = static_cast<char*>(workspace);
    auto K = [&](size_t off) { return reinterpret_cast<unsigned long long*>(ws + off); };
    auto U32 = [&](size_t off) { return reinterpret_cast<unsigned*>(ws + off); };
    auto I32 = [&](size_t off) { return reinterpret_cast<int*>(ws + off); };
    const long long n = 2 * T;
    const int nt = (int)tiles_of(n);
    OPHIP_LAUNCH("sfm_p2d_expand", stream, p2d_expand_kernel, dim3((unsigned)((n + kThreads - 1) / kThreads)), dim3(kThreads), 0, stream,
                 mkpts0, mkpts1, pair_offsets, pair_images, P, n, K(w.keys_a), U32(w.vals_a));
    OPHIP_CHECK_LAUNCH();
    int in_b = 0;
    const int rc = radix_sort(__func__, K(w.keys_a), U32(w.vals_a), K(w.keys_b), U32(w.vals_b), n, kImageShift + bit_length((unsigned)(I - 1)),
                              I32(w.hist), I32(w.digit_total), stream, &in_b);
    if (rc) return rc;
    const unsigned long long* keys = in_b ? K(w.keys_b) : K(w.keys_a);
    const unsigned* vals = in_b ? U32(w.vals_b) : U32(w.vals_a);
    if (in_b) {                                                               // the ranking stage reads the sorted values at vals_a
        hipError_t e = hipMemcpyAsync(U32(w.vals_a), vals, (size_t)n * 4, hipMemcpyDeviceToDevice, stream);
        if (e != hipSuccess) return ophip_fail(e, __func__);
        vals = U32(w.vals_a);
    }
    OPHIP_LAUNCH("sfm_p2d_head_count", stream, p2d_head_count_kernel, dim3(nt), dim3(kThreads), 0, stream, keys, n, I32(w.tile_count));
    OPHIP_LAUNCH("sfm_p2d_scan_one", stream, p2d_scan_one_kernel, dim3(1), dim3(kThreads), 0, stream, I32(w.tile_count), nt, I32(w.ctl));
    OPHIP_LAUNCH("sfm_p2d_segment", stream, p2d_segment_kernel, dim3(nt), dim3(kThreads), 0, stream, keys, vals, n, I32(w.tile_count),
                 I32(w.ustart), K(w.ukey), I32(w.obs_uid));
    OPHIP_CHECK_LAUNCH();
    hipError_t e = hipMemcpyAsync(unique_count, I32(w.ctl), sizeof(int), hipMemcpyDeviceToDevice, stream);
    if (e != hipSuccess) return ophip_fail(e, __func__);
    return 0;
}

extern "C" int ophip_sfm_points2d_rank(const float* mconf, long long T, int I, int U, void* workspace, size_t workspace_bytes, float* keypoints,
                                       float* scores, long long* kpt_offsets, long long* match_ids, void* stream_) {
    if (!mconf || !workspace || !keypoints || !scores || !kpt_offsets || !match_ids) return ophip_bad_arg(__func__, "null pointer");
    if (!sizes_ok(T, I) || U < 1 || U > 2 * T) return ophip_bad_arg(__func__, "bad sizes");
    const Workspace w = workspace_layout(T, I);
    if (workspace_bytes < w.total) return ophip_bad_arg(__func__, "workspace too small (ophip_sfm_points2d_workspace_bytes)");
    if ((uintptr_t)workspace & 255) return ophip_bad_arg(__func__, "workspace 256-byte aligned");
    hipStream_t stream = (hipStream_t)stream_;
    char* ws = static_cast<char*>(workspace);
    auto K = [&](size_t off) { return reinterpret_cast<unsigned long long*>(ws + off); };
    auto U32 = [&](size_t off) { return reinterpret_cast<unsigned*>(ws + off); };
    auto I32 = [&](size_t off) { return reinterpret_cast<int*>(ws + off); };
    const long long n = 2 * T;
    const unsigned ug = (unsigned)((U + kThreads - 1) / kThreads);
    double* score = reinterpret_cast<double*>(ws + w.score);
    // sort 2 works in keys_b / vals_b (score keys) and keys_a (image keys); vals_a holds sort 1's values until the score kernel has run
    hipError_t e = hipMemsetAsync(ws + w.img_count, 0, (size_t)I * 4, stream);
    if (e != hipSuccess) return ophip_fail(e, __func__);
    OPHIP_LAUNCH("sfm_p2d_score", stream, p2d_score_kernel, dim3(ug), dim3(kThreads), 0, stream, I32(w.ustart), K(w.ukey), U, n, U32(w.vals_a),
                 mconf, score, K(w.keys_b), U32(w.vals_b), I32(w.img_count), I);
    OPHIP_CHECK_LAUNCH();
    int in_b = 0;
    int rc = radix_sort(__func__, K(w.keys_b), U32(w.vals_b), K(w.keys_a), U32(w.vals_a), U, 64, I32(w.hist), I32(w.digit_total), stream, &in_b);
    if (rc) return rc;                                                        // 8 passes: the order is back in keys_b / vals_b
    OPHIP_LAUNCH("sfm_p2d_image_key", stream, p2d_image_key_kernel, dim3(ug), dim3(kThreads), 0, stream, U32(w.vals_b), K(w.ukey), U, K(w.keys_b));
    OPHIP_CHECK_LAUNCH();
    rc = radix_sort(__func__, K(w.keys_b), U32(w.vals_b), K(w.keys_a), U32(w.vals_a), U, bit_length((unsigned)(I - 1)), I32(w.hist),
                    I32(w.digit_total), stream, &in_b);
    if (rc) return rc;
    const unsigned* order = in_b ? U32(w.vals_a) : U32(w.vals_b);
    OPHIP_LAUNCH("sfm_p2d_image_offsets", stream, p2d_image_offsets_kernel, dim3(1), dim3(kThreads), 0, stream, I32(w.img_count), I, kpt_offsets);
    OPHIP_LAUNCH("sfm_p2d_emit", stream, p2d_emit_kernel, dim3(ug), dim3(kThreads), 0, stream, order, K(w.ukey), score, kpt_offsets, U, I,
                 keypoints, scores, I32(w.rank));
    OPHIP_LAUNCH("sfm_p2d_match_ids", stream, p2d_match_ids_kernel, dim3((unsigned)((n + kThreads - 1) / kThreads)), dim3(kThreads), 0, stream,
                 I32(w.obs_uid), I32(w.rank), n, match_ids);
    OPHIP_CHECK_LAUNCH();
    return 0;
}
