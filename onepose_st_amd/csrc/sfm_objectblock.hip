// The keypoint-free SfM's object block (include/onepose_sfm.h): feature aggregation over tracks
// (feature_aggregation.py:10-180, "avg"), the point selection of postprocess (run.py:295-390: filter_bbox, get_tkl,
// filter_track_length, merge) and the per-point descriptor mean (feature_process.py:255-308, 527-541).
//
// What is pinned bit for bit is float arithmetic in a fixed order, so this file is compiled with -ffp-contract=off and every sum
// below is written in the order the reference adds:
//   aggregate    an integer pass takes the maximum writer ordinal per slot (the reference's loop order: tracks in order, a track's
//                reference rows in order, then its query slot), then one wave per writer writes if it is the winner.  A query writes
//                the float32 running sum of its rows in row order divided once by the count.  No float atomics.
//   box_test     0 < (p - c4).v < v.v, float64
//   pair_count / pair_emit
//                the N x N distance test, never stored: a workgroup holds kPerThread points per thread in registers, stages tiles of
//                partners in LDS (every lane reads the same address: a broadcast), and covers one chunk of the partner range, so the
//                grid is (point blocks) x (chunks).  It emits counts, and after the caller's scan the partner indices, ascending.
//   merge_resolve
//                one wave walks the points that have a partner in index order: a point whose partners hold a recorded point is
//                skipped (and, if no group holds it, dropped: the reference's quirk); otherwise it is accepted and records them all.
//   group_emit   float64 running mean of a group's members in ascending index order, and their ids
//   point_mean   one wave per point, lanes over the descriptor: float64 running sum over the observation rows in the given order
// Sorting, scans and compaction of the integer tables between these launches are the caller's (sfm_objectblock.py).
#include <hip/hip_runtime.h>
#include <stdint.h>
#include <math.h>
#include "onepose_sfm.h"
#include "capi_error.h"

using capi::bad_arg;
using capi::blocks_of;
using capi::fail;
using capi::g_error;

namespace {

constexpr int kThreads = 256;                     // 4 waves of 64
constexpr int kPerThread = 4;                     // points a thread of the pair test holds in registers
constexpr int kTile = OPSFM_PAIR_TILE;            // partners staged in LDS at a time
static_assert(kThreads * kPerThread == OPSFM_PAIR_BLOCK, "a workgroup's points");
static_assert(kTile == kThreads, "thread t stages partner t of the tile");

// ---- stage A -----------------------------------------------------------------------------------------------------------------------------
struct TrackTables {
    const long long *assigned_image, *assigned_kpt, *row_offsets, *ref_image, *ref_kpt, *kpt_offsets;
    int P, I;
    long long R, U;
};

// writer w: rows first (w < R: row w of the track that owns it), then one query writer per track (w = R + p).
// -> its slot (-1 if the tables point outside), its ordinal in the reference's loop order (1-based; 0 = nobody), its track
__device__ __forceinline__ void writer_of(const TrackTables& t, long long w, long long* slot, int* ordinal, int* track) {
    int p;
    long long img, kpt;
    if (w < t.R) {
        int lo = 0, hi = t.P - 1;                 // the last track p with row_offsets[p] <= w (every track owns at least one row)
        while (lo < hi) {
            const int mid = (lo + hi + 1) >> 1;
            if (t.row_offsets[mid] <= w) lo = mid;
            else hi = mid - 1;
        }
        p = lo;
        img = t.ref_image[w];
        kpt = t.ref_kpt[w];
        *ordinal = (int)(w + p + 1);
    } else {
        p = (int)(w - t.R);
        img = t.assigned_image[p];
        kpt = t.assigned_kpt[p];
        *ordinal = (int)(t.row_offsets[p + 1] + p + 1);
    }
    *track = p;
    long long s = -1;
    if (img >= 0 && img < t.I) {
        const long long k0 = t.kpt_offsets[img], k1 = t.kpt_offsets[img + 1];
        if (kpt >= 0 && kpt < k1 - k0 && k0 + kpt < t.U) s = k0 + kpt;
    }
    *slot = s;
}

__global__ __launch_bounds__(kThreads) void agg_winner_kernel(TrackTables t, int* winner, unsigned char* scores_cleared) {
    const long long w = (long long)blockIdx.x * kThreads + threadIdx.x;
    if (w >= t.R + t.P) return;
    long long slot;
    int ordinal, track;
    writer_of(t, w, &slot, &ordinal, &track);
    if (slot < 0) return;
    atomicMax(&winner[slot], ordinal);
    if (w >= t.R) scores_cleared[slot] = 1;       // every query clears its score, winner or not
}

// rows [r0, r1) of src [.][dim] -> dst [dim]: float32 running sum in row order (the first row starts it), one division by the count
__device__ __forceinline__ void mean_rows_f32(const float* src, long long r0, long long r1, int dim, float* dst, int lane) {
    const float cnt = (float)(r1 - r0);
    for (int d = lane; d < dim; d += 64) {
        float s = src[r0 * dim + d];
        for (long long r = r0 + 1; r < r1; ++r) s = s + src[r * dim + d];
        dst[d] = s / cnt;
    }
}

__global__ __launch_bounds__(kThreads) void agg_write_kernel(TrackTables t, const int* winner, const float* fc0, const float* fc1,
                                                              const float* f0, const float* f1, int dim_c, int dim_f, float* desc_coarse,
                                                              float* desc_fine, unsigned char* written) {
    const int lane = threadIdx.x & 63;
    const long long w = (long long)blockIdx.x * (kThreads / 64) + (threadIdx.x >> 6);     // one wave per writer
    if (w >= t.R + t.P) return;
    long long slot;
    int ordinal, track;
    writer_of(t, w, &slot, &ordinal, &track);
    if (slot < 0 || winner[slot] != ordinal) return;                                       // uniform over the wave
    float* dc = desc_coarse + slot * dim_c;
    float* df = desc_fine + slot * dim_f;
    if (w < t.R) {
        for (int d = lane; d < dim_c; d += 64) dc[d] = fc1[w * dim_c + d];
        for (int d = lane; d < dim_f; d += 64) df[d] = f1[w * dim_f + d];
    } else {
        const long long r0 = t.row_offsets[track], r1 = t.row_offsets[track + 1];
        mean_rows_f32(fc0, r0, r1, dim_c, dc, lane);
        mean_rows_f32(f0, r0, r1, dim_f, df, lane);
    }
    if (lane == 0) written[slot] = 1;
}

// ---- stage B -----------------------------------------------------------------------------------------------------------------------------
__global__ __launch_bounds__(kThreads) void box_test_kernel(const double* xyz, long long Q, const double* corners, unsigned char* keep) {
    const long long q = (long long)blockIdx.x * kThreads + threadIdx.x;
    if (q >= Q) return;
    const double cx = corners[12], cy = corners[13], cz = corners[14];
    const double dx = xyz[3 * q] - cx, dy = xyz[3 * q + 1] - cy, dz = xyz[3 * q + 2] - cz;
    bool in = true;
    const int other[3] = {5, 0, 7};               // v45, v40, v47
    for (int k = 0; k < 3; ++k) {
        const double vx = corners[3 * other[k]] - cx, vy = corners[3 * other[k] + 1] - cy, vz = corners[3 * other[k] + 2] - cz;
        const double m = (dx * vx + dy * vy) + dz * vz;
        const double vv = (vx * vx + vy * vy) + vz * vz;
        in = in && (0.0 < m) && (m < vv);
    }
    keep[q] = in ? 1 : 0;
}

// grid (point blocks, chunks).  EMIT = false: counts[j * C + c] = partners of j in chunk c; EMIT = true: their indices, ascending, from
// positions[j * C + c] on.  A partner is tested as s = (dx^2 + dy^2) + dz^2, sqrt(s) < thr; the square root is only taken when
// s < 4 thr^2 (beyond that it cannot be below thr), which leaves the decision exactly the reference's.
template <bool EMIT>
__global__ __launch_bounds__(kThreads) void pair_kernel(const double* xyz, int N, double thr, int chunk_len, int C, long long* counts,
                                                         const long long* positions, int* neighbours, long long E) {
    __shared__ double sx[kTile], sy[kTile], sz[kTile];
    const int tid = threadIdx.x;
    const double nan = __longlong_as_double(0x7ff8000000000000LL);
    const double near2 = 4.0 * thr * thr;
    double px[kPerThread], py[kPerThread], pz[kPerThread];
    long long cur[kPerThread];
    for (int k = 0; k < kPerThread; ++k) {
        const long long j = (long long)blockIdx.x * OPSFM_PAIR_BLOCK + k * kThreads + tid;
        const bool valid = j < N;
        px[k] = valid ? xyz[3 * j] : nan;         // a NaN point is close to nobody
        py[k] = valid ? xyz[3 * j + 1] : nan;
        pz[k] = valid ? xyz[3 * j + 2] : nan;
        cur[k] = EMIT && valid ? positions[j * C + blockIdx.y] : 0;
    }
    const long long i0 = (long long)blockIdx.y * chunk_len;
    const long long i1 = i0 + chunk_len < N ? i0 + chunk_len : N;
    for (long long t0 = i0; t0 < i1; t0 += kTile) {
        __syncthreads();
        const long long i = t0 + tid;
        sx[tid] = i < i1 ? xyz[3 * i] : nan;
        sy[tid] = i < i1 ? xyz[3 * i + 1] : nan;
        sz[tid] = i < i1 ? xyz[3 * i + 2] : nan;
        __syncthreads();
        const int nt = i1 - t0 < kTile ? (int)(i1 - t0) : kTile;
        for (int ii = 0; ii < nt; ++ii) {
            const double x = sx[ii], y = sy[ii], z = sz[ii];
#pragma unroll
            for (int k = 0; k < kPerThread; ++k) {
                const double dx = px[k] - x, dy = py[k] - y, dz = pz[k] - z;
                const double s = (dx * dx + dy * dy) + dz * dz;
                if (s < near2 && sqrt(s) < thr) {
                    if (EMIT) {
                        if (cur[k] >= 0 && cur[k] < E) neighbours[cur[k]] = (int)(t0 + ii);
                    }
                    ++cur[k];
                }
            }
        }
    }
    if (!EMIT) {
        for (int k = 0; k < kPerThread; ++k) {
            const long long j = (long long)blockIdx.x * OPSFM_PAIR_BLOCK + k * kThreads + tid;
            if (j < N) counts[j * C + blockIdx.y] = cur[k];
        }
    }
}

// one wave.  recorded [N] bytes start at 0.
__global__ __launch_bounds__(64) void merge_resolve_kernel(const long long* positions, int C, const int* neighbours, const long long* multi,
                                                            int M, int N, unsigned char* recorded, unsigned char* accepted) {
    const int lane = threadIdx.x;
    for (int t = 0; t < M; ++t) {
        const long long j = multi[t];
        if (j < 0 || j >= N) continue;            // uniform
        const long long e0 = positions[j * C], e1 = positions[(j + 1) * C];
        bool any = false;
        for (long long e = e0 + lane; e < e1; e += 64) {
            const int i = neighbours[e];
            any = any || (i >= 0 && i < N && recorded[i]);
        }
        if (__ballot(any) == 0ULL) {
            for (long long e = e0 + lane; e < e1; e += 64) {
                const int i = neighbours[e];
                if (i >= 0 && i < N) recorded[i] = 1;
            }
            if (lane == 0) accepted[j] = 1;
        }
        __threadfence_block();                    // the next point reads what this one recorded
        __syncthreads();
    }
}

__global__ __launch_bounds__(kThreads) void group_emit_kernel(const double* xyz, const long long* ids, const long long* accepted_idx,
                                                               const long long* positions, int C, const int* neighbours,
                                                               const long long* group_offsets, int G, int N, double* keypoints3d,
                                                               long long* group_members, long long members_total) {
    const int g = blockIdx.x * kThreads + threadIdx.x;
    if (g >= G) return;
    const long long j = accepted_idx[g];
    if (j < 0 || j >= N) return;
    const long long e0 = positions[j * C], e1 = positions[(j + 1) * C];
    const long long m0 = group_offsets[g];
    double sx = 0.0, sy = 0.0, sz = 0.0;
    for (long long e = e0; e < e1; ++e) {
        int i = neighbours[e];
        if (i < 0 || i >= N) i = (int)j;
        if (e == e0) {                            // np.add.reduce starts from the first row
            sx = xyz[3 * (long long)i];
            sy = xyz[3 * (long long)i + 1];
            sz = xyz[3 * (long long)i + 2];
        } else {
            sx = sx + xyz[3 * (long long)i];
            sy = sy + xyz[3 * (long long)i + 1];
            sz = sz + xyz[3 * (long long)i + 2];
        }
        const long long m = m0 + (e - e0);
        if (m >= 0 && m < members_total) group_members[m] = ids[i];
    }
    const double cnt = (double)(e1 - e0);
    keypoints3d[3 * (long long)g] = sx / cnt;
    keypoints3d[3 * (long long)g + 1] = sy / cnt;
    keypoints3d[3 * (long long)g + 2] = sz / cnt;
}

// ---- stage C -----------------------------------------------------------------------------------------------------------------------------
__global__ __launch_bounds__(kThreads) void point_mean_kernel(const float* table, long long U, int dim, const long long* obs,
                                                               const long long* run_offsets, int G, double* out) {
    const int lane = threadIdx.x & 63;
    const long long g = (long long)blockIdx.x * (kThreads / 64) + (threadIdx.x >> 6);      // one wave per point
    if (g >= G) return;
    const long long r0 = run_offsets[g], r1 = run_offsets[g + 1];
    const double cnt = (double)(r1 - r0);
    for (int d = lane; d < dim; d += 64) {
        double s = 0.0;
        for (long long r = r0; r < r1; ++r) {
            const long long u = obs[r];
            const double v = (u >= 0 && u < U) ? (double)table[u * dim + d] : 0.0;
            s = r == r0 ? v : s + v;
        }
        out[g * dim + d] = s / cnt;
    }
}

inline bool pair_sizes_ok(int N, int chunk_len, int C) {
    return N >= 1 && N <= OPSFM_MAX_ITEMS && chunk_len >= kTile && chunk_len % kTile == 0 && C >= 1 && C <= OPSFM_PAIR_MAX_CHUNKS &&
           (long long)chunk_len * C >= N;
}

}  // namespace

extern "C" int opsfm_abi_version(void) { return OPSFM_ABI_VERSION; }

extern "C" const char* opsfm_last_error(void) { return g_error; }

extern "C" size_t opsfm_workspace_bytes(long long n_slots, long long n_points) {
    if (n_slots < 0 || n_points < 0 || n_slots > OPSFM_MAX_ITEMS || n_points > OPSFM_MAX_ITEMS) return 0;
    const size_t a = (size_t)n_slots * 4, b = (size_t)n_points;
    return (((a > b ? a : b) + 255) & ~(size_t)255) + 256;
}

extern "C" int opsfm_aggregate(const long long* assigned_image, const long long* assigned_kpt, const long long* row_offsets,
                               const long long* ref_image, const long long* ref_kpt, const float* feature_c0, const float* feature_c1,
                               const float* feature0, const float* feature1, const long long* kpt_offsets, int P, long long R, int I,
                               long long U, int dim_c, int dim_f, void* workspace, size_t workspace_bytes, float* desc_coarse,
                               float* desc_fine, unsigned char* written, unsigned char* scores_cleared, void* stream_) {
    if (!assigned_image || !assigned_kpt || !row_offsets || !ref_image || !ref_kpt || !feature_c0 || !feature_c1 || !feature0 || !feature1 ||
        !kpt_offsets || !workspace || !desc_coarse || !desc_fine || !written || !scores_cleared)
        return bad_arg(__func__, "null pointer");
    if (P < 1 || R < P || I < 1 || U < 1 || dim_c < 1 || dim_f < 1 || R + P > OPSFM_MAX_ITEMS || U > OPSFM_MAX_ITEMS)
        return bad_arg(__func__, "bad sizes");
    if (workspace_bytes < (size_t)U * 4) return bad_arg(__func__, "workspace too small (opsfm_workspace_bytes)");
    if ((uintptr_t)workspace & 255) return bad_arg(__func__, "workspace 256-byte aligned");
    hipStream_t stream = (hipStream_t)stream_;
    int* winner = static_cast<int*>(workspace);
    hipError_t e = hipMemsetAsync(winner, 0, (size_t)U * 4, stream);
    if (e == hipSuccess) e = hipMemsetAsync(desc_coarse, 0, (size_t)U * dim_c * 4, stream);
    if (e == hipSuccess) e = hipMemsetAsync(desc_fine, 0, (size_t)U * dim_f * 4, stream);
    if (e == hipSuccess) e = hipMemsetAsync(written, 0, (size_t)U, stream);
    if (e == hipSuccess) e = hipMemsetAsync(scores_cleared, 0, (size_t)U, stream);
    if (e != hipSuccess) return fail(e, __func__);
    const TrackTables t{assigned_image, assigned_kpt, row_offsets, ref_image, ref_kpt, kpt_offsets, P, I, R, U};
    const long long W = R + P;
    hipLaunchKernelGGL(agg_winner_kernel, dim3(blocks_of(W, kThreads)), dim3(kThreads), 0, stream, t, winner, scores_cleared);
    hipLaunchKernelGGL(agg_write_kernel, dim3(blocks_of(W, kThreads / 64)), dim3(kThreads), 0, stream, t, winner, feature_c0, feature_c1,
                       feature0, feature1, dim_c, dim_f, desc_coarse, desc_fine, written);
    CAPI_CHECK_LAUNCH();
    return 0;
}

extern "C" int opsfm_box_test(const double* xyz, long long Q, const double* corners, unsigned char* keep, void* stream_) {
    if (!xyz || !corners || !keep) return bad_arg(__func__, "null pointer");
    if (Q < 1 || Q > OPSFM_MAX_ITEMS) return bad_arg(__func__, "bad sizes");
    hipLaunchKernelGGL(box_test_kernel, dim3(blocks_of(Q, kThreads)), dim3(kThreads), 0, (hipStream_t)stream_, xyz, Q, corners, keep);
    CAPI_CHECK_LAUNCH();
    return 0;
}

extern "C" int opsfm_pair_count(const double* xyz, int N, double dist_threshold, int chunk_len, int n_chunks, long long* counts,
                                void* stream_) {
    if (!xyz || !counts) return bad_arg(__func__, "null pointer");
    if (!pair_sizes_ok(N, chunk_len, n_chunks) || !(dist_threshold > 0.0)) return bad_arg(__func__, "bad sizes");
    hipLaunchKernelGGL(pair_kernel<false>, dim3(blocks_of(N, OPSFM_PAIR_BLOCK), n_chunks), dim3(kThreads), 0, (hipStream_t)stream_, xyz, N,
                       dist_threshold, chunk_len, n_chunks, counts, (const long long*)nullptr, (int*)nullptr, 0LL);
    CAPI_CHECK_LAUNCH();
    return 0;
}

extern "C" int opsfm_pair_emit(const double* xyz, int N, double dist_threshold, int chunk_len, int n_chunks, const long long* positions,
                               int* neighbours, long long E, void* stream_) {
    if (!xyz || !positions || !neighbours) return bad_arg(__func__, "null pointer");
    if (!pair_sizes_ok(N, chunk_len, n_chunks) || !(dist_threshold > 0.0) || E < N) return bad_arg(__func__, "bad sizes");
    hipLaunchKernelGGL(pair_kernel<true>, dim3(blocks_of(N, OPSFM_PAIR_BLOCK), n_chunks), dim3(kThreads), 0, (hipStream_t)stream_, xyz, N,
                       dist_threshold, chunk_len, n_chunks, (long long*)nullptr, positions, neighbours, E);
    CAPI_CHECK_LAUNCH();
    return 0;
}

extern "C" int opsfm_merge_resolve(const long long* positions, int n_chunks, const int* neighbours, const long long* multi, int M, int N,
                                   void* workspace, size_t workspace_bytes, unsigned char* accepted, void* stream_) {
    if (!positions || !neighbours || !workspace || !accepted || (M > 0 && !multi)) return bad_arg(__func__, "null pointer");
    if (N < 1 || M < 0 || M > N || n_chunks < 1) return bad_arg(__func__, "bad sizes");
    if (workspace_bytes < (size_t)N) return bad_arg(__func__, "workspace too small (opsfm_workspace_bytes)");
    if (M == 0) return 0;
    hipStream_t stream = (hipStream_t)stream_;
    unsigned char* recorded = static_cast<unsigned char*>(workspace);
    hipError_t e = hipMemsetAsync(recorded, 0, (size_t)N, stream);
    if (e != hipSuccess) return fail(e, __func__);
    hipLaunchKernelGGL(merge_resolve_kernel, dim3(1), dim3(64), 0, stream, positions, n_chunks, neighbours, multi, M, N, recorded, accepted);
    CAPI_CHECK_LAUNCH();
    return 0;
}

extern "C" int opsfm_group_emit(const double* xyz, const long long* ids, const long long* accepted_idx, const long long* positions,
                                int n_chunks, const int* neighbours, const long long* group_offsets, int G, int N, double* keypoints3d,
                                long long* group_members, long long members_total, void* stream_) {
    if (!xyz || !ids || !accepted_idx || !positions || !neighbours || !group_offsets || !keypoints3d || !group_members)
        return bad_arg(__func__, "null pointer");
    if (G < 1 || N < G || n_chunks < 1 || members_total < G) return bad_arg(__func__, "bad sizes");
    hipLaunchKernelGGL(group_emit_kernel, dim3(blocks_of(G, kThreads)), dim3(kThreads), 0, (hipStream_t)stream_, xyz, ids, accepted_idx,
                       positions, n_chunks, neighbours, group_offsets, G, N, keypoints3d, group_members, members_total);
    CAPI_CHECK_LAUNCH();
    return 0;
}

extern "C" int opsfm_point_mean(const float* table, long long U, int dim, const long long* obs, const long long* run_offsets, int G,
                                double* out, void* stream_) {
    if (!table || !obs || !run_offsets || !out) return bad_arg(__func__, "null pointer");
    if (U < 1 || dim < 1 || G < 1) return bad_arg(__func__, "bad sizes");
    hipLaunchKernelGGL(point_mean_kernel, dim3(blocks_of(G, kThreads / 64)), dim3(kThreads), 0, (hipStream_t)stream_, table, U, dim, obs,
                       run_offsets, G, out);
    CAPI_CHECK_LAUNCH();
    return 0;
}
