// The keypoint-free SfM's track assignment and row tables (include/onepose_sfm_tracks.h):
// get_keyframes_greedy / build_initial_depth_pose (dataset/coarse_colmap_dataset.py:115-171, 220-310), MatchingPairData
// (data_construct/construct_matching_data.py) and ConstructOptimizationData (data_construct/construct_optimization_data.py).
//
//   assign       the greedy rounds.  Only the rounds are sequential: a round is select_kernel (one workgroup, one remaining image per
//                thread: the stable descending sort of the carried order by unoccupied count, as a rank count in LDS; the first image
//                becomes the keyframe and leaves the order) and take_kernel (16 lanes per slot of the keyframe: an unoccupied slot
//                takes its point, the lanes walk the point's track and rob every element in another image with one compare-and-swap,
//                which also decrements that image's count -- each element is robbed at most once over all rounds, and no round
//                touches more than the keyframe's own tracks).  All I rounds are enqueued back to back; every launch reads the done
//                flag first.  No cooperative launch, no workgroup waits for another.  Integer atomics only (max, sub, cas) on values
//                whose final state does not depend on the order, so every output is identical run to run.
//   finish       the states as point ids and z of K (R X + t) on the occupied slots, float64, in the written order (this file is
//                compiled with -ffp-contract=off)
//   track_rows   per track element: first occurrence of its image in the track, and the keypoints of the first and the last occurrence
//   pair_keys / pair_emit
//                the fine matcher's rows: a sort key per row (the caller sorts), then the copies of the keypoints in the sorted order
//   fine_rows    per optimiser row the one pair row it reads, by binary search, with a device-side error flag
// Sorts, scans and compaction of the integer tables between these launches are the caller's (sfm_tracks.py).
//
// Seeded faults for the tests (tools/build_variant.sh sfm_tracks, EXTRA=-DOPSFT_FAULT_...): never defined in the product build.
#include <hip/hip_runtime.h>
#include <stdint.h>
#include "onepose_sfm_tracks.h"
#include "capi_error.h"

using capi::bad_arg;
using capi::blocks_of;
using capi::fail;
using capi::g_error;

namespace {

constexpr int kThreads = 256;                     // 4 waves of 64
constexpr int kSelectThreads = OPSFT_MAX_IMAGES;  // one remaining image per thread
constexpr int kLanesPerSlot = 16;                 // lanes that walk one slot's track (the mean track is ~20 elements)
constexpr int kMaxTakeBlocks = 2048;
static_assert(kSelectThreads <= 1024, "one workgroup");

// ---- the greedy rounds -----------------------------------------------------------------------------------------------------------------
// Python's sorted(items, key=count, reverse=True) is stable and the sorted dict is carried into the next round: the rank of the image at
// carried position i is the number of images with a larger count plus the number with an equal count at an earlier position.
__global__ __launch_bounds__(kSelectThreads) void select_kernel(const int* count, int* order, int* keyframes, int* ctrl, int I) {
    __shared__ int s_cnt[kSelectThreads];
    __shared__ int s_img[kSelectThreads];
    if (ctrl[0]) return;                          // done: uniform over the workgroup
    const int n = min(ctrl[1], I);
    const int n_kf = ctrl[2];
    const int i = threadIdx.x;
    int img = -1, c = -1;
    if (i < n) {
        img = order[i];
        c = (img >= 0 && img < I) ? count[img] : -1;
    }
    s_cnt[i] = c;
    s_img[i] = img;
    __syncthreads();
    int rank = -1;
    if (i < n) {
        rank = 0;
        for (int j = 0; j < n; ++j) {
            const int cj = s_cnt[j];
#ifdef OPSFT_FAULT_TIE_INITIAL_ORDER
            rank += (cj > c) || (cj == c && s_img[j] < img);
#else
            rank += (cj > c) || (cj == c && j < i);
#endif
        }
    }
    __syncthreads();                              // every thread has read ctrl and order
    if (n == 0) {
        if (i == 0) ctrl[0] = 1;
        return;
    }
    if (rank == 0) {
        if (c <= 0 || n_kf >= I) {
            ctrl[0] = 1;                          // no unoccupied slot is left: every point is assigned
        } else {
            keyframes[n_kf] = img;
            ctrl[2] = n_kf + 1;
            ctrl[3] = img;
            ctrl[1] = n - 1;
        }
    } else if (rank > 0) {
        order[rank - 1] = img;                    // the popped image leaves the order
    }
}

struct TakeTables {
    const long long *kpt_offsets, *slot_point, *track_offsets, *elem_image, *elem_slot;
    int I, Q;
    long long U, E;
};

__global__ __launch_bounds__(kThreads) void take_kernel(TakeTables t, int* state, int* count, int* assigned_image, int* assigned_kpt,
                                                        const int* ctrl) {
    if (ctrl[0]) return;
    const int kf = ctrl[3];
    if (kf < 0 || kf >= t.I) return;
    const long long k0 = t.kpt_offsets[kf], k1 = min(t.kpt_offsets[kf + 1], t.U);
    if (k0 < 0) return;
    const int sub = threadIdx.x & (kLanesPerSlot - 1);
    const long long group = ((long long)blockIdx.x * kThreads + threadIdx.x) / kLanesPerSlot;
    const long long n_groups = (long long)gridDim.x * (kThreads / kLanesPerSlot);
    for (long long s = k0 + group; s < k1; s += n_groups) {
        const int st = __shfl(state[s], 0, kLanesPerSlot);        // lane 0 of the group writes state[s] below: one read for all
#ifdef OPSFT_FAULT_ROBBED_IS_OWNED
        if (st != -2 && st != -3) continue;
#else
        if (st != -2) continue;
#endif
        const long long p = t.slot_point[s];
        if (p < 0 || p >= t.Q) continue;
        if (sub == 0) {
            state[s] = (int)p;
            assigned_image[p] = kf;
#ifdef OPSFT_FAULT_FIRST_KEYPOINT_WINS
            atomicMin((unsigned*)&assigned_kpt[p], (unsigned)(s - k0));
#else
            atomicMax(&assigned_kpt[p], (int)(s - k0));            // two keypoints of one point in the keyframe: the later write wins
#endif
        }
        const long long e0 = max(t.track_offsets[p], 0LL), e1 = min(t.track_offsets[p + 1], t.E);
        for (long long e = e0 + sub; e < e1; e += kLanesPerSlot) {
            const long long img = t.elem_image[e], slot = t.elem_slot[e];
            if (img == kf || img < 0 || img >= t.I || slot < 0 || slot >= t.U) continue;
            if (atomicCAS(&state[slot], -2, -3) == -2) atomicSub(&count[img], 1);
        }
    }
}

__global__ __launch_bounds__(kThreads) void finish_kernel(const int* state, const long long* slot_image, const long long* point_ids,
                                                          const double* xyz, const double* K, const double* R, const double* t, int I,
                                                          long long U, int Q, long long* state_ids, double* initial_depth) {
    const long long u = (long long)blockIdx.x * kThreads + threadIdx.x;
    if (u >= U) return;
    const int st = state[u];
    const long long img = slot_image[u];
    long long id = st;
    double depth = -1.0;
    if (st >= 0 && st < Q && img >= 0 && img < I) {
        id = point_ids[st];
        const double* X = xyz + 3 * (long long)st;
        const double* Ri = R + 9 * img;
        const double* Ki = K + 9 * img;
        const double* ti = t + 3 * img;
        const double cx = ((Ri[0] * X[0] + Ri[1] * X[1]) + Ri[2] * X[2]) + ti[0];
        const double cy = ((Ri[3] * X[0] + Ri[4] * X[1]) + Ri[5] * X[2]) + ti[1];
        const double cz = ((Ri[6] * X[0] + Ri[7] * X[1]) + Ri[8] * X[2]) + ti[2];
        depth = (Ki[6] * cx + Ki[7] * cy) + Ki[8] * cz;
    }
    state_ids[u] = id;
    initial_depth[u] = depth;
}

// ---- row tables ------------------------------------------------------------------------------------------------------------------------
__global__ __launch_bounds__(kThreads) void track_rows_kernel(const long long* track_offsets, const long long* elem_point,
                                                              const long long* elem_image, const long long* track_kpt,
                                                              const int* assigned_image, int Q, long long E, unsigned char* other,
                                                              long long* match_kpt, long long* ref_kpt) {
    const long long e = (long long)blockIdx.x * kThreads + threadIdx.x;
    if (e >= E) return;
    const long long p = elem_point[e];
    unsigned char flag = 0;
    long long mk = -1, rk = -1;
    if (p >= 0 && p < Q) {
        const long long e0 = max(track_offsets[p], 0LL), e1 = min(track_offsets[p + 1], E);
        const long long img = elem_image[e];
        bool first = e >= e0 && e < e1;
        for (long long j = e0; first && j < e; ++j) first = elem_image[j] != img;
        if (first) {
            long long last = e;
            for (long long j = e + 1; j < e1; ++j)
                if (elem_image[j] == img) last = j;
            flag = img != assigned_image[p];
#ifdef OPSFT_FAULT_LAST_OCCURRENCE
            mk = track_kpt[last];
#else
            mk = track_kpt[e];
#endif
            rk = track_kpt[last];
        }
    }
    other[e] = flag;
    match_kpt[e] = mk;
    ref_kpt[e] = rk;
}

struct PairTables {
    const long long *owner_slot, *row_elem, *slot_image, *kpt_offsets, *elem_image;
    int I;
    long long U, E, M;
};

// pair row m -> left image, left keypoint, right image; false if a table points outside
__device__ __forceinline__ bool pair_row(const PairTables& t, long long m, long long* slot, long long* left, long long* kpt, long long* e,
                                         long long* right) {
    *slot = t.owner_slot[m];
    *e = t.row_elem[m];
    if (*slot < 0 || *slot >= t.U || *e < 0 || *e >= t.E) return false;
    *left = t.slot_image[*slot];
    *right = t.elem_image[*e];
    if (*left < 0 || *left >= t.I || *right < 0 || *right >= t.I) return false;
    *kpt = *slot - t.kpt_offsets[*left];
    return true;
}

__global__ __launch_bounds__(kThreads) void pair_keys_kernel(PairTables t, const long long* id_rank, long long key_stride, long long* keys) {
    const long long m = (long long)blockIdx.x * kThreads + threadIdx.x;
    if (m >= t.M) return;
    long long slot, left, kpt, e, right, key = -1;
    if (pair_row(t, m, &slot, &left, &kpt, &e, &right)) {
#ifdef OPSFT_FAULT_RIGHT_BY_INDEX
        const long long r = right;
#else
        const long long r = id_rank[right];                       // np.unique: the right images ascend by COLMAP id
#endif
        key = (left * t.I + r) * key_stride + kpt;
    }
    keys[m] = key;
}

__global__ __launch_bounds__(kThreads) void pair_emit_kernel(PairTables t, const long long* perm, const long long* match_kpt,
                                                             const double* xys, double* mkpts0_c, double* mkpts1_c, long long* mkpts0_idx,
                                                             long long* row_left, long long* row_right) {
    const long long r = (long long)blockIdx.x * kThreads + threadIdx.x;
    if (r >= t.M) return;
    const long long m = perm[r];
    long long slot, left = -1, kpt = -1, e, right = -1;
    double a0 = 0.0, a1 = 0.0, b0 = 0.0, b1 = 0.0;
    if (m >= 0 && m < t.M && pair_row(t, m, &slot, &left, &kpt, &e, &right)) {
        a0 = xys[2 * slot];
        a1 = xys[2 * slot + 1];
        const long long other = t.kpt_offsets[right] + match_kpt[e];
        if (match_kpt[e] >= 0 && other < t.U) {
            b0 = xys[2 * other];
            b1 = xys[2 * other + 1];
        }
    }
    mkpts0_c[2 * r] = a0;
    mkpts0_c[2 * r + 1] = a1;
    mkpts1_c[2 * r] = b0;
    mkpts1_c[2 * r + 1] = b1;
    mkpts0_idx[r] = kpt;
    row_left[r] = left;
    row_right[r] = right;
}

__global__ __launch_bounds__(kThreads) void fine_rows_kernel(const long long* row_point, const long long* ref_image, const int* assigned_image,
                                                             const int* assigned_kpt, const long long* image_ids, const long long* pair_left,
                                                             const long long* pair_right, const long long* pair_offsets,
                                                             const long long* mkpts0_idx, int I, int Q, long long R, long long Np, long long M,
                                                             long long* fine_row, int* error_flag) {
    const long long j = (long long)blockIdx.x * kThreads + threadIdx.x;
    if (j >= R) return;
    long long found = -1;
    const long long p = row_point[j], right = ref_image[j];
    if (p >= 0 && p < Q && right >= 0 && right < I) {
        const long long left = assigned_image[p], kpt = assigned_kpt[p], right_id = image_ids[right];
        long long lo = 0, hi = Np;                                // the first pair not below (left, right id)
        while (lo < hi) {
            const long long mid = (lo + hi) >> 1;
            const long long pl = pair_left[mid], pr = pair_right[mid];
            const long long pid = (pr >= 0 && pr < I) ? image_ids[pr] : -1;
            if (pl < left || (pl == left && pid < right_id)) lo = mid + 1;
            else hi = mid;
        }
        if (lo < Np && pair_left[lo] == left && pair_right[lo] == right) {
            const long long r0 = max(pair_offsets[lo], 0LL), r1 = min(pair_offsets[lo + 1], M);
            long long a = r0, b = r1;                             // lower bound of kpt
            while (a < b) {
                const long long mid = (a + b) >> 1;
                if (mkpts0_idx[mid] < kpt) a = mid + 1;
                else b = mid;
            }
            long long c = a, d = r1;                              // upper bound
            while (c < d) {
                const long long mid = (c + d) >> 1;
                if (mkpts0_idx[mid] <= kpt) c = mid + 1;
                else d = mid;
            }
            if (c - a == 1) found = a;
        }
    }
    fine_row[j] = found;
    if (found < 0) atomicOr(error_flag, 1);
}

}  // namespace

extern "C" {

int opsft_abi_version(void) { return OPSFT_ABI_VERSION; }
const char* opsft_last_error(void) { return g_error; }

int opsft_assign(const long long* kpt_offsets, const long long* slot_point, const long long* track_offsets, const long long* elem_image,
                 const long long* elem_slot, int I, long long U, int Q, long long E, int max_slots, int* state, int* count, int* order,
                 int* assigned_image, int* assigned_kpt, int* keyframes, int* ctrl, void* stream) {
    if (I < 1 || I > OPSFT_MAX_IMAGES) return bad_arg(__func__, "between 1 and OPSFT_MAX_IMAGES images");
    if (U < 1 || U > OPSFT_MAX_ITEMS || Q < 1 || Q > OPSFT_MAX_ITEMS || E < 1 || E > OPSFT_MAX_ITEMS || max_slots < 1 || max_slots > U)
        return bad_arg(__func__, "table sizes");
    if (!kpt_offsets || !slot_point || !track_offsets || !elem_image || !elem_slot || !state || !count || !order || !assigned_image ||
        !assigned_kpt || !keyframes || !ctrl)
        return bad_arg(__func__, "null pointer");
    hipStream_t s = (hipStream_t)stream;
    const TakeTables t{kpt_offsets, slot_point, track_offsets, elem_image, elem_slot, I, Q, U, E};
    const unsigned take_blocks = min(blocks_of(max_slots, kThreads / kLanesPerSlot), (unsigned)kMaxTakeBlocks);
    for (int round = 0; round < I; ++round) {
        select_kernel<<<1, kSelectThreads, 0, s>>>(count, order, keyframes, ctrl, I);
        take_kernel<<<take_blocks, kThreads, 0, s>>>(t, state, count, assigned_image, assigned_kpt, ctrl);
    }
    select_kernel<<<1, kSelectThreads, 0, s>>>(count, order, keyframes, ctrl, I);      // sets the done flag after the I-th keyframe
    CAPI_CHECK_LAUNCH();
    return 0;
}

int opsft_finish(const int* state, const long long* slot_image, const long long* point_ids, const double* xyz, const double* K,
                 const double* R, const double* t, int I, long long U, int Q, long long* state_ids, double* initial_depth, void* stream) {
    if (I < 1 || U < 1 || U > OPSFT_MAX_ITEMS || Q < 1) return bad_arg(__func__, "table sizes");
    if (!state || !slot_image || !point_ids || !xyz || !K || !R || !t || !state_ids || !initial_depth) return bad_arg(__func__, "null pointer");
    finish_kernel<<<blocks_of(U, kThreads), kThreads, 0, (hipStream_t)stream>>>(state, slot_image, point_ids, xyz, K, R, t, I, U, Q,
                                                                                   state_ids, initial_depth);
    CAPI_CHECK_LAUNCH();
    return 0;
}

int opsft_track_rows(const long long* track_offsets, const long long* elem_point, const long long* elem_image, const long long* track_kpt,
                     const int* assigned_image, int Q, long long E, unsigned char* other, long long* match_kpt, long long* ref_kpt,
                     void* stream) {
    if (Q < 1 || E < 1 || E > OPSFT_MAX_ITEMS) return bad_arg(__func__, "table sizes");
    if (!track_offsets || !elem_point || !elem_image || !track_kpt || !assigned_image || !other || !match_kpt || !ref_kpt)
        return bad_arg(__func__, "null pointer");
    track_rows_kernel<<<blocks_of(E, kThreads), kThreads, 0, (hipStream_t)stream>>>(track_offsets, elem_point, elem_image, track_kpt,
                                                                                       assigned_image, Q, E, other, match_kpt, ref_kpt);
    CAPI_CHECK_LAUNCH();
    return 0;
}

int opsft_pair_keys(const long long* owner_slot, const long long* row_elem, const long long* slot_image, const long long* kpt_offsets,
                    const long long* elem_image, const long long* id_rank, int I, long long U, long long E, long long M,
                    long long key_stride, long long* keys, void* stream) {
    if (I < 1 || I > OPSFT_MAX_IMAGES || U < 1 || E < 1 || M < 1 || M > OPSFT_MAX_ITEMS || key_stride < 1 || key_stride > OPSFT_MAX_ITEMS)
        return bad_arg(__func__, "table sizes");
    if (!owner_slot || !row_elem || !slot_image || !kpt_offsets || !elem_image || !id_rank || !keys) return bad_arg(__func__, "null pointer");
    const PairTables t{owner_slot, row_elem, slot_image, kpt_offsets, elem_image, I, U, E, M};
    pair_keys_kernel<<<blocks_of(M, kThreads), kThreads, 0, (hipStream_t)stream>>>(t, id_rank, key_stride, keys);
    CAPI_CHECK_LAUNCH();
    return 0;
}

int opsft_pair_emit(const long long* perm, const long long* owner_slot, const long long* row_elem, const long long* slot_image,
                    const long long* kpt_offsets, const long long* elem_image, const long long* match_kpt, const double* xys, int I,
                    long long U, long long E, long long M, double* mkpts0_c, double* mkpts1_c, long long* mkpts0_idx,
                    long long* row_left, long long* row_right, void* stream) {
    if (I < 1 || I > OPSFT_MAX_IMAGES || U < 1 || E < 1 || M < 1 || M > OPSFT_MAX_ITEMS) return bad_arg(__func__, "table sizes");
    if (!perm || !owner_slot || !row_elem || !slot_image || !kpt_offsets || !elem_image || !match_kpt || !xys || !mkpts0_c || !mkpts1_c ||
        !mkpts0_idx || !row_left || !row_right)
        return bad_arg(__func__, "null pointer");
    const PairTables t{owner_slot, row_elem, slot_image, kpt_offsets, elem_image, I, U, E, M};
    pair_emit_kernel<<<blocks_of(M, kThreads), kThreads, 0, (hipStream_t)stream>>>(t, perm, match_kpt, xys, mkpts0_c, mkpts1_c, mkpts0_idx,
                                                                                      row_left, row_right);
    CAPI_CHECK_LAUNCH();
    return 0;
}

int opsft_fine_rows(const long long* row_point, const long long* ref_image, const int* assigned_image, const int* assigned_kpt,
                    const long long* image_ids, const long long* pair_left, const long long* pair_right, const long long* pair_offsets,
                    const long long* mkpts0_idx, int I, int Q, long long R, long long Np, long long M, long long* fine_row,
                    int* error_flag, void* stream) {
    if (I < 1 || Q < 1 || R < 1 || R > OPSFT_MAX_ITEMS || Np < 1 || M < 1) return bad_arg(__func__, "table sizes");
    if (!row_point || !ref_image || !assigned_image || !assigned_kpt || !image_ids || !pair_left || !pair_right || !pair_offsets ||
        !mkpts0_idx || !fine_row || !error_flag)
        return bad_arg(__func__, "null pointer");
    fine_rows_kernel<<<blocks_of(R, kThreads), kThreads, 0, (hipStream_t)stream>>>(row_point, ref_image, assigned_image, assigned_kpt,
                                                                                      image_ids, pair_left, pair_right, pair_offsets,
                                                                                      mkpts0_idx, I, Q, R, Np, M, fine_row, error_flag);
    CAPI_CHECK_LAUNCH();
    return 0;
}

}  // extern "C"
