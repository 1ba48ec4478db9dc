// The training-mode forward's one own step (include/ext/onepose_train_forward.h): the ground-truth rows of the sparse
// ground truth in ascending order, and the coarse match list cut and padded to exactly T rows.  The header is the specification.
//
// gt_count_kernel    one workgroup per OPTRN_BLOCK rows: the number of its ground-truth rows.
// gt_offsets_kernel  ONE workgroup: the block counts -> their exclusive prefix sum, in place, 256 at a time with a running carry; the total.
// gt_scatter_kernel  the workgroups of the first kernel: an exclusive scan of their own flags, then row r goes to offset + rank.
// pad_kernel         one lane per output row: a copy of a predicted row, or a ground-truth row drawn by the counter-based sampler.
// No atomics, no workgroup waits for another.
#include "capi_error.h"
#include "device_loop.h"
#include "ext/onepose_train_forward.h"

#pragma clang fp contract(off)

namespace {

using capi::bad_arg;
using capi::blocks_of;
using devloop::align_up;
using devloop::clamped_count;
using devloop::mix64;

constexpr int kThreads = OPTRN_BLOCK;
static_assert(kThreads == 256, "the scans below are written for 256 lanes");

__device__ __forceinline__ int gt_flag(const long long* __restrict__ gt_j, long long r, long long rows, int M) {
    if (r >= rows) return 0;
    const long long j = gt_j[r];
    return (j >= 0 && j < M) ? 1 : 0;
}

// inclusive scan of one int per lane over the workgroup (Hillis-Steele in LDS); every lane gets its own prefix, sh[kThreads - 1] the total
__device__ __forceinline__ int block_inclusive(int v, int* sh) {
    const int tid = threadIdx.x;
    sh[tid] = v;
    __syncthreads();
    for (int d = 1; d < kThreads; d <<= 1) {
        const int add = tid >= d ? sh[tid - d] : 0;
        __syncthreads();
        sh[tid] += add;
        __syncthreads();
    }
    return sh[tid];
}

__global__ __launch_bounds__(kThreads) void gt_count_kernel(const long long* __restrict__ gt_j, long long rows, int M, int* __restrict__ counts) {
    __shared__ int sh[kThreads];
    const long long r = (long long)blockIdx.x * kThreads + threadIdx.x;
    block_inclusive(gt_flag(gt_j, r, rows, M), sh);
    if (threadIdx.x == 0) counts[blockIdx.x] = sh[kThreads - 1];
}

__global__ __launch_bounds__(kThreads) void gt_offsets_kernel(int* __restrict__ counts, int blocks, int* __restrict__ n_gt_total) {
    __shared__ int sh[kThreads];
    int carry = 0;
    for (int base = 0; base < blocks; base += kThreads) {
        const int k = base + (int)threadIdx.x;
        const int v = k < blocks ? counts[k] : 0;
        const int incl = block_inclusive(v, sh);
        const int total = sh[kThreads - 1];
        if (k < blocks) counts[k] = carry + (incl - v);
        carry += total;
        __syncthreads();                                   // sh is written again by the next round
    }
    if (threadIdx.x == 0) *n_gt_total = carry;
}

__global__ __launch_bounds__(kThreads) void gt_scatter_kernel(const long long* __restrict__ gt_j, long long rows, int M,
                                                               const int* __restrict__ offsets, int* __restrict__ gt_rows) {
    __shared__ int sh[kThreads];
    const long long r = (long long)blockIdx.x * kThreads + threadIdx.x;
    const int flag = gt_flag(gt_j, r, rows, M);
    const int incl = block_inclusive(flag, sh);
    if (flag) gt_rows[offsets[blockIdx.x] + (incl - 1)] = (int)r;      // offset + rank < the total <= rows
}

struct Pad {
    const long long *b_ids, *i_ids, *j_ids;
    const float *mconf, *mkpts_3d, *mkpts_c;
    const int* count;
    int cap;
    const int *gt_rows, *n_gt_total;
    const long long* gt_j;
    const float* keypoints3d;
    long long kp_bstride;
    int B, N, M, w_c, T, G;
    unsigned long long seed;
    int step;
    float scale;
    const float* query_scale;
    long long *out_b_ids, *out_i_ids, *out_j_ids;
    float *out_mconf, *out_mkpts_3d, *out_mkpts_c;
    unsigned char* out_gt_mask;
    int *out_count, *n_keep, *status;
};

__device__ __forceinline__ uint64_t draw(uint64_t seed, int step, int c, int s) {
    const uint64_t counter = (((uint64_t)step * 2ull + (uint64_t)c) << 32) | (uint64_t)(unsigned)s;
    return mix64(seed + 0x9E3779B97F4A7C15ull * (counter + 1ull));
}

__global__ __launch_bounds__(kThreads) void pad_kernel(Pad p) {
    const int s = blockIdx.x * kThreads + threadIdx.x;
    if (s >= p.T) return;
    const int P = clamped_count(p.count, p.cap);
    const int room = p.T - p.G;
    const int n_keep = P < room ? P : room;
    const int n_gt = clamped_count(p.n_gt_total, p.B * p.N);
    if (s == 0) {
        *p.out_count = n_gt == 0 ? 0 : p.T;
        *p.n_keep = n_keep;
        *p.status = n_gt == 0 ? OPTRN_NO_GT : OPTRN_OK;
    }
    if (n_gt == 0) return;
    long long b, i, j;
    float conf, x3[3], xc[2];
    if (s < n_keep) {
        const int src = P <= room ? s : (int)(draw(p.seed, p.step, 0, s) % (uint64_t)P);
        b = p.b_ids[src];
        i = p.i_ids[src];
        j = p.j_ids[src];
        conf = p.mconf[src];
        for (int a = 0; a < 3; ++a) x3[a] = p.mkpts_3d[3 * (long long)src + a];
        for (int a = 0; a < 2; ++a) xc[a] = p.mkpts_c[2 * (long long)src + a];
    } else {
        const int u = s - n_keep;
        int r = p.gt_rows[draw(p.seed, p.step, 1, u) % (uint64_t)n_gt];
        const int rows = p.B * p.N;
        r = r < 0 ? 0 : (r >= rows ? rows - 1 : r);         // entry 1 writes rows below B * N only: a table of another origin cannot index outside
        b = r / p.N;
        i = r % p.N;
        j = p.gt_j[r];
        conf = 0.0f;
        const float* x = p.keypoints3d + b * p.kp_bstride + 3 * i;
        for (int a = 0; a < 3; ++a) x3[a] = x[a];
        float sx = p.scale, sy = p.scale;
        if (p.query_scale != nullptr) {
            sx = p.scale * p.query_scale[2 * b + 1];
            sy = p.scale * p.query_scale[2 * b];
        }
        xc[0] = (float)(j % p.w_c) * sx;
        xc[1] = (float)(j / p.w_c) * sy;
    }
    p.out_b_ids[s] = b;
    p.out_i_ids[s] = i;
    p.out_j_ids[s] = j;
    p.out_mconf[s] = conf;
    for (int a = 0; a < 3; ++a) p.out_mkpts_3d[3 * (long long)s + a] = x3[a];
    for (int a = 0; a < 2; ++a) p.out_mkpts_c[2 * (long long)s + a] = xc[a];
    p.out_gt_mask[s] = conf == 0.0f ? 1 : 0;
}

const char* sizes_wrong(int B, int N, int M) {
    if (B < 1 || B > OPTRN_MAX_BATCH) return "B outside [1, OPTRN_MAX_BATCH]";
    if (N < 1 || N > OPTRN_MAX_ROWS || M < 1 || M > OPTRN_MAX_ROWS) return "N and M: in [1, OPTRN_MAX_ROWS]";
    if ((long long)B * N > OPTRN_MAX_ROWS) return "B * N above OPTRN_MAX_ROWS";
    return nullptr;
}

}  // namespace

extern "C" {

int optrn_abi_version(void) { return OPTRN_ABI_VERSION; }
const char* optrn_last_error(void) { return capi::g_error; }

size_t optrn_gt_list_bytes(int B, int N) {
    if (sizes_wrong(B, N, 1) != nullptr) return 0;
    return align_up((size_t)blocks_of((long long)B * N, kThreads) * sizeof(int));
}

int optrn_gt_list(const long long* gt_j, int B, int N, int M, void* workspace, size_t workspace_bytes, int* gt_rows, int* n_gt_total,
                  void* stream) {
    if (gt_j == nullptr || workspace == nullptr || gt_rows == nullptr || n_gt_total == nullptr) return bad_arg(__func__, "null pointer");
    if (const char* what = sizes_wrong(B, N, M)) return bad_arg(__func__, what);
    if (workspace_bytes < optrn_gt_list_bytes(B, N)) return bad_arg(__func__, "workspace smaller than optrn_gt_list_bytes(B, N)");
    const long long rows = (long long)B * N;
    const int blocks = (int)blocks_of(rows, kThreads);
    int* counts = (int*)workspace;
    gt_count_kernel<<<blocks, kThreads, 0, (hipStream_t)stream>>>(gt_j, rows, M, counts);
    CAPI_CHECK_LAUNCH();
    gt_offsets_kernel<<<1, kThreads, 0, (hipStream_t)stream>>>(counts, blocks, n_gt_total);
    CAPI_CHECK_LAUNCH();
    gt_scatter_kernel<<<blocks, kThreads, 0, (hipStream_t)stream>>>(gt_j, rows, M, counts, gt_rows);
    CAPI_CHECK_LAUNCH();
    return 0;
}

int optrn_pad_matches(const long long* b_ids, const long long* i_ids, const long long* j_ids, const float* mconf, const float* mkpts_3d,
                      const float* mkpts_c, const int* count, int cap, const int* gt_rows, const int* n_gt_total, const long long* gt_j,
                      const float* keypoints3d, long long kp_bstride, int B, int N, int M, int w_c, int T, int G,
                      unsigned long long seed, int step, float scale, const float* query_scale, long long* out_b_ids,
                      long long* out_i_ids, long long* out_j_ids, float* out_mconf, float* out_mkpts_3d, float* out_mkpts_c,
                      unsigned char* out_gt_mask, int* out_count, int* n_keep, int* status, void* stream) {
    if (b_ids == nullptr || i_ids == nullptr || j_ids == nullptr || mconf == nullptr || mkpts_3d == nullptr || mkpts_c == nullptr ||
        gt_rows == nullptr || n_gt_total == nullptr || gt_j == nullptr || keypoints3d == nullptr || out_b_ids == nullptr ||
        out_i_ids == nullptr || out_j_ids == nullptr || out_mconf == nullptr || out_mkpts_3d == nullptr || out_mkpts_c == nullptr ||
        out_gt_mask == nullptr || out_count == nullptr || n_keep == nullptr || status == nullptr)
        return bad_arg(__func__, "null pointer");
    if (const char* what = sizes_wrong(B, N, M)) return bad_arg(__func__, what);
    if (cap < 1 || cap > OPTRN_MAX_ROWS) return bad_arg(__func__, "cap outside [1, OPTRN_MAX_ROWS]");
    if (!(0 < G && G < T)) return bad_arg(__func__, "0 < G < T: min-num-gt-pad should be less than num-train-matches");
    if ((long long)T > (long long)B * N) return bad_arg(__func__, "T above B * N");
    if (w_c < 1) return bad_arg(__func__, "w_c: at least 1");
    if (step < 0 || step >= OPTRN_MAX_STEP) return bad_arg(__func__, "step outside [0, OPTRN_MAX_STEP)");
    if (kp_bstride != 0 && kp_bstride < 3LL * N) return bad_arg(__func__, "kp_bstride: 0 (shared) or at least 3 * N");
    const Pad p = {b_ids, i_ids, j_ids, mconf, mkpts_3d, mkpts_c, count, cap, gt_rows, n_gt_total, gt_j, keypoints3d, kp_bstride, B, N, M, w_c,
                   T, G, seed, step, scale, query_scale, out_b_ids, out_i_ids, out_j_ids, out_mconf, out_mkpts_3d, out_mkpts_c, out_gt_mask,
                   out_count, n_keep, status};
    pad_kernel<<<blocks_of(T, kThreads), kThreads, 0, (hipStream_t)stream>>>(p);
    CAPI_CHECK_LAUNCH();
    return 0;
}

}  // extern "C"
