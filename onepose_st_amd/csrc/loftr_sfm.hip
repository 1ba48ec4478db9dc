// The SfM calls of the LoFTR matcher (src/KeypointFreeSfM/loftr_for_sfm/loftr.py:79-167): the fine-only branch's coarse ids from
// provided keypoints, and the backbone-feature sampler (loftr_for_sfm/utils/sample_feature_from_featuremap.py:6-80) behind
// extract_coarse_feature / extract_fine_feature.  Both are launch-bound: a few thousand keypoints, one row of 128 or 256 floats each.
//
// The arithmetic (sfm_sample.h, shared with sfm_fine.hip) is written in the reference's order of operations and rounding, in the
// keypoints' own dtype (COLMAP's float64 xys and the feature file's float32 keypoints can meet in one pair), with contraction into FMA
// switched off: the ids and the nearest samples are compared bit for bit.
#include "tile.h"
#include "onepose_hip.h"
#include <math.h>
#include <stdint.h>
#include "sfm_sample.h"

namespace {

// ---- coarse ids of provided matches ------------------------------------------------------------------------------------------------
struct IdsArgs {
    void* kp[2];                // [K][2] (x, y) in image pixels, clipped in place
    const float* scale[2];      // [1][2] (h factor, w factor) or NULL (1, 1)
    int xmax[2], ymax[2];       // hw_i[1] - 2, hw_i[0] - 2
    int wc[2];
    long long L[2];             // hc * wc
    long long* ids[2];          // i_ids, j_ids [K]
    float cscale;               // hw0_i[0] / hw0_c[0] (for both images, as the reference)
    int K;
    int* bad;                   // ids outside [0, L) (+ NaN keypoints)
};

template <typename T>
__device__ __forceinline__ void coarse_id(const IdsArgs& p, int img, int k) {
#pragma clang fp contract(off)
    T* kp = static_cast<T*>(p.kp[img]);
    const T x = sfmsample::clip(kp[2 * k], (T)p.xmax[img]), y = sfmsample::clip(kp[2 * k + 1], (T)p.ymax[img]);
    kp[2 * k] = x;
    kp[2 * k + 1] = y;
    const float* s = p.scale[img];
    const float sx = s ? p.cscale * s[1] : p.cscale, sy = s ? p.cscale * s[0] : p.cscale;
    const long long id = sfmsample::cell_id<T>(x, y, sx, sy, p.wc[img]);
    if (id < 0 || id >= p.L[img]) atomicAdd(p.bad, 1);
    p.ids[img][k] = id;
}

template <typename T0, typename T1>
__global__ __launch_bounds__(256) void sfm_coarse_ids_kernel(IdsArgs p) {
    const int t = blockIdx.x * 256 + threadIdx.x;
    if (t < p.K) coarse_id<T0>(p, 0, t);
    else if (t < 2 * p.K) coarse_id<T1>(p, 1, t - p.K);
}

// ---- feature sampling: F.grid_sample(map, normalised keypoints, align_corners=True, zero padding) ---------------------------------
struct SampleJob {
    const float* map;           // [h * w][C] channels-last
    const void* kpts;           // [K][2] (x, y) in image pixels, f32 or f64
    const float* scale;         // [2] (h factor, w factor): imghw = scale * (H, W)
    float* out;                 // [K][C]
    int h, w, C, K, H, W, kpt_double, nearest;
};

struct SampleJobs {
    SampleJob job[OPHIP_SAMPLE_MAX_JOBS];
    int n;
};

__global__ __launch_bounds__(256) void sfm_sample_kernel(SampleJobs jobs) {
#pragma clang fp contract(off)
    int g = blockIdx.x * 4 + (threadIdx.x >> 6);                    // one wave per keypoint
    const int lane = threadIdx.x & 63;
    int ji = 0;
    while (ji < jobs.n && g >= jobs.job[ji].K) g -= jobs.job[ji++].K;
    if (ji >= jobs.n) return;
    const SampleJob& j = jobs.job[ji];
    const int k = g;
    if (lane >= j.C / 4) return;
    const float eh = j.scale[0] * (float)j.H, ew = j.scale[1] * (float)j.W;       // imghw = scale * hw_i
    const char* kp = static_cast<const char*>(j.kpts) + (size_t)k * (j.kpt_double ? 16 : 8);
    const f32x4 o = sfmsample::sample_row(j.map, j.h, j.w, j.C, kp, j.kpt_double, eh, ew, j.nearest, lane);
    *reinterpret_cast<f32x4*>(j.out + (size_t)k * j.C + 4 * lane) = o;
}

}  // namespace

extern "C" int ophip_loftr_coarse_ids(void* mkpts0, int mk0_double, void* mkpts1, int mk1_double, int K, int h0i, int w0i, int h1i, int w1i,
                                      int h0c, int w0c, int h1c, int w1c, float coarse_scale, const float* scale0, const float* scale1,
                                      long long* i_ids, long long* j_ids, int* bad_count, void* stream_) {
    if (!bad_count || (K > 0 && (!mkpts0 || !mkpts1 || !i_ids || !j_ids))) return ophip_bad_arg(__func__, "null pointer");
    if ((scale0 == nullptr) != (scale1 == nullptr)) return ophip_bad_arg(__func__, "scale0 and scale1 come together");
    if (K < 0 || K > (1 << 29) || h0i < 2 || w0i < 2 || h1i < 2 || w1i < 2 || h0c < 1 || w0c < 1 || h1c < 1 || w1c < 1 || !(coarse_scale > 0.f))
        return ophip_bad_arg(__func__, "bad sizes");
    hipStream_t stream = (hipStream_t)stream_;
    hipError_t e = hipMemsetAsync(bad_count, 0, sizeof(int), stream);
    if (e != hipSuccess) return ophip_fail(e, __func__);
    if (K == 0) return 0;
    IdsArgs a{{mkpts0, mkpts1}, {scale0, scale1}, {w0i - 2, w1i - 2}, {h0i - 2, h1i - 2}, {w0c, w1c},
              {(long long)h0c * w0c, (long long)h1c * w1c}, {i_ids, j_ids}, coarse_scale, K, bad_count};
    const dim3 grid((2 * K + 255) / 256);
    if (mk0_double && mk1_double) OPHIP_LAUNCH("sfm_coarse_ids", stream, (sfm_coarse_ids_kernel<double, double>), grid, dim3(256), 0, stream, a);
    else if (mk0_double) OPHIP_LAUNCH("sfm_coarse_ids", stream, (sfm_coarse_ids_kernel<double, float>), grid, dim3(256), 0, stream, a);
    else if (mk1_double) OPHIP_LAUNCH("sfm_coarse_ids", stream, (sfm_coarse_ids_kernel<float, double>), grid, dim3(256), 0, stream, a);
    else OPHIP_LAUNCH("sfm_coarse_ids", stream, (sfm_coarse_ids_kernel<float, float>), grid, dim3(256), 0, stream, a);
    OPHIP_CHECK_LAUNCH();
    return 0;
}

extern "C" int ophip_sample_features(const ophip_sample_job* jobs, int n_jobs, void* stream_) {
    if (!jobs || n_jobs < 1 || n_jobs > OPHIP_SAMPLE_MAX_JOBS) return ophip_bad_arg(__func__, "1 to OPHIP_SAMPLE_MAX_JOBS jobs");
    SampleJobs a{};
    long long total = 0;
    for (int i = 0; i < n_jobs; ++i) {
        const ophip_sample_job& s = jobs[i];
        if (s.K < 0 || (s.C != 128 && s.C != 256) || s.h < 1 || s.w < 1 || s.H < 1 || s.W < 1) return ophip_bad_arg(__func__, "bad sizes (C 128 or 256)");
        if (s.K > 0 && (!s.map || !s.keypoints || !s.scale || !s.out)) return ophip_bad_arg(__func__, "null pointer");
        if (((uintptr_t)s.map | (uintptr_t)s.out) & 15) return ophip_bad_arg(__func__, "map and out must be 16-byte aligned");
        a.job[i] = SampleJob{s.map, s.keypoints, s.scale, s.out, s.h, s.w, s.C, s.K, s.H, s.W, s.keypoints_double ? 1 : 0, s.nearest ? 1 : 0};
        total += s.K;
    }
    a.n = n_jobs;
    if (total == 0) return 0;
    if (total > (1LL << 31) - 4) return ophip_bad_arg(__func__, "too many keypoints");
    hipStream_t stream = (hipStream_t)stream_;
    OPHIP_LAUNCH("sfm_sample", stream, sfm_sample_kernel, dim3((unsigned)((total + 3) / 4)), dim3(256), 0, stream, a);
    OPHIP_CHECK_LAUNCH();
    return 0;
}
