// The fine half of the SfM matcher over a whole pair list (include/onepose_sfm_fine.h): the per-row forms of the
// two kernels of csrc/loftr_sfm.hip.  There one call serves one image pair, so the image sizes, the scales and the maps are launch
// arguments; here every pair row names its two images and the kernels look sizes, scales and maps up in device tables, so that one
// launch serves the rows of many pairs.
//
//   row_ids      ophip_loftr_coarse_ids per row: clip into a copy, divide by 8 * scale[[1, 0]], round half to even, cell id; ids outside
//                the grid are counted and the smallest offending row is kept (integer atomics: the result does not depend on the order)
//   sample_rows  ophip_sample_features per row: the four feature tables of a bucket of rows in one launch, one wave per row and table,
//                16-byte loads of the map rows, f32 rows out
//
// The ids and the samples come from the functions of sfm_sample.h, which the per-pair kernels call too, so the two agree bit for bit
// by construction.  Both kernels are memory- and launch-bound.
#include <hip/hip_runtime.h>
#include <math.h>
#include <stdint.h>
#include "onepose_sfm_fine.h"
#include "capi_error.h"
#include "sfm_sample.h"

using capi::bad_arg;
using capi::fail;
using capi::g_error;

namespace {

using sfmsample::f32x4;

// ---- cell ids of the rows' keypoints -------------------------------------------------------------------------------------------------
struct IdsArgs {
    const void* kp[2];          // [M][2] (x, y) in image pixels: read only
    void* out[2];               // [M][2] the clipped copies
    const long long* image[2];  // [M] row_left, row_right
    const int* hw;              // [I][2] (H, W)
    const float* scale;         // [I][2] (h factor, w factor)
    long long* ids[2];          // i_ids, j_ids [M]
    int* ctrl;                  // bad ids, smallest bad row
    long long M;
    int I;
    float cscale;               // 8: image rows per coarse row
};

template <typename T>
__device__ __forceinline__ void row_id(const IdsArgs& p, int side, long long r) {
#pragma clang fp contract(off)
    const T* kp = static_cast<const T*>(p.kp[side]);
    T* out = static_cast<T*>(p.out[side]);
    T x = kp[2 * r], y = kp[2 * r + 1];
    const long long img = p.image[side][r];
    long long id = -1, L = 0;
    if (img >= 0 && img < p.I) {
        const int H = p.hw[2 * img], W = p.hw[2 * img + 1];
        x = sfmsample::clip(x, (T)(W - 2));
        y = sfmsample::clip(y, (T)(H - 2));
        const float* s = p.scale + 2 * img;
        const int wc = W / 8;
        id = sfmsample::cell_id<T>(x, y, p.cscale * s[1], p.cscale * s[0], wc);
        L = (long long)(H / 8) * wc;
    }
    out[2 * r] = x;
    out[2 * r + 1] = y;
    if (id < 0 || id >= L) {
        atomicAdd(p.ctrl, 1);
        atomicMin(p.ctrl + 1, (int)r);
    }
    p.ids[side][r] = id;
}

template <typename T0, typename T1>
__global__ __launch_bounds__(256) void row_ids_kernel(IdsArgs p) {
    const long long t = (long long)blockIdx.x * 256 + threadIdx.x;
    if (t < p.M) row_id<T0>(p, 0, t);
    else if (t < 2 * p.M) row_id<T1>(p, 1, t - p.M);
}

__global__ void init_ctrl_kernel(int* ctrl) {
    if (threadIdx.x == 0) {
        ctrl[0] = 0;
        ctrl[1] = OPSFF_NO_ROW;
    }
}

// ---- feature sampling: F.grid_sample(map, normalised keypoints, align_corners=True, zero padding) per row ---------------------------
struct SideArgs {
    const float* coarse;        // [n_group][(H / 8) * (W / 8)][256]
    const float* fine;          // [n_group][(H / 2) * (W / 2)][128]
    long long coarse_bs, fine_bs;
    const void* kpts;           // [M][2]
    const long long* image;     // [M]
    float* out_c;               // [M][256]
    float* out_f;               // [M][128]
    int n_group, H, W, kpt_double;
};

struct SampleArgs {
    SideArgs side[2];
    const long long* image_index;   // [I] index within the group
    const float* scale;             // [I][2]
    const long long* rows;          // [n] or NULL
    long long row0, M;
    int n, I;
};

__global__ __launch_bounds__(256) void sample_rows_kernel(SampleArgs a) {
#pragma clang fp contract(off)
    const long long g = (long long)blockIdx.x * 4 + (threadIdx.x >> 6);      // one wave per (table, row)
    const int lane = threadIdx.x & 63;
    if (g >= 4LL * a.n) return;
    const int table = (int)(g / a.n), k = (int)(g % a.n);                    // coarse left, coarse right, fine left, fine right
    const SideArgs& s = a.side[table & 1];
    const int nearest = table < 2;
    const int C = nearest ? 256 : 128;
    if (lane >= C / 4) return;
    const long long r = a.rows ? a.rows[k] : a.row0 + k;
    if (r < 0 || r >= a.M) return;
    float* out = (nearest ? s.out_c : s.out_f) + (size_t)r * C + 4 * lane;
    f32x4 o = {0.f, 0.f, 0.f, 0.f};
    const long long img = s.image[r];
    const long long b = (img >= 0 && img < a.I) ? a.image_index[img] : -1;
    if (b < 0 || b >= s.n_group) {                                           // a row of another bucket: nothing of it is read
        *reinterpret_cast<f32x4*>(out) = o;
        return;
    }
    const int h = nearest ? s.H / 8 : s.H / 2, w = nearest ? s.W / 8 : s.W / 2;
    const float* map = nearest ? s.coarse + (size_t)b * s.coarse_bs : s.fine + (size_t)b * s.fine_bs;
    const float* sc = a.scale + 2 * img;
    const float eh = sc[0] * (float)s.H, ew = sc[1] * (float)s.W;           // imghw = scale * hw_i
    const char* kp = static_cast<const char*>(s.kpts) + (size_t)r * (s.kpt_double ? 16 : 8);
    o = sfmsample::sample_row(map, h, w, C, kp, s.kpt_double, eh, ew, nearest, lane);
    *reinterpret_cast<f32x4*>(out) = o;
}

}  // namespace

extern "C" int opsff_abi_version(void) { return OPSFF_ABI_VERSION; }

extern "C" const char* opsff_last_error(void) { return g_error; }

extern "C" int opsff_row_ids(const void* mkpts0, int mk0_double, const void* mkpts1, int mk1_double, const long long* row_left,
                             const long long* row_right, const int* image_hw, const float* image_scale, int I, long long M,
                             float coarse_scale, void* mkpts0_out, void* mkpts1_out, long long* i_ids, long long* j_ids, int* ctrl,
                             void* stream_) {
    if (!ctrl) return bad_arg(__func__, "null pointer");
    if (M < 0 || M > OPSFF_MAX_ROWS || I < 1 || !(coarse_scale > 0.f)) return bad_arg(__func__, "bad sizes");
    if (M > 0 && (!mkpts0 || !mkpts1 || !row_left || !row_right || !image_hw || !image_scale || !mkpts0_out || !mkpts1_out || !i_ids || !j_ids))
        return bad_arg(__func__, "null pointer");
    hipStream_t stream = (hipStream_t)stream_;
    hipLaunchKernelGGL(init_ctrl_kernel, dim3(1), dim3(64), 0, stream, ctrl);
    CAPI_CHECK_LAUNCH();
    if (M == 0) return 0;
    IdsArgs a{{mkpts0, mkpts1}, {mkpts0_out, mkpts1_out}, {row_left, row_right}, image_hw, image_scale, {i_ids, j_ids}, ctrl, M, I, coarse_scale};
    const dim3 grid((unsigned)((2 * M + 255) / 256));
    if (mk0_double && mk1_double) hipLaunchKernelGGL((row_ids_kernel<double, double>), grid, dim3(256), 0, stream, a);
    else if (mk0_double) hipLaunchKernelGGL((row_ids_kernel<double, float>), grid, dim3(256), 0, stream, a);
    else if (mk1_double) hipLaunchKernelGGL((row_ids_kernel<float, double>), grid, dim3(256), 0, stream, a);
    else hipLaunchKernelGGL((row_ids_kernel<float, float>), grid, dim3(256), 0, stream, a);
    CAPI_CHECK_LAUNCH();
    return 0;
}

extern "C" int opsff_sample_rows(const float* coarse0, long long coarse0_bstride, const float* fine0, long long fine0_bstride, int n_group0,
                                 int H0, int W0, const float* coarse1, long long coarse1_bstride, const float* fine1, long long fine1_bstride,
                                 int n_group1, int H1, int W1, const void* mkpts0, int mk0_double, const void* mkpts1, int mk1_double,
                                 const long long* row_left, const long long* row_right, const long long* image_index,
                                 const float* image_scale, int I, const long long* rows, long long row0, int n, long long M,
                                 float* feature_c0, float* feature_c1, float* feature0, float* feature1, void* stream_) {
    if (n < 0 || n > (1 << 28) || M < 0 || M > OPSFF_MAX_ROWS || I < 1 || n_group0 < 1 || n_group1 < 1) return bad_arg(__func__, "bad sizes");
    if (H0 < 8 || W0 < 8 || H1 < 8 || W1 < 8 || H0 % 8 || W0 % 8 || H1 % 8 || W1 % 8) return bad_arg(__func__, "image sizes: multiples of 8");
    if (!rows && (row0 < 0 || row0 + n > M)) return bad_arg(__func__, "rows outside the tables");
    if (n == 0) return 0;
    if (!coarse0 || !fine0 || !coarse1 || !fine1 || !mkpts0 || !mkpts1 || !row_left || !row_right || !image_index || !image_scale ||
        !feature_c0 || !feature_c1 || !feature0 || !feature1)
        return bad_arg(__func__, "null pointer");
    if (((uintptr_t)coarse0 | (uintptr_t)fine0 | (uintptr_t)coarse1 | (uintptr_t)fine1 | (uintptr_t)feature_c0 | (uintptr_t)feature_c1 |
         (uintptr_t)feature0 | (uintptr_t)feature1) & 15)
        return bad_arg(__func__, "maps and outputs must be 16-byte aligned");
    if ((coarse0_bstride | fine0_bstride | coarse1_bstride | fine1_bstride) & 3) return bad_arg(__func__, "image strides: multiples of 4 floats");
    if ((n_group0 > 1 && (coarse0_bstride < (long long)(H0 / 8) * (W0 / 8) * 256 || fine0_bstride < (long long)(H0 / 2) * (W0 / 2) * 128)) ||
        (n_group1 > 1 && (coarse1_bstride < (long long)(H1 / 8) * (W1 / 8) * 256 || fine1_bstride < (long long)(H1 / 2) * (W1 / 2) * 128)))
        return bad_arg(__func__, "image strides smaller than a map");
    SampleArgs a{};
    a.side[0] = SideArgs{coarse0, fine0, coarse0_bstride, fine0_bstride, mkpts0, row_left, feature_c0, feature0, n_group0, H0, W0, mk0_double ? 1 : 0};
    a.side[1] = SideArgs{coarse1, fine1, coarse1_bstride, fine1_bstride, mkpts1, row_right, feature_c1, feature1, n_group1, H1, W1, mk1_double ? 1 : 0};
    a.image_index = image_index;
    a.scale = image_scale;
    a.rows = rows;
    a.row0 = row0;
    a.M = M;
    a.n = n;
    a.I = I;
    hipStream_t stream = (hipStream_t)stream_;
    hipLaunchKernelGGL(sample_rows_kernel, dim3((unsigned)n), dim3(256), 0, stream, a);      // 4 n waves, 4 per workgroup
    CAPI_CHECK_LAUNCH();
    return 0;
}
