// The coarse context of the LoFTR matcher's fine windows (include/ext/onepose_fine_context.h): the published
// FinePreprocess with fine_concat_coarse_feat, between the window gather and the fine transformer.
//
//   win'[k][r] = merge_feat(cat[win[k][r], down_proj(coarse[b_k][id_k])])  =  Wm[:, :128] . win[k][r]  +  u_k,
//   u_k = Wm[:, 128:] . (Wd . coarse[b_k][id_k] + bd) + bm
//
// The context half of merge_feat is the same for the W * W rows of a match, so it is taken out of the row product: half the matrix work,
// and the repeated [K * W * W][128] context never exists.  Two kernels, both images in each:
//
//   context_kernel  64 (match, image) pairs per workgroup: the coarse rows gathered into split-bf16 planes, c = Wd x + bd into planes
//                   (feature-row accumulators, store_featrow_acc), u = Wm[:, 128:] c + bm to the scratch [2][K][128]
//   rows_kernel     64 window rows per workgroup (rows_linear_kernel<128, 128> of loftr_fine.hip with another epilogue): Wm[:, :128] x
//                   plus the u of THE ROW's match -- a tile is not match-aligned (at W = 5 it holds pieces of three or four matches)
//
// Every product is the split-bf16 MFMA of tile_bf16.h (hi + lo, lo . lo dropped, f32 accumulate).  In place (out == win) is safe:
// a workgroup reads its 64 rows into LDS before the barrier, writes the same 64 rows after it, and no other workgroup touches them.
#include "tile_bf16.h"
#include "capi_error.h"
#include "ext/onepose_fine_context.h"

using capi::bad_arg;
using capi::g_error;

namespace {

constexpr int CF = 128, CC = 256, ROWS = OPFCX_TILE_ROWS;
constexpr size_t FRAGS_D = (size_t)CF * CC / 8, FRAGS_M = (size_t)CF * CF / 8;      // bf16x8 fragments of Wd and of each half of Wm

struct Weights {
    const bf16x8 *d_hi, *d_lo;      // Wd [128][256]
    const bf16x8 *w_hi, *w_lo;      // Wm[:, :128] (the window half)
    const bf16x8 *c_hi, *c_lo;      // Wm[:, 128:] (the context half)
    const float *bd, *bm;
};

struct ContextArgs {
    const float* coarse[2];         // [B][L][256]
    long long bstride[2];
    const long long* b_ids;
    const long long* ids[2];        // i_ids, j_ids
    int K, B, L[2];
    Weights w;
    float* u;                       // [2][K][128]
};

__global__ __launch_bounds__(256) OPHIP_WAVES_PER_SIMD(1, 2) void context_kernel(ContextArgs p) {
    // X planes [64][256] bf16 (hi, lo): 2 x 32 KiB; after the first product the c planes [64][128] (2 x 16 KiB) take the first half
    __shared__ __attribute__((aligned(16))) char smem[2 * ROWS * CC * 2];
    constexpr int XB = CC * 2, CB = CF * 2;
    char* XH = smem;
    char* XL = smem + ROWS * XB;
    char* CH = smem;
    char* CL = smem + ROWS * CB;
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const long long row0 = (long long)blockIdx.x * ROWS, total = 2LL * p.K;
    for (int i = tid; i < ROWS * (CC / 8); i += 256) {
        const int row = i / (CC / 8), ch = i % (CC / 8);
        const long long g = row0 + row;
        f32x4 v0 = {0.f, 0.f, 0.f, 0.f}, v1 = v0;
        if (g < total) {
            const int s = g >= p.K;
            const long long k = g - (s ? p.K : 0);
            const long long b = p.b_ids[k], id = p.ids[s][k];
            if (b >= 0 && b < p.B && id >= 0 && id < p.L[s]) {          // an id outside the tables reads a zero row
                const float* src = p.coarse[s] + (size_t)b * p.bstride[s] + (size_t)id * CC + 8 * ch;
                v0 = *reinterpret_cast<const f32x4*>(src);
                v1 = *reinterpret_cast<const f32x4*>(src + 4);
            }
        }
        bf16x8 vh, vl;
#pragma unroll
        for (int j = 0; j < 4; ++j) {
            __bf16 hh, ll;
            split_bf16(v0[j], hh, ll); vh[j] = hh; vl[j] = ll;
            split_bf16(v1[j], hh, ll); vh[4 + j] = hh; vl[4 + j] = ll;
        }
        const int off = plane_off(row, ch, XB);
        *reinterpret_cast<bf16x8*>(XH + off) = vh;
        *reinterpret_cast<bf16x8*>(XL + off) = vl;
    }
    __syncthreads();
    const int r = lane & 31, h = lane >> 5;
    // c = Wd x + bd: wave w owns features 32 w .. 32 w + 31 of both 32-row tiles, as D[feature row][token col]
    f32x16 acc[1][2];
    acc[0][0] = zero16(); acc[0][1] = zero16();
    constexpr int TSD = (CC / 16) * 64, TSM = (CF / 16) * 64;
    gemm_bf16<1, 2, 3, true, CC / 16, 2>(acc, p.w.d_hi + (size_t)wave * TSD + lane, p.w.d_lo + (size_t)wave * TSD + lane, 4 * TSD, XH, XL, XB, 0, lane);
#pragma unroll
    for (int reg = 0; reg < 16; ++reg) {
        const float bias = p.w.bd[32 * wave + 8 * (reg >> 2) + 4 * h + (reg & 3)];
        acc[0][0][reg] += bias;
        acc[0][1][reg] += bias;
    }
    __syncthreads();                                                     // every wave has read the X planes
    store_featrow_acc<3>(acc[0][0], CH, CL, CB, 32 * wave, 0, lane);
    store_featrow_acc<3>(acc[0][1], CH, CL, CB, 32 * wave, 32, lane);
    __syncthreads();
    // u = Wm[:, 128:] c + bm, as D[token row][feature col]
    acc[0][0] = zero16(); acc[0][1] = zero16();
    gemm_bf16<1, 2, 3, false, CF / 16, 2>(acc, p.w.c_hi + (size_t)wave * TSM + lane, p.w.c_lo + (size_t)wave * TSM + lane, 4 * TSM, CH, CL, CB, 0, lane);
    const int col = 32 * wave + r;
    const float bias = p.w.bm[col];
#pragma unroll
    for (int tt = 0; tt < 2; ++tt)
#pragma unroll
        for (int reg = 0; reg < 16; ++reg) {
            const long long g = row0 + 32 * tt + acc_row(reg, h);
            if (g < total) p.u[(size_t)g * CF + col] = acc[0][tt][reg] + bias;
        }
}

struct RowsArgs {
    const float* win[2];            // [K][WW][128]
    float* out[2];
    const float* u;                 // [2][K][128]
    long long T;                    // K * WW rows per image
    int K, WW, tiles;               // tiles per image
    unsigned inv_ww;                // ceil(2^16 / WW): n / WW == (n * inv_ww) >> 16 for n < 64 + WW <= 185
    Weights w;
};

__global__ __launch_bounds__(256) OPHIP_WAVES_PER_SIMD(1, 2) void rows_kernel(RowsArgs p) {
    __shared__ __attribute__((aligned(16))) char smem[2 * ROWS * CF * 2];
    constexpr int ROWB = CF * 2;
    char* XH = smem;
    char* XL = smem + ROWS * ROWB;
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const int s = (int)blockIdx.x >= p.tiles;
    const long long tok0 = (long long)((int)blockIdx.x - (s ? p.tiles : 0)) * ROWS;
    const int live = (int)(p.T - tok0 < ROWS ? p.T - tok0 : ROWS);
    load_rows_to_planes<3, CF, ROWS>(XH, XL, p.win[s] + (size_t)tok0 * CF, 0, live, tid, 256);
    __syncthreads();
    f32x16 acc[1][2];
    acc[0][0] = zero16(); acc[0][1] = zero16();
    constexpr int TS = (CF / 16) * 64;
    gemm_bf16<1, 2, 3, false, CF / 16, 2>(acc, p.w.w_hi + (size_t)wave * TS + lane, p.w.w_lo + (size_t)wave * TS + lane, 4 * TS, XH, XL, ROWB, 0, lane);
    // the context is looked up per ROW: match of row tok0 + n is k0 + (first + n) / WW with first = tok0 % WW
    const int r = lane & 31, h = lane >> 5, col = 32 * wave + r;
    const long long k0 = tok0 / p.WW;
    const int first = (int)(tok0 - k0 * p.WW);
    const float* u = p.u + ((size_t)s * p.K + (size_t)k0) * CF + col;
    float* out = p.out[s] + (size_t)tok0 * CF + col;
#pragma unroll
    for (int tt = 0; tt < 2; ++tt)
#pragma unroll
        for (int reg = 0; reg < 16; ++reg) {
            const int n = 32 * tt + acc_row(reg, h);
            if (n < live) {
                const unsigned dk = ((unsigned)(first + n) * p.inv_ww) >> 16;
                out[(size_t)n * CF] = acc[0][tt][reg] + u[(size_t)dk * CF];
            }
        }
}

bool misaligned(const void* a) { return ((uintptr_t)a & 15) != 0; }

}  // namespace

extern "C" int opfcx_abi_version(void) { return OPFCX_ABI_VERSION; }

extern "C" const char* opfcx_last_error(void) { return g_error; }

extern "C" size_t opfcx_wpack_bytes(void) { return 2 * 2 * 8 * (FRAGS_D + 2 * FRAGS_M) + 2 * CF * sizeof(float); }

extern "C" size_t opfcx_context_floats(int K) { return K > 0 ? (size_t)2 * K * CF : 0; }

extern "C" int opfcx_merge(const float* win0, const float* win1, const float* coarse0, long long coarse0_bstride, const float* coarse1,
                           long long coarse1_bstride, const long long* b_ids, const long long* i_ids, const long long* j_ids, int K, int B,
                           int L0, int L1, int W, const void* wpack, float* context, float* out0, float* out1, void* stream_) {
    if (!win0 || !win1 || !coarse0 || !coarse1 || !b_ids || !i_ids || !j_ids || !wpack || !context || !out0 || !out1)
        return bad_arg(__func__, "null pointer");
    if (K < 0 || B < 1 || L0 < 1 || L1 < 1) return bad_arg(__func__, "bad sizes (K >= 0, B >= 1, L0 >= 1, L1 >= 1)");
    if (W < 3 || W > 11 || (W & 1) == 0) return bad_arg(__func__, "window: odd, from 3 to 11");
    const int WW = W * W;
    const long long T = (long long)K * WW;
    if (T > OPFCX_MAX_ROWS) return bad_arg(__func__, "K * W * W exceeds OPFCX_MAX_ROWS");
    if (misaligned(win0) || misaligned(win1) || misaligned(coarse0) || misaligned(coarse1) || misaligned(wpack) || misaligned(context) ||
        misaligned(out0) || misaligned(out1))
        return bad_arg(__func__, "pointers must be 16-byte aligned");
    if (coarse0_bstride < 0 || coarse1_bstride < 0 || ((coarse0_bstride | coarse1_bstride) & 3) ||
        (coarse0_bstride > 0 && coarse0_bstride < (long long)L0 * CC) || (coarse1_bstride > 0 && coarse1_bstride < (long long)L1 * CC))
        return bad_arg(__func__, "image strides: 0, or a multiple of 4 floats that holds L * 256");
    if (K == 0) return 0;
    const bf16x8* hi = reinterpret_cast<const bf16x8*>(wpack);
    const bf16x8* lo = hi + FRAGS_D + 2 * FRAGS_M;
    const float* bias = reinterpret_cast<const float*>(lo + FRAGS_D + 2 * FRAGS_M);
    const Weights w{hi, lo, hi + FRAGS_D, lo + FRAGS_D, hi + FRAGS_D + FRAGS_M, lo + FRAGS_D + FRAGS_M, bias, bias + CF};
    hipStream_t stream = (hipStream_t)stream_;
    ContextArgs c{{coarse0, coarse1}, {coarse0_bstride, coarse1_bstride}, b_ids, {i_ids, j_ids}, K, B, {L0, L1}, w, context};
    hipLaunchKernelGGL(context_kernel, dim3(capi::blocks_of(2LL * K, ROWS)), dim3(256), 0, stream, c);
    CAPI_CHECK_LAUNCH();
    const int tiles = (int)capi::blocks_of(T, ROWS);
    RowsArgs a{{win0, win1}, {out0, out1}, context, T, K, WW, tiles, (65536u + WW - 1) / WW, w};
    hipLaunchKernelGGL(rows_kernel, dim3(2u * tiles), dim3(256), 0, stream, a);
    CAPI_CHECK_LAUNCH();
    return 0;
}
