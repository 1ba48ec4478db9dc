// One pixel of the query crop, written once: crop_resize_kernel (prep.hip, the box as launch arguments) and crop_box_kernel
// (track_crop.hip, the box read from device memory) must agree bit for bit, because a grey level that sits on .5 moves with one rounding.
//
// Why the fused form below is the contract.  crop_resize_kernel used to spell the interpolation as plain sums of products and was
// compiled with contraction on, so which product of each sum went into an FMA was the compiler's choice.  The same expressions under
// the same flags came out differently in track_crop.hip (there the box sides are loaded and known to be positive, in prep.hip they are
// opaque kernel arguments; read in the gfx950 ISA: u = mul + add unfused, then v fused the other way round).  So the fusion the
// compiler had chosen for crop_resize_kernel was read from its ISA and is now written out, with contraction off, for both kernels:
//     u = fma(0.5, wb, fma(-0.5, S, X) inv)     top    = fma(1 - a, p00, a p10)     val = fma(1 - b, top, b bottom)
//     v = fma(0.5, hb, fma(-0.5, S, Y) inv)     bottom = fma(1 - a, p01, a p11)
// (0.5 S is exact, so fma(-0.5, S, X) has the bits of X - 0.5 S, which is how track_crop.hip had spelt it; the fused spelling is the one
// in crop_resize_kernel's ISA).  A compiler that would fuse differently no longer changes a bit.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

// crop pixel (X, Y) of the S x S crop of box [x0, x0 + wb) x [y0, y0 + hb) of the H x W frame img, in [0, 1]: crop_img_by_bbox's two
// cv2.warpAffine calls (an integer-shift crop to the box, then an isotropic resize by S / wb about the crop centre, zero border) as one
// bilinear pass.  wb, hb > 0 and x0 + wb, y0 + hb do not overflow: the callers' guards
__device__ __forceinline__ float crop_pixel(const unsigned char* __restrict__ img, int H, int W, int x0, int y0, int wb, int hb, int S, int X,
                                            int Y) {
#pragma clang fp contract(off)
    const float inv = (float)wb / (float)S;                    // 1 / scale of the second warp
    const float u = fmaf(0.5f, (float)wb, fmaf(-0.5f, (float)S, (float)X) * inv);
    const float v = fmaf(0.5f, (float)hb, fmaf(-0.5f, (float)S, (float)Y) * inv);
    const float fu = floorf(u), fv = floorf(v);
    const int i0 = (int)fu, j0 = (int)fv;
    const float a = u - fu, b = v - fv;
    auto px = [&](int i, int j) -> float {                     // the box crop with zeros outside it and outside the frame
        if (i < 0 || i >= wb || j < 0 || j >= hb) return 0.f;
        const int x = x0 + i, y = y0 + j;                      // below x0 + wb, y0 + hb: no overflow
        return (x >= 0 && x < W && y >= 0 && y < H) ? (float)img[(size_t)y * W + x] : 0.f;
    };
    const float top = fmaf(1.f - a, px(i0, j0), a * px(i0 + 1, j0)), bottom = fmaf(1.f - a, px(i0, j0 + 1), a * px(i0 + 1, j0 + 1));
    const float val = fmaf(1.f - b, top, b * bottom);
    return fminf(fmaxf(rintf(val), 0.f), 255.f) / 255.0f;      // cv2 writes uint8; astype(float32) / 255 is a true division
}
