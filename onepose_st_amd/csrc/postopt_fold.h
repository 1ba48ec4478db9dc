// The float64 row fold of the SfM depth refinement, shared by the first-order solver (postopt.hip, libonepose_hip.so) and the
// Levenberg-Marquardt solver (postopt_lm.hip, libonepose_postopt_lm.so): the 3x3 helpers, pytorch3d's so3 maps, AngleAxisRotatePoint
// and fold_row, which turns one residual row into h(d) = d * a + b.  One copy; every expression is evaluated in the written order.
#pragma once
#include <hip/hip_runtime.h>
#include <math.h>

namespace {

constexpr int kRow = 8;                      // doubles per folded row: a0 a1 a2 b0 b1 (b2 + 1e-4) f0 f1

// so3_log_map's acos_linear_extrapolation at the bounds +-(1 - 1e-4): (x - x0) * (-1 / sqrt(1 - x0^2)) + acos(x0), the two constants as
// Python's math module computes them
constexpr double kCosBound = 0.9999;
constexpr double kDacosAtBound = -70.71244595191452;
constexpr double kAcosHi = 0.014142253477512098;
constexpr double kAcosLo = 3.127450400112281;

__device__ __forceinline__ void mat3_mul(const double* A, const double* B, double* C) {
#pragma clang fp contract(off)
    for (int i = 0; i < 3; ++i)
        for (int j = 0; j < 3; ++j) C[3 * i + j] = A[3 * i] * B[j] + A[3 * i + 1] * B[3 + j] + A[3 * i + 2] * B[6 + j];
}

__device__ __forceinline__ void mat3_vec(const double* A, const double* x, double* y) {
#pragma clang fp contract(off)
    for (int i = 0; i < 3; ++i) y[i] = A[3 * i] * x[0] + A[3 * i + 1] * x[1] + A[3 * i + 2] * x[2];
}

// general 3x3 inverse (torch.inverse / np.linalg.inv semantics, adjugate over the determinant)
__device__ __forceinline__ void inv3(const double* m, double* o) {
#pragma clang fp contract(off)
    const double c00 = m[4] * m[8] - m[5] * m[7], c01 = m[5] * m[6] - m[3] * m[8], c02 = m[3] * m[7] - m[4] * m[6];
    const double det = m[0] * c00 + m[1] * c01 + m[2] * c02;
    const double r = 1.0 / det;
    o[0] = c00 * r; o[1] = (m[2] * m[7] - m[1] * m[8]) * r; o[2] = (m[1] * m[5] - m[2] * m[4]) * r;
    o[3] = c01 * r; o[4] = (m[0] * m[8] - m[2] * m[6]) * r; o[5] = (m[2] * m[3] - m[0] * m[5]) * r;
    o[6] = c02 * r; o[7] = (m[1] * m[6] - m[0] * m[7]) * r; o[8] = (m[0] * m[4] - m[1] * m[3]) * r;
}

// pytorch3d so3_exp_map(eps = 1e-4): theta = sqrt(max(|w|^2, eps)), R = I + sin(theta) / theta * hat(w) + (1 - cos theta) / theta^2 * hat(w)^2
__device__ void so3_exp(const double* w, double* R) {
#pragma clang fp contract(off)
    const double nrm = w[0] * w[0] + w[1] * w[1] + w[2] * w[2];
    const double th = sqrt(nrm < 1e-4 ? 1e-4 : nrm);
    const double inv = 1.0 / th;
    const double f1 = inv * sin(th), f2 = inv * inv * (1.0 - cos(th));
    const double K[9] = {0.0, -w[2], w[1], w[2], 0.0, -w[0], -w[1], w[0], 0.0};
    double K2[9];
    mat3_mul(K, K, K2);
    for (int i = 0; i < 9; ++i) R[i] = f1 * K[i] + f2 * K2[i] + ((i % 4 == 0) ? 1.0 : 0.0);
}

// pytorch3d so3_log_map(eps = 1e-4, cos_bound = 1e-4): phi = acos of the trace's cosine, linearly extrapolated outside +-(1 - 1e-4);
// phi / (2 sin phi), or 0.5 + phi^2 / 12 where |sin phi| <= 0.5e-4; hat_inv of that factor times (R - R^T)
__device__ void so3_log(const double* R, double* w) {
#pragma clang fp contract(off)
    const double c = ((R[0] + R[4] + R[8]) - 1.0) * 0.5;
    double phi;
    if (c >= kCosBound) phi = (c - kCosBound) * kDacosAtBound + kAcosHi;
    else if (c <= -kCosBound) phi = (c - -kCosBound) * kDacosAtBound + kAcosLo;
    else phi = acos(c);
    const double s = sin(phi);
    const double f = fabs(s) > 0.5 * 1e-4 ? phi / (2.0 * s) : 0.5 + (phi * phi) * (1.0 / 12);
    w[0] = f * (R[7] - R[5]);
    w[1] = f * (R[2] - R[6]);
    w[2] = f * (R[3] - R[1]);
}

// AngleAxisRotatePoint (residual_utils.py:3-52): Rodrigues, or p + w x p where |w|^2 == 0
__device__ void aa_rotate(const double* w, const double* p, double* o) {
#pragma clang fp contract(off)
    const double t2 = w[0] * w[0] + w[1] * w[1] + w[2] * w[2];
    if (t2 > 0.0) {
        const double th = sqrt(t2), ct = cos(th), st = sin(th), ti = 1.0 / th;
        const double w0 = w[0] * ti, w1 = w[1] * ti, w2 = w[2] * ti;
        const double x0 = w1 * p[2] - w2 * p[1], x1 = w2 * p[0] - w0 * p[2], x2 = w0 * p[1] - w1 * p[0];
        const double tmp = (w0 * p[0] + w1 * p[1] + w2 * p[2]) * (1.0 - ct);
        o[0] = p[0] * ct + x0 * st + w0 * tmp;
        o[1] = p[1] * ct + x1 * st + w1 * tmp;
        o[2] = p[2] * ct + x2 * st + w2 * tmp;
    } else {
        o[0] = p[0] + (w[1] * p[2] - w[2] * p[1]);
        o[1] = p[1] + (w[2] * p[0] - w[0] * p[2]);
        o[2] = p[2] + (w[0] * p[1] - w[1] * p[0]);
    }
}

struct FoldInputs {
    const double *K0, *K1, *mk0, *mk1f, *aa;   // [L][9], [L][9], [L][2], [L][2], [F][6]
    const long long *left, *right;              // [L] frame indices
    int F;
};

// Row r folded into out[kRow]: unprojection by K0^-1, pose0^-1 through so3_exp / inverse / so3_log, the two rotations and K1 are linear
// in the depth d, so the homogeneous projection into frame 1 is h(d) = d * out[0:3] + out[3:6] (out[5] carries the reference's + 1e-4);
// out[6:8] = mkpts1_f.
__device__ __forceinline__ void fold_row(const FoldInputs& p, long long r, double* out) {
#pragma clang fp contract(off)
    const long long i0 = p.left[r], i1 = p.right[r];
    if (i0 < 0 || i0 >= p.F || i1 < 0 || i1 >= p.F) {             // the host validates; a bad index poisons its row, never reads past
        for (int k = 0; k < kRow; ++k) out[k] = __builtin_nan("");
        return;
    }
    double K0[9], Ki[9], K1[9];
    for (int k = 0; k < 9; ++k) { K0[k] = p.K0[r * 9 + k]; K1[k] = p.K1[r * 9 + k]; }
    inv3(K0, Ki);
    const double uv1[3] = {p.mk0[2 * r], p.mk0[2 * r + 1], 1.0};
    double ray[3];
    mat3_vec(Ki, uv1, ray);                                        // K0^-1 [u, v, 1]: the camera-0 point per unit depth
    // pose0^-1 as the reference builds it: R^-1 = inverse(so3_exp_map(w0)), t^-1 = -R^-1 t0, back to angle-axis by so3_log_map
    const double* a0 = p.aa + 6 * i0;
    const double* a1 = p.aa + 6 * i1;
    double R0[9], Ri[9], wi[3], ti[3];
    so3_exp(a0, R0);
    inv3(R0, Ri);
    mat3_vec(Ri, a0 + 3, ti);
    for (int k = 0; k < 3; ++k) ti[k] = -1.0 * ti[k];
    so3_log(Ri, wi);
    // world = rot(w^-1, d * ray) + t^-1, camera 1 = rot(w1, world) + t1: linear in d
    double aw[3], ac[3], bc[3], a[3], b[3];
    aa_rotate(wi, ray, aw);
    aa_rotate(a1, aw, ac);
    aa_rotate(a1, ti, bc);
    for (int k = 0; k < 3; ++k) bc[k] = bc[k] + a1[3 + k];
    mat3_vec(K1, ac, a);
    mat3_vec(K1, bc, b);
    out[0] = a[0]; out[1] = a[1]; out[2] = a[2];
    out[3] = b[0]; out[4] = b[1]; out[5] = b[2] + 1e-4;
    out[6] = p.mk1f[2 * r]; out[7] = p.mk1f[2 * r + 1];
}

}  // namespace
