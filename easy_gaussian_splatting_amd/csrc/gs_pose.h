// gs_pose.h -- the pose correction of pose.CameraDeltas for the captured step (gs_pose.hip; DESIGN.md "Poses in the captured step"):
// the corrected view matrix [[exp([omega]x), tau], [0, 1]] @ w2c and the chain from the view matrix' gradient back to the 6-vector.
// Plain C++ in fp64 that compiles for the device and for the host alike: tests/test_pose_host.py builds it with the host compiler
// (tests/hostmath/posemath.cpp) and holds it to torch's float64 matrix_exp and autograd.
#pragma once
#include <math.h>
#include <stdint.h>

#ifdef __HIPCC__
#define GS_HD __host__ __device__ __forceinline__
#else
#define GS_HD static inline
#endif

namespace gs {

// Below this theta^2 the three coefficients come from their series (through theta^10: the first term left out is below 1e-22
// there); above it from the closed forms, none of which cancels any more: (1 - cos) is written 2 sin^2(theta / 2), and
// theta - sin(theta) has lost under four digits at theta = 0.1.
constexpr double kPoseSeriesTheta2 = 1e-2;

// sin(theta) / theta, (1 - cos(theta)) / theta^2, (theta - sin(theta)) / theta^3 from t2 = theta^2: smooth through theta = 0
GS_HD void pose_coeffs(double t2, double& A, double& B, double& C) {
    if (t2 < kPoseSeriesTheta2) {
        A = 1.0 + t2 * (-1.0 / 6.0 + t2 * (1.0 / 120.0 + t2 * (-1.0 / 5040.0 + t2 * (1.0 / 362880.0 + t2 * (-1.0 / 39916800.0)))));
        B = 0.5 + t2 * (-1.0 / 24.0 + t2 * (1.0 / 720.0 + t2 * (-1.0 / 40320.0 + t2 * (1.0 / 3628800.0 + t2 * (-1.0 / 479001600.0)))));
        C = 1.0 / 6.0 + t2 * (-1.0 / 120.0 + t2 * (1.0 / 5040.0 + t2 * (-1.0 / 362880.0 + t2 * (1.0 / 39916800.0 + t2 * (-1.0 / 6227020800.0)))));
    } else {
        const double th = sqrt(t2), s = sin(th), h = sin(0.5 * th);
        A = s / th;
        B = 2.0 * h * h / t2;
        C = (th - s) / (t2 * th);
    }
}

// R = exp([w]x) = I + A [w]x + B [w]x^2 (Rodrigues; [w]x^2 = w w^T - theta^2 I), row-major
GS_HD void pose_rotation(const double w[3], double R[9]) {
    const double t2 = w[0] * w[0] + w[1] * w[1] + w[2] * w[2];
    double A, B, C;
    pose_coeffs(t2, A, B, C);
    R[0] = 1.0 + B * (w[0] * w[0] - t2); R[1] = B * w[0] * w[1] - A * w[2];   R[2] = B * w[0] * w[2] + A * w[1];
    R[3] = B * w[0] * w[1] + A * w[2];   R[4] = 1.0 + B * (w[1] * w[1] - t2); R[5] = B * w[1] * w[2] - A * w[0];
    R[6] = B * w[0] * w[2] - A * w[1];   R[7] = B * w[1] * w[2] + A * w[0];   R[8] = 1.0 + B * (w[2] * w[2] - t2);
}

// rows 0-2 of [[R, tau], [0, 1]] @ w2c in fp64, not rounded: V[3][4] row-major (row 3 of the product is w2c's own)
template <class T>
GS_HD void pose_compose_rows(const double d[6], const T* w2c, double V[12]) {
    double R[9];
    pose_rotation(d, R);
#pragma unroll
    for (int i = 0; i < 3; ++i) {
#pragma unroll
        for (int j = 0; j < 4; ++j)
            V[4 * i + j] = R[3 * i] * (double)w2c[j] + R[3 * i + 1] * (double)w2c[4 + j] + R[3 * i + 2] * (double)w2c[8 + j] +
                           d[3 + i] * (double)w2c[12 + j];
    }
}

// viewmat[16] = [[exp([omega]x), tau], [0, 1]] @ w2c, delta = {omega, tau}: formed in fp64, every entry rounded to fp32 once.
// delta == 0 hands w2c back bit for bit (the product would turn a -0 into +0).
GS_HD void pose_compose(const float delta[6], const float w2c[16], float viewmat[16]) {
    bool zero = true;
#pragma unroll
    for (int i = 0; i < 6; ++i) zero = zero && delta[i] == 0.f;
    double d[6], V[12];
#pragma unroll
    for (int i = 0; i < 6; ++i) d[i] = (double)delta[i];
    pose_compose_rows(d, w2c, V);
#pragma unroll
    for (int i = 0; i < 12; ++i) viewmat[i] = zero ? w2c[i] : (float)V[i];
#pragma unroll
    for (int i = 12; i < 16; ++i) viewmat[i] = w2c[i];
}

// v_delta[6] = dL / d delta from the view matrix' gradient as gs_project_bwd_cam hands it out: v_A[9] and v_t[3] (rows 0-2 of
// v_viewmats, the projection's part) and v_campos[3], the gradient of the camera centre the SH colours look from.
//   1. the centre's term into the matrix: V = [[A, t], [0, 1]], campos = -inv(A) t, u = -inv(A)^T v_campos:  v_t += u,
//      v_A += u campos^T  (what autograd gets from the 4x4 inverse; the general 3x3 inverse, no orthonormality assumed)
//   2. through the product: v_E = v_V[0:3, :] @ w2c^T; v_tau = its last column, v_R = its first three
//   3. through the exponential: R(omega + d) = exp([J_l d]x) R with J_l the left Jacobian of SO(3), so
//      v_omega = J_l^T a,  a = vee(M - M^T),  M = v_R R^T;  J_l^T = I - B [w]x + C [w]x^2.
template <class T>
GS_HD void pose_vjp(const double d[6], const T* w2c, const double v_A_in[9], const double v_t_in[3], const double v_campos[3],
                    double v_delta[6]) {
    double V[12], R[9];
    pose_compose_rows(d, w2c, V);
    pose_rotation(d, R);
    // 1.
    const double a00 = V[0], a01 = V[1], a02 = V[2], a10 = V[4], a11 = V[5], a12 = V[6], a20 = V[8], a21 = V[9], a22 = V[10];
    const double c00 = a11 * a22 - a12 * a21, c01 = a12 * a20 - a10 * a22, c02 = a10 * a21 - a11 * a20;   // cofactors of row 0
    const double c10 = a02 * a21 - a01 * a22, c11 = a00 * a22 - a02 * a20, c12 = a01 * a20 - a00 * a21;
    const double c20 = a01 * a12 - a02 * a11, c21 = a02 * a10 - a00 * a12, c22 = a00 * a11 - a01 * a10;
    const double idet = 1.0 / (a00 * c00 + a01 * c01 + a02 * c02);
    // inv(A)[i][j] = cof[j][i] / det, so inv(A)^T[i][j] = cof[i][j] / det
    const double t0 = V[3], t1 = V[7], t2 = V[11];
    const double campos[3] = {-(c00 * t0 + c10 * t1 + c20 * t2) * idet, -(c01 * t0 + c11 * t1 + c21 * t2) * idet,
                              -(c02 * t0 + c12 * t1 + c22 * t2) * idet};
    const double u[3] = {-(c00 * v_campos[0] + c01 * v_campos[1] + c02 * v_campos[2]) * idet,
                         -(c10 * v_campos[0] + c11 * v_campos[1] + c12 * v_campos[2]) * idet,
                         -(c20 * v_campos[0] + c21 * v_campos[1] + c22 * v_campos[2]) * idet};
    double vV[12];
#pragma unroll
    for (int i = 0; i < 3; ++i) {
#pragma unroll
        for (int j = 0; j < 3; ++j) vV[4 * i + j] = v_A_in[3 * i + j] + u[i] * campos[j];
        vV[4 * i + 3] = v_t_in[i] + u[i];
    }
    // 2.
    double vR[9];
#pragma unroll
    for (int i = 0; i < 3; ++i) {
#pragma unroll
        for (int k = 0; k < 4; ++k) {
            const double e = vV[4 * i] * (double)w2c[4 * k] + vV[4 * i + 1] * (double)w2c[4 * k + 1] + vV[4 * i + 2] * (double)w2c[4 * k + 2] +
                             vV[4 * i + 3] * (double)w2c[4 * k + 3];
            if (k < 3) vR[3 * i + k] = e;
            else v_delta[3 + i] = e;
        }
    }
    // 3.  M[i][j] = sum_k vR[i][k] R[j][k]
    auto M = [&](int i, int j) { return vR[3 * i] * R[3 * j] + vR[3 * i + 1] * R[3 * j + 1] + vR[3 * i + 2] * R[3 * j + 2]; };
    const double a[3] = {M(2, 1) - M(1, 2), M(0, 2) - M(2, 0), M(1, 0) - M(0, 1)};
    const double t2w = d[0] * d[0] + d[1] * d[1] + d[2] * d[2];
    double A, B, C;
    pose_coeffs(t2w, A, B, C);
    const double wa[3] = {d[1] * a[2] - d[2] * a[1], d[2] * a[0] - d[0] * a[2], d[0] * a[1] - d[1] * a[0]};           // w x a
    const double wwa[3] = {d[1] * wa[2] - d[2] * wa[1], d[2] * wa[0] - d[0] * wa[2], d[0] * wa[1] - d[1] * wa[0]};   // w x (w x a)
#pragma unroll
    for (int i = 0; i < 3; ++i) v_delta[i] = a[i] - B * wa[i] + C * wwa[i];
}

}  // namespace gs
