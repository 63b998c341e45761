// gs_normals.h -- THE definition of the normal-consistency regulariser (gs_normals.hip, normals.py): the normal of a
// Gaussian in camera space with its VJP to the quaternion, the normal of a rendered depth map by central differences, and the loss
// between the blended normals and the depth normals with its gradients.  Plain C++ that compiles for the device and for the host
// alike: tests/hostmath/normals.cpp builds it with the host compiler, tests/test_normals_host.py holds it to float64 restatements
// and tests/test_gpu_normals.py holds the kernels to it bit for bit.  Every product that feeds a sum is an explicit fmaf, so the
// result is the same with and without -ffp-contract; every division and square root is the correctly rounded one.
//
// Gaussian normal (pinhole; viewmat [4][4] row-major, world -> camera):
//   q_hat = q / |q| (wxyz), k = the index of the smallest scale value (the lowest index wins a tie; order only, no exp),
//   n_w = column k of R(q_hat), n_c = R_wc n_w, p_c = R_wc mean + t, n_c = -n_c where dot(n_c, p_c) > 0 (towards the camera).
//   VJP: to the quaternion only, through the column and the normalisation; k and the sign are piecewise constant.  Several cameras:
//   the gradient of n_w is summed in camera order, then taken through the quaternion once.
//
// Depth normal at an interior pixel (x, y) of a z-depth map d (camera K: fx, fy, cx, cy; x right, y down, z forward):
//   P(x, y) = d(x, y) * (u_x, v_y, 1), u_x = ((x + 0.5) - cx) / fx, v_y = ((y + 0.5) - cy) / fy
//   A = P(x, y + 1) - P(x, y - 1), B = P(x + 1, y) - P(x - 1, y), c = A x B, n_d = c / |c|      (a fronto-parallel plane: (0, 0, -1))
// A pixel's depth is *usable* when alpha >= min_alpha and 0 < d < inf (normal_depth_ok: the depth, or 0 for "none"); a centre is
// *valid* when it is interior, its own and its four neighbours' depths are usable and kNormalMinLen2 <= |c|^2 < inf.
// Loss: w = valid * (1 - mask) (LossComputer's convention: mask = 1 excludes; no mask: 0), e = 1 - dot(Nb, n_d) with Nb the blended,
// un-normalised normal; value = sum(w e) / sum(w) in fp64, exactly 0 when sum(w) == 0.
// Gradients, s = upstream * (1 / sum(w)) rounded once: v_Nb = (-(s w)) n_d; the depth of each of the four neighbours receives
// dot(v_P, (u, v, 1)) of its point, v_P = +-v_A or +-v_B, v_A = B x v_c, v_B = v_c x A, v_c = (v_n - n_d dot(n_d, v_n)) / |c|,
// v_n = (-(s w)) Nb.  A pixel's depth gradient is the sum of what the centres above, below, left and right of it send, in that order.
#pragma once
#include <math.h>
#include <stdint.h>

#ifdef __HIPCC__
#define GS_NM_HD __host__ __device__ __forceinline__
#else
#define GS_NM_HD static inline
#endif

namespace gs {

constexpr float kNormalMinLen2 = 1e-30f;   // |A x B|^2 below this: no normal (a normal float32, far above the subnormals)

// ---- the normal of a Gaussian ----

GS_NM_HD int normal_axis(float s0, float s1, float s2) {
    int k = 0;
    float m = s0;
    if (s1 < m) { k = 1; m = s1; }
    if (s2 < m) k = 2;
    return k;
}

// q_hat and |q| of a raw quaternion
GS_NM_HD float normal_quat_unit(const float* q, float qh[4]) {
    const float len = sqrtf(fmaf(q[3], q[3], fmaf(q[2], q[2], fmaf(q[1], q[1], q[0] * q[0]))));
    qh[0] = q[0] / len; qh[1] = q[1] / len; qh[2] = q[2] / len; qh[3] = q[3] / len;
    return len;
}

// column k of the rotation matrix of the unit quaternion (w, x, y, z)
GS_NM_HD void normal_rot_column(const float qh[4], int k, float n[3]) {
    const float w = qh[0], x = qh[1], y = qh[2], z = qh[3];
    if (k == 0) {
        n[0] = fmaf(-2.f, fmaf(y, y, z * z), 1.f);
        n[1] = 2.f * fmaf(x, y, w * z);
        n[2] = 2.f * fmaf(x, z, -(w * y));
    } else if (k == 1) {
        n[0] = 2.f * fmaf(x, y, -(w * z));
        n[1] = fmaf(-2.f, fmaf(x, x, z * z), 1.f);
        n[2] = 2.f * fmaf(y, z, w * x);
    } else {
        n[0] = 2.f * fmaf(x, z, w * y);
        n[1] = 2.f * fmaf(y, z, -(w * x));
        n[2] = fmaf(-2.f, fmaf(x, x, y * y), 1.f);
    }
}

// g: the gradient of the column; v: the gradient of (w, x, y, z)
GS_NM_HD void normal_rot_column_vjp(const float qh[4], int k, const float g[3], float v[4]) {
    const float w = qh[0], x = qh[1], y = qh[2], z = qh[3];
    if (k == 0) {
        v[0] = 2.f * fmaf(z, g[1], -(y * g[2]));
        v[1] = 2.f * fmaf(y, g[1], z * g[2]);
        v[2] = fmaf(-4.f * y, g[0], 2.f * fmaf(x, g[1], -(w * g[2])));
        v[3] = fmaf(-4.f * z, g[0], 2.f * fmaf(w, g[1], x * g[2]));
    } else if (k == 1) {
        v[0] = 2.f * fmaf(x, g[2], -(z * g[0]));
        v[1] = fmaf(-4.f * x, g[1], 2.f * fmaf(y, g[0], w * g[2]));
        v[2] = 2.f * fmaf(x, g[0], z * g[2]);
        v[3] = fmaf(-4.f * z, g[1], 2.f * fmaf(y, g[2], -(w * g[0])));
    } else {
        v[0] = 2.f * fmaf(y, g[0], -(x * g[1]));
        v[1] = fmaf(-4.f * x, g[2], 2.f * fmaf(z, g[0], -(w * g[1])));
        v[2] = fmaf(-4.f * y, g[2], 2.f * fmaf(w, g[0], z * g[1]));
        v[3] = 2.f * fmaf(x, g[0], y * g[1]);
    }
}

// n_w into camera space, faced towards the camera.  Returns the sign applied (+1 or -1).
GS_NM_HD float normal_to_camera(const float* vm, const float* mean, const float nw[3], float nc[3]) {
    const float n0 = fmaf(vm[2], nw[2], fmaf(vm[1], nw[1], vm[0] * nw[0]));
    const float n1 = fmaf(vm[6], nw[2], fmaf(vm[5], nw[1], vm[4] * nw[0]));
    const float n2 = fmaf(vm[10], nw[2], fmaf(vm[9], nw[1], vm[8] * nw[0]));
    const float p0 = fmaf(vm[2], mean[2], fmaf(vm[1], mean[1], fmaf(vm[0], mean[0], vm[3])));
    const float p1 = fmaf(vm[6], mean[2], fmaf(vm[5], mean[1], fmaf(vm[4], mean[0], vm[7])));
    const float p2 = fmaf(vm[10], mean[2], fmaf(vm[9], mean[1], fmaf(vm[8], mean[0], vm[11])));
    const float s = fmaf(n2, p2, fmaf(n1, p1, n0 * p0)) > 0.f ? -1.f : 1.f;
    nc[0] = s * n0; nc[1] = s * n1; nc[2] = s * n2;
    return s;
}

// The normals of Gaussian i under C cameras: normals[c * N * 3 + 3 i ..]
GS_NM_HD void gauss_normals_fwd(int64_t N, int C, int64_t i, const float* means, const float* quats, const float* scales,
                                const float* viewmats, float* normals) {
    float qh[4], nw[3], nc[3];
    normal_quat_unit(quats + 4 * i, qh);
    const int k = normal_axis(scales[3 * i], scales[3 * i + 1], scales[3 * i + 2]);
    normal_rot_column(qh, k, nw);
    for (int c = 0; c < C; ++c) {
        normal_to_camera(viewmats + 16 * c, means + 3 * i, nw, nc);
        float* o = normals + ((int64_t)c * N + i) * 3;
        o[0] = nc[0]; o[1] = nc[1]; o[2] = nc[2];
    }
}

// v_quats[4 i ..] from v_normals [C][N][3]
GS_NM_HD void gauss_normals_bwd(int64_t N, int C, int64_t i, const float* means, const float* quats, const float* scales,
                                const float* viewmats, const float* v_normals, float* v_quats) {
    float qh[4], nw[3], nc[3], g[3] = {0.f, 0.f, 0.f}, vh[4];
    const float len = normal_quat_unit(quats + 4 * i, qh);
    const int k = normal_axis(scales[3 * i], scales[3 * i + 1], scales[3 * i + 2]);
    normal_rot_column(qh, k, nw);
    for (int c = 0; c < C; ++c) {
        const float* vm = viewmats + 16 * c;
        const float s = normal_to_camera(vm, means + 3 * i, nw, nc);
        const float* v = v_normals + ((int64_t)c * N + i) * 3;
        const float a0 = s * v[0], a1 = s * v[1], a2 = s * v[2];
        // g += R_wc^T (s v)
        g[0] += fmaf(vm[8], a2, fmaf(vm[4], a1, vm[0] * a0));
        g[1] += fmaf(vm[9], a2, fmaf(vm[5], a1, vm[1] * a0));
        g[2] += fmaf(vm[10], a2, fmaf(vm[6], a1, vm[2] * a0));
    }
    normal_rot_column_vjp(qh, k, g, vh);
    // through q / |q|: (vh - q_hat dot(q_hat, vh)) / |q|
    const float d = fmaf(qh[3], vh[3], fmaf(qh[2], vh[2], fmaf(qh[1], vh[1], qh[0] * vh[0])));
    float* o = v_quats + 4 * i;
    o[0] = fmaf(-qh[0], d, vh[0]) / len;
    o[1] = fmaf(-qh[1], d, vh[1]) / len;
    o[2] = fmaf(-qh[2], d, vh[2]) / len;
    o[3] = fmaf(-qh[3], d, vh[3]) / len;
}

// ---- the normal of a depth map and the loss ----

struct NormalCam { float fx, fy, cx, cy; };
GS_NM_HD NormalCam normal_cam(const float* K) {
    NormalCam c;
    c.fx = K[0]; c.cx = K[2]; c.fy = K[4]; c.cy = K[5];
    return c;
}

// the depth where the pixel has a usable one, else 0
GS_NM_HD float normal_depth_ok(float d, float alpha, float min_alpha) {
    return (alpha >= min_alpha && d > 0.f && d <= 3.402823466e+38f) ? d : 0.f;
}
GS_NM_HD float normal_ray(int i, float c, float f) { return (((float)i + 0.5f) - c) / f; }

struct NormalCentre {
    float A[3], B[3], n[3], len;   // len = |A x B|
};

// The centre (x, y) from its own usable depth and its neighbours' (left, right, up = y - 1, down = y + 1): false when it is not
// valid.  The caller knows it to be interior.
GS_NM_HD bool normal_centre(const NormalCam& cam, int x, int y, float dc, float dl, float dr, float du, float dd, NormalCentre& o) {
    if (!(dc > 0.f && dl > 0.f && dr > 0.f && du > 0.f && dd > 0.f)) return false;
    const float ux = normal_ray(x, cam.cx, cam.fx), ul = normal_ray(x - 1, cam.cx, cam.fx), ur = normal_ray(x + 1, cam.cx, cam.fx);
    const float vy = normal_ray(y, cam.cy, cam.fy), vu = normal_ray(y - 1, cam.cy, cam.fy), vd = normal_ray(y + 1, cam.cy, cam.fy);
    o.A[0] = fmaf(dd, ux, -(du * ux)); o.A[1] = fmaf(dd, vd, -(du * vu)); o.A[2] = dd - du;
    o.B[0] = fmaf(dr, ur, -(dl * ul)); o.B[1] = fmaf(dr, vy, -(dl * vy)); o.B[2] = dr - dl;
    const float c0 = fmaf(o.A[1], o.B[2], -(o.A[2] * o.B[1]));
    const float c1 = fmaf(o.A[2], o.B[0], -(o.A[0] * o.B[2]));
    const float c2 = fmaf(o.A[0], o.B[1], -(o.A[1] * o.B[0]));
    const float len2 = fmaf(c2, c2, fmaf(c1, c1, c0 * c0));
    if (!(len2 >= kNormalMinLen2 && len2 <= 3.402823466e+38f)) return false;
    o.len = sqrtf(len2);
    o.n[0] = c0 / o.len; o.n[1] = c1 / o.len; o.n[2] = c2 / o.len;
    return true;
}

GS_NM_HD float normal_loss_weight(float m) { return 1.f - m; }   // of a valid centre; one rounding

// acc += {w e, w} of a valid centre of weight w != 0: the product of two fp32 numbers is exact in fp64, only the sums round
GS_NM_HD void normal_loss_accumulate(double acc[2], const NormalCentre& c, const float* nb, float w) {
    const float e = 1.f - fmaf(nb[2], c.n[2], fmaf(nb[1], c.n[1], nb[0] * c.n[0]));
    acc[0] += (double)w * (double)e;
    acc[1] += (double)w;
}

// value = sum(w e) / sum(w) and 1 / sum(w), each formed in fp64 and rounded to fp32 once; exactly {0, 0} when nothing counts
GS_NM_HD void normal_loss_finish(double sum_we, double sum_w, float& value, float& inv_w) {
    const bool any = sum_w > 0.0;
    value = any ? (float)(sum_we / sum_w) : 0.f;
    inv_w = any ? (float)(1.0 / sum_w) : 0.f;
}

// The gradients a valid centre of weight w sends, g = -(s w): v_nb[3] to its own blended normal and send[4] to the depths of its
// {up, down, left, right} neighbours.
GS_NM_HD void normal_centre_vjp(const NormalCam& cam, int x, int y, const NormalCentre& c, const float* nb, float g, float v_nb[3],
                                float send[4]) {
    v_nb[0] = g * c.n[0]; v_nb[1] = g * c.n[1]; v_nb[2] = g * c.n[2];
    const float vn0 = g * nb[0], vn1 = g * nb[1], vn2 = g * nb[2];
    const float d = fmaf(c.n[2], vn2, fmaf(c.n[1], vn1, c.n[0] * vn0));
    const float vc0 = fmaf(-c.n[0], d, vn0) / c.len, vc1 = fmaf(-c.n[1], d, vn1) / c.len, vc2 = fmaf(-c.n[2], d, vn2) / c.len;
    // v_A = B x v_c, v_B = v_c x A
    const float a0 = fmaf(c.B[1], vc2, -(c.B[2] * vc1)), a1 = fmaf(c.B[2], vc0, -(c.B[0] * vc2)), a2 = fmaf(c.B[0], vc1, -(c.B[1] * vc0));
    const float b0 = fmaf(vc1, c.A[2], -(vc2 * c.A[1])), b1 = fmaf(vc2, c.A[0], -(vc0 * c.A[2])), b2 = fmaf(vc0, c.A[1], -(vc1 * c.A[0]));
    const float ux = normal_ray(x, cam.cx, cam.fx), ul = normal_ray(x - 1, cam.cx, cam.fx), ur = normal_ray(x + 1, cam.cx, cam.fx);
    const float vy = normal_ray(y, cam.cy, cam.fy), vu = normal_ray(y - 1, cam.cy, cam.fy), vd = normal_ray(y + 1, cam.cy, cam.fy);
    send[0] = -fmaf(a1, vu, fmaf(a0, ux, a2));
    send[1] = fmaf(a1, vd, fmaf(a0, ux, a2));
    send[2] = -fmaf(b1, vy, fmaf(b0, ul, b2));
    send[3] = fmaf(b1, vy, fmaf(b0, ur, b2));
}

// what the pixel's depth receives: from the centre above it (whose "down" it is), below, left of it (whose "right" it is), right
GS_NM_HD float normal_depth_gather(float from_above_down, float from_below_up, float from_left_right, float from_right_left) {
    return ((from_above_down + from_below_up) + from_left_right) + from_right_left;
}

}  // namespace gs
