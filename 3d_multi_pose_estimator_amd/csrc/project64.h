// The binary64 camera model and the 3-unknown Levenberg-Marquardt step of the geometry stages (refine.hip, skel_refine.hip,
// regroup.hip, consolidate.hip, calib.hip), stated once so that every file rounds the same operations in the same order:
// DESIGN.md 2.2.  include/mpe.h words the lines under mpe_refine_batch; harness/refine.py is their numpy statement, and
// tests/native/camera64_test.cpp holds this file to it bit for bit on the host.  A camera is (T [12] the 3 x 4 extrinsics,
// dist [5], K [9] float): calib.hip and camfit.hip pass their trial cameras, everyone else cfg->P[c].  Plain inline functions that need
// <math.h> and <stdint.h> only.  Contraction is off from here to the end of the including file (a host build passes
// -ffp-contract=off); f64 quotients and roots are the language's correctly rounded ones.
#pragma once
#include <math.h>
#include <stddef.h>
#include <stdint.h>

#if defined(__HIPCC__) || defined(__CUDACC__)
#define MPE_CAM_HD __host__ __device__
#else
#define MPE_CAM_HD
#endif
#if defined(__clang__)
#pragma clang fp contract(off)
#endif

namespace mpe {

// |x| < inf: false for an infinity and for a NaN, so the same as isfinite on every input
MPE_CAM_HD inline bool finite3(double a, double b, double c) {
    const double inf = __builtin_huge_val();
    return fabs(a) < inf && fabs(b) < inf && fabs(c) < inf;
}

// the unsigned integer as wide as T: coordinates that are copied through keep their bits (a NaN its payload)
template <typename T>
struct Bits;
template <>
struct Bits<float> { typedef uint32_t type; };
template <>
struct Bits<double> { typedef uint64_t type; };

// joint `at` of poses [..][3], f32 or with pose_f64 f64, widened
MPE_CAM_HD inline void load3(const void *poses, int pose_f64, size_t at, double *X) {
    if (pose_f64) {
        const double *q = static_cast<const double *>(poses) + at * 3;
        X[0] = q[0], X[1] = q[1], X[2] = q[2];
    } else {
        const float *q = static_cast<const float *>(poses) + at * 3;
        X[0] = (double)q[0], X[1] = (double)q[1], X[2] = (double)q[2];
    }
}

struct Proj {                                 // the header's projection lines, kept for the Jacobian
    double pc2, h0, h1, r, f, u2, px, py;
};

// the point in the camera's frame; a caller that must not divide by pc[2] <= 0 tests it before project_pc
MPE_CAM_HD inline void to_camera(const double *T, double X0, double X1, double X2, double *pc) {
    for (int i = 0; i < 3; ++i) pc[i] = ((T[4 * i] * X0 + T[4 * i + 1] * X1) + T[4 * i + 2] * X2) + T[4 * i + 3];
}

MPE_CAM_HD inline Proj project_pc(const double *pc, const double *dist, const float *K) {
    const double kd0 = dist[0], kd1 = dist[1], kd2 = dist[4];
    Proj p;
    p.pc2 = pc[2];
    p.h0 = pc[0] / pc[2];
    p.h1 = pc[1] / pc[2];
    p.r = p.h0 * p.h0 + p.h1 * p.h1;
    p.f = ((1.0 + kd0 * p.r) + (kd1 * p.r) * p.r) + ((kd2 * p.r) * p.r) * p.r;
    const double d0 = p.h0 * p.f, d1 = p.h1 * p.f;
    double u[3];
    for (int i = 0; i < 3; ++i) u[i] = ((double)K[3 * i] * d0 + (double)K[3 * i + 1] * d1) + (double)K[3 * i + 2];
    p.u2 = u[2];
    p.px = u[0] / u[2];
    p.py = u[1] / u[2];
    return p;
}

MPE_CAM_HD inline Proj project(const double *T, const double *dist, const float *K, double X0, double X1, double X2) {
    double pc[3];
    to_camera(T, X0, X1, X2, pc);
    return project_pc(pc, dist, K);
}

// d f / d r of the lens model at p
MPE_CAM_HD inline double radial_slope(const double *dist, const Proj &p) {
    return (dist[0] + (2.0 * dist[1]) * p.r) + ((3.0 * dist[4]) * p.r) * p.r;
}

// The tail of every Jacobian of (px, py): (ak, bk) = the derivative of (h0, h1) by one unknown, fd = radial_slope
MPE_CAM_HD inline void jacobian_tail(const Proj &p, const float *K, double fd, double ak, double bk, double *jx, double *jy) {
    const double qk = fd * (2.0 * (p.h0 * ak + p.h1 * bk));
    const double mk = ak * p.f + p.h0 * qk, nk = bk * p.f + p.h1 * qk;
    const double v0 = (double)K[0] * mk + (double)K[1] * nk, v1 = (double)K[3] * mk + (double)K[4] * nk;
    const double v2 = (double)K[6] * mk + (double)K[7] * nk;
    *jx = (v0 - p.px * v2) / p.u2;
    *jy = (v1 - p.py * v2) / p.u2;
}

// the derivatives of (px, py) by the point's X0, X1, X2
MPE_CAM_HD inline void point_jacobian(const double *T, const double *dist, const float *K, const Proj &p, double *jx, double *jy) {
    const double fd = radial_slope(dist, p);
    for (int k = 0; k < 3; ++k) {
        const double ak = (T[k] - p.h0 * T[8 + k]) / p.pc2, bk = (T[4 + k] - p.h1 * T[8 + k]) / p.pc2;
        jacobian_tail(p, K, fd, ak, bk, jx + k, jy + k);
    }
}

// the derivatives of (px, py) by the six-vector (w, tau) of a rigid perturbation of the camera, d pc = w x pc + tau: those
// by the camera-frame point through the shared tail, then the cross products; fd = radial_slope
MPE_CAM_HD inline void rigid_jacobian(const Proj &pr, const float *K, double fd, const double *pc, double *jx, double *jy) {
    const double da[3] = {1.0 / pc[2], 0.0, (-pr.h0) / pc[2]}, db[3] = {0.0, 1.0 / pc[2], (-pr.h1) / pc[2]};
    double cx[3], cy[3];
    for (int k = 0; k < 3; ++k) jacobian_tail(pr, K, fd, da[k], db[k], cx + k, cy + k);
    jx[0] = cx[2] * pc[1] - cx[1] * pc[2];
    jx[1] = cx[0] * pc[2] - cx[2] * pc[0];
    jx[2] = cx[1] * pc[0] - cx[0] * pc[1];
    jx[3] = cx[0], jx[4] = cx[1], jx[5] = cx[2];
    jy[0] = cy[2] * pc[1] - cy[1] * pc[2];
    jy[1] = cy[0] * pc[2] - cy[2] * pc[0];
    jy[2] = cy[1] * pc[0] - cy[0] * pc[1];
    jy[3] = cy[0], jy[4] = cy[1], jy[5] = cy[2];
}

// Huber's cost of a residual of length e, and the weight of its normal equations; huber <= 0: the plain square
MPE_CAM_HD inline double rho(double e, double huber) {
    return (huber <= 0.0 || e <= huber) ? e * e : (2.0 * huber) * e - huber * huber;
}

MPE_CAM_HD inline double huber_weight(double e, double huber) { return (huber <= 0.0 || e <= huber) ? 1.0 : huber / e; }

// The normal equations of three unknowns, folded term by term in the caller's order, and one damped step on them
struct Normal3 {
    double A00 = 0.0, A01 = 0.0, A02 = 0.0, A11 = 0.0, A12 = 0.0, A22 = 0.0, g0 = 0.0, g1 = 0.0, g2 = 0.0;

    // a pixel residual (rx, ry) of weight w with the Jacobian rows jx, jy
    MPE_CAM_HD void add_pixel(double w, const double *jx, const double *jy, double rx, double ry) {
        A00 = A00 + w * (jx[0] * jx[0] + jy[0] * jy[0]);
        A01 = A01 + w * (jx[0] * jx[1] + jy[0] * jy[1]);
        A02 = A02 + w * (jx[0] * jx[2] + jy[0] * jy[2]);
        A11 = A11 + w * (jx[1] * jx[1] + jy[1] * jy[1]);
        A12 = A12 + w * (jx[1] * jx[2] + jy[1] * jy[2]);
        A22 = A22 + w * (jx[2] * jx[2] + jy[2] * jy[2]);
        g0 = g0 + w * (jx[0] * rx + jy[0] * ry);
        g1 = g1 + w * (jx[1] * rx + jy[1] * ry);
        g2 = g2 + w * (jx[2] * rx + jy[2] * ry);
    }

    // a scalar residual q with the Jacobian row m
    MPE_CAM_HD void add_bone(const double *m, double q) {
        A00 = A00 + m[0] * m[0];
        A01 = A01 + m[0] * m[1];
        A02 = A02 + m[0] * m[2];
        A11 = A11 + m[1] * m[1];
        A12 = A12 + m[1] * m[2];
        A22 = A22 + m[2] * m[2];
        g0 = g0 + m[0] * q;
        g1 = g1 + m[1] * q;
        g2 = g2 + m[2] * q;
    }

    // (A + lambda diag A) e = -g, LDL^T written out -> every pivot is positive and e is finite
    MPE_CAM_HD bool lm_step(double lambda, double *e) const {
        const double M00 = A00 + lambda * A00, M11 = A11 + lambda * A11, M22 = A22 + lambda * A22;
        const double D0 = M00;
        const double L10 = A01 / D0, L20 = A02 / D0;
        const double D1 = M11 - L10 * A01;
        const double t = A12 - L20 * A01;
        const double L21 = t / D1;
        const double D2 = (M22 - L20 * A02) - L21 * t;
        const double z0 = -g0;
        const double z1 = -g1 - L10 * z0;
        const double z2 = (-g2 - L20 * z0) - L21 * z1;
        e[2] = z2 / D2;
        e[1] = z1 / D1 - L21 * e[2];
        e[0] = (z0 / D0 - L10 * e[1]) - L20 * e[2];
        return D0 > 0.0 && D1 > 0.0 && D2 > 0.0 && finite3(e[0], e[1], e[2]);
    }
};

}  // namespace mpe
