// cv2.triangulatePoints for one pair of views, in f64: the 4 x 4 DLT system A, its right singular vector of the smallest singular
// value, dehomogenised.  ONE definition for every kernel that solves pairs (dlt_common.h) and for the stand-alone host program
// tests/native/dlt_solve_host.cpp; it needs <math.h> only.
//
// The result is ONE vector, so nothing is accumulated: the cyclic one-sided Jacobi runs on the columns of A^T, i.e. it rotates
// the ROWS of A until they are orthogonal.  The converged rows are sigma_i v_i^T, and the wanted v is orthogonal to the three rows
// that are not the shortest: their 4-D cross product (four 3 x 3 cofactors).  That stays accurate when sigma_4 is tiny (noise-free
// matched pairs), where dividing the shortest row by its norm does not.
//
// A rotation needs (c, s) orthonormal to a few ulp, not a correctly rounded t: the square root and the quotient of
// t = sign(zeta) / (|zeta| + sqrt(1 + zeta^2)) come from the hardware's rsq / rcp estimates and one Newton step each (the operands
// are sums of squares of O(1) numbers: no scaling, no fix-up), c = rsqrt(1 + t^2) is kept.  The host build writes 1 / sqrt(x) and
// 1 / x for the estimates; its bits are not the device's, a pair's bits are the same on every DEVICE call site.
//
// The squared row norms are computed at the start of a sweep and carried across its rotations (al' = al - t ga, be' = be + t ga):
// a carried norm of a row that has become tiny is rounding noise, which can only make the sweep skip or waste a rotation -- the
// sweep that ends the iteration rotates nothing, so it tests every pair on freshly computed norms.
//
// gfx950, -O3: 663 instructions (422 f64), no scratch; the solver with V accumulated and IEEE sqrt / division was 942 (615) and
// indexed V through scratch.  profiles/r07_dlt_solver.txt has the kernel times of each step.
#pragma once
#include <math.h>

#if defined(__HIPCC__) || defined(__CUDACC__)
#define MPE_DLT_HD __host__ __device__
#else
#define MPE_DLT_HD
#endif
#if defined(__clang__)
#define MPE_DLT_UNROLL _Pragma("unroll")
#else
#define MPE_DLT_UNROLL
#endif

namespace mpe {
namespace dltc {

constexpr int DLT_MAX_SWEEPS = 12;

MPE_DLT_HD inline double dlt_rsq_est(double x) {
#if defined(__HIP_DEVICE_COMPILE__)
    return __builtin_amdgcn_rsq(x);
#elif defined(MPE_DLT_COARSE_ESTIMATES)      // host test only: an estimate of 24 bits, so that the Newton step has work to do
    return (double)(float)(1.0 / sqrt(x));
#else
    return 1.0 / sqrt(x);
#endif
}

MPE_DLT_HD inline double dlt_rcp_est(double x) {
#if defined(__HIP_DEVICE_COMPILE__)
    return __builtin_amdgcn_rcp(x);
#elif defined(MPE_DLT_COARSE_ESTIMATES)
    return (double)(float)(1.0 / x);
#else
    return 1.0 / x;
#endif
}

MPE_DLT_HD inline double dlt_rsqrt(double x) {
#if defined(__HIP_DEVICE_COMPILE__)
    return rsqrt(x);
#else
    return 1.0 / sqrt(x);
#endif
}

// (c, s) and t = s / c of the rotation that makes two vectors with squared norms al, be and inner product ga (!= 0) orthogonal; the
// rotated vectors have the squared norms al - t ga and be + t ga
MPE_DLT_HD inline void dlt_rotation(double al, double be, double ga, double *c_out, double *s_out, double *t_out) {
    const double d = be - al, g2 = 2.0 * fabs(ga);
    const double sg = (d == 0.0 || (d > 0.0) == (ga > 0.0)) ? 1.0 : -1.0;
    const double h = d * d + g2 * g2;                     // > 0: ga != 0 (an h that underflows or overflows gives a NaN
    const double y = dlt_rsq_est(h);                      //      rotation, as it gave a NaN t before)
    const double r0 = h * y;
    const double r = fma(0.5 * y, fma(-r0, r0, h), r0);   // sqrt(h), one Newton step
    const double den = fabs(d) + r;
    const double q0 = dlt_rcp_est(den);
    const double q = fma(q0, fma(-den, q0, 1.0), q0);     // 1 / den, one Newton step
    const double t = sg * g2 * q;
    const double c = dlt_rsqrt(1.0 + t * t);
    *t_out = t;
    *c_out = c;
    *s_out = c * t;
}

// out[3]: the triangulated point; returns the sweeps used (<= DLT_MAX_SWEEPS)
MPE_DLT_HD inline int dlt_solve(const double *P1, const double *P2, double x1, double y1, double x2, double y2,
                                double *out) {
#if defined(__clang__)
#pragma clang fp contract(fast)      // an iteration to convergence: its result does not hang on the rounding of single steps
#endif
    double A[4][4];
MPE_DLT_UNROLL
    for (int k = 0; k < 4; ++k) {
        A[0][k] = x1 * P1[8 + k] - P1[k];
        A[1][k] = y1 * P1[8 + k] - P1[4 + k];
        A[2][k] = x2 * P2[8 + k] - P2[k];
        A[3][k] = y2 * P2[8 + k] - P2[4 + k];
    }
    // converged when every pair of rows is orthogonal to a few ulp: |<a_p,a_q>| <= 4e-16 |a_p||a_q|
    int sweeps = 0;
    for (; sweeps < DLT_MAX_SWEEPS; ++sweeps) {
        bool rotated = false;
        double nr[4];                     // squared row norms: computed at the start of a sweep, carried across its rotations
MPE_DLT_UNROLL
        for (int j = 0; j < 4; ++j) {
            nr[j] = 0;
MPE_DLT_UNROLL
            for (int k = 0; k < 4; ++k) nr[j] += A[j][k] * A[j][k];
        }
MPE_DLT_UNROLL
        for (int p = 0; p < 3; ++p)
MPE_DLT_UNROLL
            for (int q = p + 1; q < 4; ++q) {
                const double al = nr[p], be = nr[q];
                double ga = 0;
MPE_DLT_UNROLL
                for (int k = 0; k < 4; ++k) ga += A[p][k] * A[q][k];
                if (ga * ga <= 1.6e-31 * (al * be) || ga == 0.0) continue;
                rotated = true;
                double c, s, t;
                dlt_rotation(al, be, ga, &c, &s, &t);
                nr[p] = al - t * ga;
                nr[q] = be + t * ga;
MPE_DLT_UNROLL
                for (int k = 0; k < 4; ++k) {
                    const double ap = A[p][k], aq = A[q][k];
                    A[p][k] = c * ap - s * aq;
                    A[q][k] = s * ap + c * aq;
                }
            }
        if (!rotated) break;
    }
    // the shortest row (the first of equal norms) is left out
    int jm = 0;
    double best = 0;
MPE_DLT_UNROLL
    for (int j = 0; j < 4; ++j) {
        double nn = 0;
MPE_DLT_UNROLL
        for (int k = 0; k < 4; ++k) nn += A[j][k] * A[j][k];
        if (j == 0 || nn < best) {
            best = nn;
            jm = j;
        }
    }
    double a[4], b[4], e[4];
MPE_DLT_UNROLL
    for (int k = 0; k < 4; ++k) {
        a[k] = jm == 0 ? A[1][k] : A[0][k];
        b[k] = jm <= 1 ? A[2][k] : A[1][k];
        e[k] = jm <= 2 ? A[3][k] : A[2][k];
    }
    // 4-D cross product of a, b, e (up to a common sign, which the dehomogenisation removes)
    const double m01 = b[0] * e[1] - b[1] * e[0], m02 = b[0] * e[2] - b[2] * e[0], m03 = b[0] * e[3] - b[3] * e[0];
    const double m12 = b[1] * e[2] - b[2] * e[1], m13 = b[1] * e[3] - b[3] * e[1], m23 = b[2] * e[3] - b[3] * e[2];
    const double v0 = a[1] * m23 - a[2] * m13 + a[3] * m12;
    const double v1 = -(a[0] * m23 - a[2] * m03 + a[3] * m02);
    const double v2 = a[0] * m13 - a[1] * m03 + a[3] * m01;
    const double v3 = -(a[0] * m12 - a[1] * m02 + a[2] * m01);
    out[0] = v0 / v3;
    out[1] = v1 / v3;
    out[2] = v2 / v3;
    return sweeps;
}

}  // namespace dltc
}  // namespace mpe
