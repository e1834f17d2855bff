// The binary64 ray lines of mpe_geom_scores_batch (include/mpe.h words them), shared by geom.hip and consolidate.hip so
// that both files round the same operations in the same order: the two Newton steps on the lens model, the unit ray of a
// pixel, the camera centre, and the distance of two rays at their closest points in front of both cameras.  Contraction
// is off from here to the end of the including file; f64 quotients and roots are the language's correctly rounded ones.
#pragma once
#include "dlt_common.h"

#pragma clang fp contract(off)

namespace mpe {

// Two Newton steps on the lens model from undistort_point's (x, y), the header's lines: the five fixed-point iterations
// leave up to 1.5e-2 px at the image border, the steps bring a ray within 1e-6 px of its pixel everywhere.
__device__ inline void polish_point(const DevCfg *cfg, int cam, double u, double v, double *px, double *py) {
    const float *K = cfg->K[cam];
    const double *dc = cfg->dist[cam];
    const double k1 = dc[0], k2 = dc[1], p1 = dc[2], p2 = dc[3], k3 = dc[4];
    const double xt = (u - (double)K[2]) * (1.0 / (double)K[0]), yt = (v - (double)K[5]) * (1.0 / (double)K[4]);
    double x = *px, y = *py;
    for (int it = 0; it < 2; ++it) {
        const double r = x * x + y * y;
        const double f = 1.0 + ((k3 * r + k2) * r + k1) * r;
        const double fd = ((3.0 * k3) * r + 2.0 * k2) * r + k1;
        const double tx = 2.0 * x, ty = 2.0 * y;
        const double ex = ((x * f + p1 * (tx * y)) + p2 * (r + tx * x)) - xt;
        const double ey = ((y * f + p1 * (r + ty * y)) + p2 * (tx * y)) - yt;
        const double a = ((f + (tx * x) * fd) + p1 * ty) + (3.0 * p2) * tx;
        const double b = ((tx * y) * fd + p1 * tx) + p2 * ty;
        const double d = ((f + (ty * y) * fd) + (3.0 * p1) * ty) + p2 * tx;
        const double det = a * d - b * b;
        const double nx = x - (d * ex - b * ey) / det, ny = y - (a * ey - b * ex) / det;
        x = nx, y = ny;
    }
    *px = x;
    *py = y;
}

// the centre of camera c in the world frame
__device__ inline void camera_centre(const DevCfg *cfg, int c, double *o) {
    const double *T = cfg->P[c];
    for (int k = 0; k < 3; ++k) o[k] = -((T[k] * T[3] + T[4 + k] * T[7]) + T[8 + k] * T[11]);
}

// the unit direction, world frame, of the ray of pixel (u, v) of camera c: undistort_point, the two Newton steps, the
// rotation, the norm
__device__ inline void unit_ray(const DevCfg *cfg, int c, double u, double v, double *r) {
    double x, y;
    dltc::undistort_point(cfg, c, u, v, &x, &y);
    polish_point(cfg, c, u, v, &x, &y);
    const double *T = cfg->P[c];
    const double q0 = (T[0] * x + T[4] * y) + T[8], q1 = (T[1] * x + T[5] * y) + T[9], q2 = (T[2] * x + T[6] * y) + T[10];
    const double n = sqrt((q0 * q0 + q1 * q1) + q2 * q2);
    r[0] = q0 / n, r[1] = q1 / n, r[2] = q2 / n;
}

// the distance of the rays (o1, p1) and (o2, p2) at their closest points, both parameters clamped at 0; clip > 0 bounds it
__device__ inline double ray_distance(const double *p1, const double *p2, const double *o1, const double *o2, double clip) {
    const double a0 = p1[0], a1 = p1[1], a2 = p1[2], b0 = p2[0], b1 = p2[1], b2 = p2[2];
    const double o10 = o1[0], o11 = o1[1], o12 = o1[2], o20 = o2[0], o21 = o2[1], o22 = o2[2];
    const double w0 = o10 - o20, w1_ = o11 - o21, w2_ = o12 - o22;
    const double b = (a0 * b0 + a1 * b1) + a2 * b2;
    const double d = (a0 * w0 + a1 * w1_) + a2 * w2_;
    const double e = (b0 * w0 + b1 * w1_) + b2 * w2_;
    const double den = 1.0 - b * b;
    double t1, t2;
    if (den < 1e-12) {
        t1 = 0.0;
        t2 = e;
    } else {
        t1 = (b * e - d) / den;
        t2 = (e - b * d) / den;
    }
    if (t1 < 0.0) t1 = 0.0;
    if (t2 < 0.0) t2 = 0.0;
    const double g0 = (o10 + t1 * a0) - (o20 + t2 * b0), g1 = (o11 + t1 * a1) - (o21 + t2 * b1), g2 = (o12 + t1 * a2) - (o22 + t2 * b2);
    double dist = sqrt((g0 * g0 + g1 * g1) + g2 * g2);
    if (clip > 0.0 && dist > clip) dist = clip;
    return dist;
}

}  // namespace mpe
