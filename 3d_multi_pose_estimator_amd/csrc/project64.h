// The binary64 projection lines of mpe_refine_batch (include/mpe.h words them), shared by refine.hip and regroup.hip so
// that both files round the same operations in the same order.  Contraction is off from here to the end of the including
// file; f64 quotients are the language's correctly rounded ones.
#pragma once
#include "mpe_internal.h"

#pragma clang fp contract(off)

namespace mpe {

struct Proj {                                 // the header's projection lines, kept for the Jacobian
    double pc2, h0, h1, r, f, u2, px, py;
};

__device__ inline Proj project(const DevCfg *cfg, int c, double X0, double X1, double X2) {
    const double *T = cfg->P[c];
    double pc[3];
    for (int i = 0; i < 3; ++i) pc[i] = ((T[4 * i] * X0 + T[4 * i + 1] * X1) + T[4 * i + 2] * X2) + T[4 * i + 3];
    const double kd0 = cfg->dist[c][0], kd1 = cfg->dist[c][1], kd2 = cfg->dist[c][4];
    Proj p;
    p.pc2 = pc[2];
    p.h0 = pc[0] / pc[2];
    p.h1 = pc[1] / pc[2];
    p.r = p.h0 * p.h0 + p.h1 * p.h1;
    p.f = ((1.0 + kd0 * p.r) + (kd1 * p.r) * p.r) + ((kd2 * p.r) * p.r) * p.r;
    const double d0 = p.h0 * p.f, d1 = p.h1 * p.f;
    const float *K = cfg->K[c];
    double u[3];
    for (int i = 0; i < 3; ++i) u[i] = ((double)K[3 * i] * d0 + (double)K[3 * i + 1] * d1) + (double)K[3 * i + 2];
    p.u2 = u[2];
    p.px = u[0] / u[2];
    p.py = u[1] / u[2];
    return p;
}

__device__ inline bool finite3(double a, double b, double c) {
    const double inf = __builtin_huge_val();
    return fabs(a) < inf && fabs(b) < inf && fabs(c) < inf;
}

}  // namespace mpe
