// The two OpenCV calls of the 3D stages restated in f64 (pose3d.hip has the citations): cv2.undistortPoints (five fixed-point iterations
// of the k1, k2, p1, p2, k3 model, here) and cv2.triangulatePoints (4 x 4 DLT system, right singular vector of the smallest singular
// value: dlt_solve.h -- a one-sided Jacobi in registers that orthogonalises the ROWS of the system and accumulates nothing; the vector
// is the 4-D cross product of the three longest converged rows).  One definition for every kernel that solves pairs (pose3d.hip: the
// row, triangulation and explicit-pair kernels; cluster.hip: the small-batch tail launch that solves every cross-camera pair of a
// frame beside the clustering), so that a pair gives the same bits wherever it was solved.
#pragma once
#include "mpe_internal.h"
#include "dlt_solve.h"

namespace mpe {
namespace dltc {

__device__ inline void undistort_point(const DevCfg *cfg, int cam, double u, double v, double *ox, double *oy) {
#pragma clang fp contract(off)
    const float *K = cfg->K[cam];
    const double fx = (double)K[0], fy = (double)K[4], cx = (double)K[2], cy = (double)K[5];
    const double *d = cfg->dist[cam];
    const double k1 = d[0], k2 = d[1], p1 = d[2], p2 = d[3], k3 = d[4];
    const double ifx = 1.0 / fx, ify = 1.0 / fy;
    double x = (u - cx) * ifx, y = (v - cy) * ify;
    const double x0 = x, y0 = y;
    for (int it = 0; it < 5; ++it) {
        const double r2 = x * x + y * y;
        const double icdist = 1.0 / (1.0 + ((k3 * r2 + k2) * r2 + k1) * r2);
        if (icdist < 0) {
            x = x0;
            y = y0;
            break;
        }
        const double dx = 2 * p1 * x * y + p2 * (r2 + 2 * x * x);
        const double dy = p1 * (r2 + 2 * y * y) + 2 * p2 * x * y;
        x = (x0 - dx) * icdist;
        y = (y0 - dy) * icdist;
    }
    *ox = x;
    *oy = y;
}

__device__ inline int pair_index(int c1, int c2, int V) {   // lexicographic index of (c1<c2)
    return c1 * V - c1 * (c1 + 1) / 2 + (c2 - c1 - 1);
}


}  // namespace dltc
}  // namespace mpe
