// The inverse of a joint's 3 x 3 normal matrix and the covariance mpe_posecov_batch reports from it (include/mpe.h has the
// rule): posecov.hip runs it per joint, and the stand-alone program tests/native/cov3_test.cpp holds it to the numpy
// statement harness/uncertainty.py (inverse3, finish) bit for bit on the host.  Header only, <math.h> only, no HIP: plain
// inline functions for host and device.  Contraction is off from here to the end of the including file (a host build
// passes -ffp-contract=off); f64 quotients and roots are the language's correctly rounded ones.
//
// A = (A00, A01, A02, A11, A12, A22), the upper triangle row by row; S and cov in the same order.
// cov3_inverse: A = L D L^T by the refinement's lines (project64.h, Normal3::lm_step) without damping, then
// S = L^-T D^-1 L^-1 written out:
//   D0 = A00 ; L10 = A01 / D0 ; L20 = A02 / D0 ; D1 = A11 - L10*A01 ; t = A12 - L20*A01 ; L21 = t / D1
//   D2 = (A22 - L20*A02) - L21*t
//   i0 = 1 / D0 ; i1 = 1 / D1 ; i2 = 1 / D2 ; m = L10*L21 - L20
//   S22 = i2 ; S12 = -L21*i2 ; S02 = m*i2
//   S11 = i1 - L21*S12 ; S01 = (-L10)*i1 + m*S12
//   S00 = (i0 + (L10*L10)*i1) + m*S02
//   -> every pivot D0, D1, D2 is > 0 (a NaN is not)
// cov3_finish: cov_q = s2 * S_q, sigma = sqrt((cov00 + cov11) + cov22) -> every cov_q and sigma is finite.
#pragma once
#include <math.h>

#if defined(__HIPCC__) || defined(__CUDACC__)
#define MPE_COV_HD __host__ __device__
#else
#define MPE_COV_HD
#endif
#if defined(__clang__)
#pragma clang fp contract(off)
#endif

namespace mpe {

MPE_COV_HD inline bool cov3_inverse(const double *A, double *S) {
    const double A00 = A[0], A01 = A[1], A02 = A[2], A11 = A[3], A12 = A[4], A22 = A[5];
    const double D0 = A00;
    const double L10 = A01 / D0, L20 = A02 / D0;
    const double D1 = A11 - L10 * A01;
    const double t = A12 - L20 * A01;
    const double L21 = t / D1;
    const double D2 = (A22 - L20 * A02) - L21 * t;
    const double i0 = 1.0 / D0, i1 = 1.0 / D1, i2 = 1.0 / D2;
    const double m = L10 * L21 - L20;
    const double S22 = i2;
    const double S12 = -L21 * i2;
    const double S02 = m * i2;
    const double S11 = i1 - L21 * S12;
    const double S01 = (-L10) * i1 + m * S12;
    const double S00 = (i0 + (L10 * L10) * i1) + m * S02;
    S[0] = S00, S[1] = S01, S[2] = S02, S[3] = S11, S[4] = S12, S[5] = S22;
    return D0 > 0.0 && D1 > 0.0 && D2 > 0.0;
}

MPE_COV_HD inline bool cov3_finish(const double *S, double s2, double *cov, double *sigma) {
    const double inf = __builtin_huge_val();
    bool finite = true;
    for (int q = 0; q < 6; ++q) {
        cov[q] = s2 * S[q];
        finite = finite && fabs(cov[q]) < inf;
    }
    *sigma = sqrt((cov[0] + cov[3]) + cov[5]);
    return finite && fabs(*sigma) < inf;
}

}  // namespace mpe
