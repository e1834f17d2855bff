// The host half of mpe_calib_step (include/mpe.h has the rule): per camera, Levenberg-Marquardt over the six numbers of a
// rigid perturbation, from the 28 sums a pass leaves.  Header only, <math.h> only, no HIP: api.hip includes it, and so does
// the stand-alone program tests/native/calib_solve_test.cpp.  harness/calibrate.py states the same in numpy; the
// two give the same delta bit for bit, which is why every sum below has its order written out.  The solve (calib_ldlt) and
// the accept / reject / lambda bookkeeping of a step (calib_lm_step) are written for any number of unknowns: camfit_solve.h
// runs them with thirteen.  C++ (a camera's state derives from calib_lm), compiled by hipcc and by the host compiler.
//
// The sums of a camera: q = 0..20 the upper triangle of A row by row ((0,0) (0,1) .. (0,5) (1,1) .. (5,5)), q = 21..26 g,
// q = 27 the cost C.
//
// calib_solve6: M = A + lambda*diag(A) (M_kk = A_kk + lambda*A_kk, M_kl = A_kl), M delta = -g by unpivoted LDL^T, column
// by column, every inner sum a left fold in increasing index:
//   for j = 0..5:
//     v_k = L_jk * D_k                                   k = 0..j-1
//     D_j = M_jj ; D_j = D_j - L_jk * v_k                k = 0..j-1 in turn
//     D_j > 0 must hold, else the solve fails here
//     for i = j+1..5:
//       t = M_ij ; t = t - L_ik * v_k                    k = 0..j-1 in turn
//       L_ij = t / D_j
//   z_i = -g_i ; z_i = z_i - L_ik * z_k                  i = 0..5, k = 0..i-1 in turn
//   y_i = z_i / D_i
//   delta_i = y_i ; delta_i = delta_i - L_ki * delta_k   i = 5..0, k = i+1..5 in turn
//   every delta_i must be finite, else the solve fails.
// calib_exp: R = I + a*W + b*W*W with W = [w]x, t = |w| = sqrt((w0*w0 + w1*w1) + w2*w2);
//   t < 1e-8: a = 1 - (t*t)/6, b = 0.5 - (t*t)/24; else a = sin(t)/t, s = sin(t/2), b = (2*(s*s))/(t*t).
//   W*W is written out: its (i,j) entry is w_i*w_j off the diagonal and -(the two other squares, lower index first, added)
//   on it.
// calib_compose: E_t = [X R_a | X t_a + tau], X = exp(w), each entry ((X_i0*y_0 + X_i1*y_1) + X_i2*y_2) (+ tau_i).
#pragma once
#include <math.h>

#if defined(__clang__)
#pragma clang fp contract(off)
#endif

#define CALIB_SUMS 28
#define CALIB_MAX_RETRIES 8
#define CALIB_SOLVE_MAX 13             // the most unknowns calib_ldlt solves for (camfit_solve.h has thirteen)

enum {                               // the status bits of include/mpe.h (MPE_CALIB_*), restated so that the header stands alone
    CALIB_HELD = 1,
    CALIB_FEW_OBS = 2,
    CALIB_CONVERGED = 4,
    CALIB_STALLED = 8,
    CALIB_ACCEPTED = 16,
    CALIB_REJECTED = 32
};

// q of A_kl, k <= l, in the upper triangle of order N stored row by row
static inline int calib_tri_of(int N, int k, int l) { return k * N - k * (k - 1) / 2 + (l - k); }
static inline int calib_tri(int k, int l) { return calib_tri_of(6, k, l); }

static inline int calib_finite(double x) { return fabs(x) < HUGE_VAL; }

// The solve above over the unknowns idx_0 < idx_1 < .. < idx_{n-1} of the N a camera has (A the stored triangle of order
// N, g [N]): M_ab = A[idx_a][idx_b], M_aa = A_aa + lambda*A_aa, M y = -g[idx], n in the place of 6.
// -> 1 and y [n], or 0 when a pivot is not > 0 or a y is not finite
static inline int calib_ldlt(const double *A, const double *g, int N, const int *idx, int n, double lambda, double *y) {
    double M[CALIB_SOLVE_MAX][CALIB_SOLVE_MAX], L[CALIB_SOLVE_MAX][CALIB_SOLVE_MAX], D[CALIB_SOLVE_MAX], v[CALIB_SOLVE_MAX], z[CALIB_SOLVE_MAX];
    for (int k = 0; k < n; ++k)
        for (int l = k; l < n; ++l) M[k][l] = M[l][k] = A[calib_tri_of(N, idx[k], idx[l])];
    for (int k = 0; k < n; ++k) M[k][k] = M[k][k] + lambda * M[k][k];
    for (int j = 0; j < n; ++j) {
        for (int k = 0; k < j; ++k) v[k] = L[j][k] * D[k];
        double d = M[j][j];
        for (int k = 0; k < j; ++k) d = d - L[j][k] * v[k];
        if (!(d > 0.0)) return 0;
        D[j] = d;
        for (int i = j + 1; i < n; ++i) {
            double t = M[i][j];
            for (int k = 0; k < j; ++k) t = t - L[i][k] * v[k];
            L[i][j] = t / d;
        }
    }
    for (int i = 0; i < n; ++i) {
        double t = -g[idx[i]];
        for (int k = 0; k < i; ++k) t = t - L[i][k] * z[k];
        z[i] = t;
    }
    for (int i = n - 1; i >= 0; --i) {
        double t = z[i] / D[i];
        for (int k = i + 1; k < n; ++k) t = t - L[k][i] * y[k];
        y[i] = t;
    }
    for (int i = 0; i < n; ++i)
        if (!calib_finite(y[i])) return 0;
    return 1;
}

// -> 1 and delta, or 0 when a pivot is not > 0 or a delta is not finite
static inline int calib_solve6(const double *A, const double *g, double lambda, double *delta) {
    static const int idx[6] = {0, 1, 2, 3, 4, 5};
    return calib_ldlt(A, g, 6, idx, 6, lambda, delta);
}

static inline double calib_norm3(const double *w) { return sqrt((w[0] * w[0] + w[1] * w[1]) + w[2] * w[2]); }

static inline void calib_exp(const double *w, double *R) {
    const double t = calib_norm3(w);
    double a, b;
    if (t < 1e-8) {
        a = 1.0 - (t * t) / 6.0;
        b = 0.5 - (t * t) / 24.0;
    } else {
        const double s = sin(t / 2.0);
        a = sin(t) / t;
        b = (2.0 * (s * s)) / (t * t);
    }
    const double W[9] = {0.0, -w[2], w[1], w[2], 0.0, -w[0], -w[1], w[0], 0.0};
    const double s0 = w[0] * w[0], s1 = w[1] * w[1], s2 = w[2] * w[2];
    const double W2[9] = {-(s1 + s2), w[0] * w[1], w[0] * w[2], w[0] * w[1], -(s0 + s2), w[1] * w[2], w[0] * w[2], w[1] * w[2], -(s0 + s1)};
    for (int i = 0; i < 9; ++i) R[i] = ((i % 4 == 0 ? 1.0 : 0.0) + a * W[i]) + b * W2[i];
}

// E (3 x 4, row major) moved by xi = (w, tau)
static inline void calib_compose(const double *Ea, const double *xi, double *Et) {
    double X[9];
    calib_exp(xi, X);
    for (int i = 0; i < 3; ++i) {
        for (int j = 0; j < 4; ++j)
            Et[4 * i + j] = (X[3 * i] * Ea[j] + X[3 * i + 1] * Ea[4 + j]) + X[3 * i + 2] * Ea[8 + j];
        Et[4 * i + 3] = Et[4 * i + 3] + xi[3 + i];
    }
}

// What a camera carries from step to step whatever its unknowns are; calib_cam and camfit_cam (camfit_solve.h) add their
// sets, the sums at the accepted one and the last perturbation.
struct calib_lm {
    double lambda, cost_start;
    double last_rot, last_trans;     // |w| and |tau| of the last trial built
    long long n_obs;                 // of the first pass
    int status, passes;              // CALIB_* bits; passes taken so far
};

static inline void calib_lm_start(calib_lm *c) {
    c->lambda = 1e-3;
    c->cost_start = c->last_rot = c->last_trans = 0.0;
    c->n_obs = 0;
    c->status = c->passes = 0;
}

enum { CALIB_LM_REFUSED = -1, CALIB_LM_STOPPED, CALIB_LM_HELD, CALIB_LM_FIRST, CALIB_LM_ACCEPTED, CALIB_LM_REJECTED };

// The bookkeeping of one step of one camera: `sums` [n_sums] (the cost last) and n_obs are what the pass at the trial
// left, Aa [n_sums] the sums at the accepted set, held the caller's hold_mask bit.  -> what the caller does with its sets:
//   REFUSED   n_obs is not the first pass's: nothing is changed
//   STOPPED   the camera had converged or stalled: nothing more is changed
//   HELD      held, or fewer than min_obs observations: trial = accepted (Aa = sums, reported, never solved)
//   FIRST     the first pass: accepted = trial, Aa = sums, lambda kept; build a trial
//   ACCEPTED  the cost fell: accepted = trial, Aa = sums, lambda / 10 (at least 1e-12); test convergence, else build a trial
//   REJECTED  the cost did not fall (an equal or NaN cost included): lambda * 10; build a trial
static inline int calib_lm_step(calib_lm *c, double *Aa, int n_sums, const double *sums, long long n_obs, int held, long long min_obs) {
    if (c->passes > 0 && n_obs != c->n_obs) return CALIB_LM_REFUSED;
    const double C = sums[n_sums - 1];
    const int first = c->passes == 0;
    ++c->passes;
    c->status &= ~(CALIB_ACCEPTED | CALIB_REJECTED | CALIB_HELD | CALIB_FEW_OBS);
    if (first) {
        c->n_obs = n_obs;
        c->cost_start = C;
    }
    if (held || c->n_obs < min_obs) {
        c->status |= CALIB_HELD | (c->n_obs < min_obs ? CALIB_FEW_OBS : 0);
        for (int i = 0; i < n_sums; ++i) Aa[i] = sums[i];
        return CALIB_LM_HELD;
    }
    if (c->status & (CALIB_CONVERGED | CALIB_STALLED)) return CALIB_LM_STOPPED;
    if (!first && !(C < Aa[n_sums - 1])) {
        c->status |= CALIB_REJECTED;
        c->lambda = c->lambda * 10.0;
        return CALIB_LM_REJECTED;
    }
    for (int i = 0; i < n_sums; ++i) Aa[i] = sums[i];
    c->status |= CALIB_ACCEPTED;
    if (first) return CALIB_LM_FIRST;
    c->lambda = fmax(c->lambda / 10.0, 1e-12);
    return CALIB_LM_ACCEPTED;
}

static inline int calib_lm_done(const calib_lm *c) { return (c->status & (CALIB_HELD | CALIB_CONVERGED | CALIB_STALLED)) != 0; }

struct calib_cam : calib_lm {
    double Ea[12], Et[12];           // accepted and trial extrinsics
    double Aa[CALIB_SUMS];           // the sums at Ea (A, g, C)
    double delta[6];                 // the perturbation that led from Ea to Et
};

static inline void calib_cam_start(calib_cam *c, const double *E) {
    for (int i = 0; i < 12; ++i) c->Ea[i] = c->Et[i] = E[i];
    for (int i = 0; i < CALIB_SUMS; ++i) c->Aa[i] = 0.0;
    for (int i = 0; i < 6; ++i) c->delta[i] = 0.0;
    calib_lm_start(c);
}

// The trial from the accepted sums: a failed solve multiplies lambda by 10 and retries, at most CALIB_MAX_RETRIES times;
// then the camera is STALLED and its trial is its accepted state.
static inline void calib_cam_trial(calib_cam *c) {
    for (int attempt = 0; attempt <= CALIB_MAX_RETRIES; ++attempt) {
        if (calib_solve6(c->Aa, c->Aa + 21, c->lambda, c->delta)) {
            calib_compose(c->Ea, c->delta, c->Et);
            c->last_rot = calib_norm3(c->delta);
            c->last_trans = calib_norm3(c->delta + 3);
            return;
        }
        if (attempt < CALIB_MAX_RETRIES) c->lambda = c->lambda * 10.0;
    }
    c->status |= CALIB_STALLED;
    for (int i = 0; i < 12; ++i) c->Et[i] = c->Ea[i];
}

// One step of one camera: `sums` and n_obs are what the pass at c->Et left.  held: the caller's hold_mask bit.
// -> 0, or -1 when n_obs is not the first pass's (nothing is changed then).
static inline int calib_cam_step(calib_cam *c, const double *sums, long long n_obs, int held, long long min_obs, double rot_tol,
                                 double trans_tol) {
    const int what = calib_lm_step(c, c->Aa, CALIB_SUMS, sums, n_obs, held, min_obs);
    if (what == CALIB_LM_REFUSED) return -1;
    if (what == CALIB_LM_STOPPED) return 0;
    if (what == CALIB_LM_HELD) {
        for (int i = 0; i < 12; ++i) c->Et[i] = c->Ea[i];
        return 0;
    }
    if (what != CALIB_LM_REJECTED)
        for (int i = 0; i < 12; ++i) c->Ea[i] = c->Et[i];
    if (what == CALIB_LM_ACCEPTED) {
        const double big = fmax(fmax(fabs(c->delta[3]), fabs(c->delta[4])), fabs(c->delta[5]));
        if (calib_norm3(c->delta) < rot_tol && big < trans_tol) {
            c->status |= CALIB_CONVERGED;
            return 0;
        }
    }
    calib_cam_trial(c);
    return 0;
}

static inline int calib_cam_done(const calib_cam *c) { return calib_lm_done(c); }
