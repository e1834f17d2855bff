// The host half of mpe_camfit_step (include/mpe.h has the rule): per camera, Levenberg-Marquardt over the thirteen unknowns
// of the camera fit -- the six numbers of a rigid perturbation, fx, fy, cx, cy and the three radial lens terms -- from the
// 105 sums a pass leaves.  Header only, <math.h> and <string.h> only, no HIP: api.hip includes it, and so does the
// stand-alone program tests/native/camfit_solve_test.cpp.  harness/camfit.py states the same in numpy; the two give the
// same delta and the same trial set bit for bit (the extrinsics to libm's sin), which is why every sum below has its
// order written out.  calib_exp, calib_compose and calib_norm3 are calib_solve.h's.
//
// The sums of a camera: q = 0..90 the upper triangle of A row by row ((0,0) (0,1) .. (0,12) (1,1) .. (12,12)), q = 91..103
// g, q = 104 the cost C.
//
// camfit_solve: idx_0 < idx_1 < .. < idx_{n-1} the free unknowns (free_mask), M_ab = A[idx_a][idx_b], M_aa = A_aa +
// lambda*A_aa, M y = -g[idx] by calib_ldlt, the unpivoted LDL^T of calib_solve6 with n in the place of 6, every inner sum a
// left fold in increasing index; delta[idx_a] = y_a, delta of a held unknown = 0.0.  With only the pose group free n = 6
// and idx = 0..5: calib_solve6's call.  The step is calib_lm_step's bookkeeping around this file's sets.
#pragma once
#include <math.h>
#include <string.h>

#include "calib_solve.h"

#if defined(__clang__)
#pragma clang fp contract(off)
#endif

#define CAMFIT_N 13
#define CAMFIT_SUMS 105
#define CAMFIT_G 91                  // q of g_0
#define CAMFIT_C 104                 // q of the cost
static_assert(CAMFIT_N <= CALIB_SOLVE_MAX, "calib_ldlt holds thirteen unknowns");

enum {                               // the groups of include/mpe.h (MPE_CAMFIT_*), restated so that the header stands alone
    CAMFIT_POSE = 1,
    CAMFIT_FOCAL = 2,
    CAMFIT_CENTRE = 4,
    CAMFIT_K1 = 8,
    CAMFIT_K2 = 16,
    CAMFIT_K3 = 32,
    CAMFIT_ALL = 63
};

static inline int camfit_tri(int k, int l) { return k * CAMFIT_N - k * (k - 1) / 2 + (l - k); }       // q of A_kl, k <= l

// the free unknowns of free_mask in ascending order -> their number
static inline int camfit_free(unsigned free_mask, int *idx) {
    static const unsigned char group[CAMFIT_N] = {CAMFIT_POSE, CAMFIT_POSE, CAMFIT_POSE, CAMFIT_POSE, CAMFIT_POSE, CAMFIT_POSE, CAMFIT_FOCAL,
                                                  CAMFIT_FOCAL, CAMFIT_CENTRE, CAMFIT_CENTRE, CAMFIT_K1, CAMFIT_K2, CAMFIT_K3};
    int n = 0;
    for (int k = 0; k < CAMFIT_N; ++k)
        if (free_mask & group[k]) idx[n++] = k;
    return n;
}

// -> 1 and delta [13], or 0 when a pivot is not > 0 or a delta is not finite (delta is all zero then)
static inline int camfit_solve(const double *A, const double *g, double lambda, unsigned free_mask, double *delta) {
    double y[CAMFIT_N];
    int idx[CAMFIT_N];
    const int n = camfit_free(free_mask, idx);
    for (int k = 0; k < CAMFIT_N; ++k) delta[k] = 0.0;
    if (!calib_ldlt(A, g, CAMFIT_N, idx, n, lambda, y)) return 0;
    for (int i = 0; i < n; ++i) delta[idx[i]] = y[i];
    return 1;
}

// One set of a camera: what a pass is taken at.
typedef struct {
    double E[12];                    // extrinsics, 3 x 4 row major
    float k[4];                      // fx, fy, cx, cy
    double dist[5];                  // kd0, kd1, p1, p2, kd2: [2] and [3] are carried, never read
} camfit_set;

// What a camera carries from step to step.
struct camfit_cam : calib_lm {
    camfit_set a, t;                 // accepted and trial
    double Aa[CAMFIT_SUMS];          // the sums at the accepted set (A, g, C)
    double delta[CAMFIT_N];          // the step that led from a to t
    double last_pix, last_lens;      // of the last trial built: max |delta_6..9| and max |delta_10..12|
};

static inline void camfit_cam_start(camfit_cam *c, const double *E, const float *k, const double *dist) {
    for (int i = 0; i < 12; ++i) c->a.E[i] = E[i];
    for (int i = 0; i < 4; ++i) c->a.k[i] = k[i];
    for (int i = 0; i < 5; ++i) c->a.dist[i] = dist[i];
    c->t = c->a;
    for (int i = 0; i < CAMFIT_SUMS; ++i) c->Aa[i] = 0.0;
    for (int i = 0; i < CAMFIT_N; ++i) c->delta[i] = 0.0;
    calib_lm_start(c);
    c->last_pix = c->last_lens = 0.0;
}

static inline double camfit_max_abs(const double *x, int n) {
    double m = 0.0;
    for (int i = 0; i < n; ++i) m = fmax(m, fabs(x[i]));
    return m;
}

// t = a moved by delta: the extrinsics by calib_compose when the pose group is free, a free intrinsic as
// (float)((double)k_a + delta), a free lens term as kd_a + delta; everything else copied.  -> 1, or 0 when fx or fy of
// the result is not finite or is <= 0
static inline int camfit_compose(const camfit_set *a, const double *delta, unsigned free_mask, camfit_set *t) {
    int idx[CAMFIT_N];
    const int n = camfit_free(free_mask, idx);
    *t = *a;
    if (free_mask & CAMFIT_POSE) calib_compose(a->E, delta, t->E);
    for (int i = 0; i < n; ++i) {
        const int u = idx[i];
        if (u >= 6 && u < 10) t->k[u - 6] = (float)((double)a->k[u - 6] + delta[u]);
        if (u >= 10) t->dist[u == 12 ? 4 : u - 10] = a->dist[u == 12 ? 4 : u - 10] + delta[u];
    }
    for (int i = 0; i < 2; ++i)
        if (!(fabsf(t->k[i]) < HUGE_VALF) || !(t->k[i] > 0.0f)) return 0;
    return 1;
}

// the free unknowns of the two sets have the same bits
static inline int camfit_same(const camfit_set *a, const camfit_set *t, unsigned free_mask) {
    if ((free_mask & CAMFIT_POSE) && memcmp(a->E, t->E, sizeof a->E)) return 0;
    if ((free_mask & CAMFIT_FOCAL) && memcmp(a->k, t->k, 2 * sizeof(float))) return 0;
    if ((free_mask & CAMFIT_CENTRE) && memcmp(a->k + 2, t->k + 2, 2 * sizeof(float))) return 0;
    if ((free_mask & CAMFIT_K1) && memcmp(a->dist, t->dist, sizeof(double))) return 0;
    if ((free_mask & CAMFIT_K2) && memcmp(a->dist + 1, t->dist + 1, sizeof(double))) return 0;
    if ((free_mask & CAMFIT_K3) && memcmp(a->dist + 4, t->dist + 4, sizeof(double))) return 0;
    return 1;
}

// The trial from the accepted sums: a failed solve or a trial without a positive finite focal length multiplies lambda by
// 10 and retries, at most CALIB_MAX_RETRIES times; then the camera is STALLED and its trial is its accepted set.  A trial
// that equals the accepted set in every free unknown, bit for bit, is CONVERGED: the rounding left nothing to move.
static inline void camfit_cam_trial(camfit_cam *c, unsigned free_mask) {
    for (int attempt = 0; attempt <= CALIB_MAX_RETRIES; ++attempt) {
        if (camfit_solve(c->Aa, c->Aa + CAMFIT_G, c->lambda, free_mask, c->delta) && camfit_compose(&c->a, c->delta, free_mask, &c->t)) {
            c->last_rot = calib_norm3(c->delta);
            c->last_trans = calib_norm3(c->delta + 3);
            c->last_pix = camfit_max_abs(c->delta + 6, 4);
            c->last_lens = camfit_max_abs(c->delta + 10, 3);
            if (camfit_same(&c->a, &c->t, free_mask)) c->status |= CALIB_CONVERGED;
            return;
        }
        if (attempt < CALIB_MAX_RETRIES) c->lambda = c->lambda * 10.0;
    }
    c->status |= CALIB_STALLED;
    c->t = c->a;
}

typedef struct {
    double rot_tol, trans_tol, pix_tol, lens_tol;
    long long min_obs;
    unsigned free_mask;
} camfit_rule;

// One step of one camera: `sums` and n_obs are what the pass at c->t left.  held: the caller's hold_mask bit.
// -> 0, or -1 when n_obs is not the first pass's (nothing is changed then).
static inline int camfit_cam_step(camfit_cam *c, const double *sums, long long n_obs, int held, const camfit_rule *r) {
    const int what = calib_lm_step(c, c->Aa, CAMFIT_SUMS, sums, n_obs, held, r->min_obs);
    if (what == CALIB_LM_REFUSED) return -1;
    if (what == CALIB_LM_STOPPED) return 0;
    if (what == CALIB_LM_HELD) {
        c->t = c->a;
        return 0;
    }
    if (what != CALIB_LM_REJECTED) c->a = c->t;
    if (what == CALIB_LM_ACCEPTED && calib_norm3(c->delta) < r->rot_tol && camfit_max_abs(c->delta + 3, 3) < r->trans_tol &&
        camfit_max_abs(c->delta + 6, 4) < r->pix_tol && camfit_max_abs(c->delta + 10, 3) < r->lens_tol) {
        c->status |= CALIB_CONVERGED;
        return 0;
    }
    camfit_cam_trial(c, r->free_mask);
    return 0;
}
