// The host half of mpe_lag_estimate (include/mpe.h has the rule): per camera, the grid entry of least mean cost and the
// parabola through its neighbours, from the K sums and counts a pass leaves.  Header only, <math.h> and <stdint.h> only, no
// HIP: api.hip includes it, and so does the stand-alone program tests/native/lag_pick_test.cpp.  harness/lag.py states the
// same on Python floats; the two give the same numbers bit for bit, which is why every line below is one rounding.
//
//   valid_i = n_obs_i >= min_obs ; m_i = cost_i / (double)n_obs_i
//   i* = the lowest valid index whose m is least; a NaN is never least (with nothing but NaN: the lowest valid index)
//   edge: i* = 0, i* = K-1 or a neighbour that is not valid -> refined = grid
//   den = (m_{i*-1} - m_{i*}) + (m_{i*+1} - m_{i*}) ; den > 0: off = (0.5 * (m_{i*-1} - m_{i*+1})) / den within -0.5 .. 0.5
//   otherwise, or when off is a NaN, off = 0 (flat)
//   k* = i* - W*sub ; lag_grid = (double)k* / (double)sub ; lag_refined = ((double)k* + off) / (double)sub
#pragma once
#include <math.h>
#include <stdint.h>

#if defined(__clang__)
#pragma clang fp contract(off)
#endif

enum {                               // the status bits of include/mpe.h (MPE_LAG_*), restated so that the header stands alone
    LAG_FEW_OBS = 1,
    LAG_EDGE = 2,
    LAG_FLAT = 4
};

struct lag_pick_result {
    int status, k_best;
    double lag_grid, lag_refined, cost_best, cost_zero;
    int64_t n_obs;
};

// the mean cost of entry i; only asked of a valid entry
inline double lag_mean(const double *cost, const int64_t *n_obs, int i) { return cost[i] / (double)n_obs[i]; }

// cost [K], n_obs [K] of one camera, K = 2*W*sub + 1
inline lag_pick_result lag_pick(const double *cost, const int64_t *n_obs, int W, int sub, int64_t min_obs) {
    const int K = 2 * W * sub + 1, zero = W * sub;
    const double nan = __builtin_nan("");
    lag_pick_result r = {0, 0, 0.0, 0.0, nan, nan, 0};
    int best = -1;
    double m_best = nan;
    for (int i = 0; i < K; ++i) {
        if (n_obs[i] < min_obs) continue;
        const double m = lag_mean(cost, n_obs, i);
        if (best < 0 || m < m_best || (m_best != m_best && m == m)) best = i, m_best = m;
    }
    if (best < 0) {
        r.status = LAG_FEW_OBS;
        return r;
    }
    r.k_best = best - zero;
    r.cost_best = m_best;
    r.n_obs = n_obs[best];
    if (n_obs[zero] >= min_obs) r.cost_zero = lag_mean(cost, n_obs, zero);
    r.lag_grid = (double)r.k_best / (double)sub;
    r.lag_refined = r.lag_grid;
    if (best == 0 || best == K - 1 || n_obs[best - 1] < min_obs || n_obs[best + 1] < min_obs) {
        r.status = LAG_EDGE;
        return r;
    }
    const double lo = lag_mean(cost, n_obs, best - 1), hi = lag_mean(cost, n_obs, best + 1);
    const double den = (lo - m_best) + (hi - m_best);
    double off = 0.0;
    if (den > 0.0) {
        off = (0.5 * (lo - hi)) / den;
        if (off > 0.5) off = 0.5;
        if (off < -0.5) off = -0.5;
        if (off != off) off = 0.0, r.status = LAG_FLAT;      // both neighbours infinite: inf - inf
    } else {
        r.status = LAG_FLAT;
    }
    r.lag_refined = ((double)r.k_best + off) / (double)sub;
    return r;
}
