// csrc/calib_solve.h on its own, built for the host with -fsanitize=address,undefined (tests/test_calib_host.py):
//   * LDL^T against 6 x 6 systems whose answer is known, and against the residual M delta + g of random ones;
//   * a pivot that is not > 0 (rank-deficient A with lambda = 0, a negative diagonal, NaN);
//   * the retry cap of calib_cam_trial (A = 0: nine failed solves, STALLED, lambda multiplied eight times, trial = accepted);
//   * Rodrigues at |w| = 0, 1e-12, 1e-3 and 3 against the closed form about an axis, and orthonormality of exp(w) R;
//   * the accept / reject / converge bookkeeping of calib_cam_step.
// Prints `tested N bad M`.  With a file name as its argument it also solves the systems of that file (per line 21 + 6 + 1
// + 12 hex floats: A, g, lambda, E_a) and prints per system `sys i stalled lambda delta[6] E_t[12]` as hex floats, for the
// comparison with the numpy statement.
#include <stdio.h>
#include <stdlib.h>
#include <string.h>

#include "calib_solve.h"

static int tested = 0, bad = 0;

static void check(int ok, const char *what) {
    ++tested;
    if (!ok) {
        ++bad;
        printf("FAILED: %s\n", what);
    }
}

static unsigned long long rng_state = 0x9E3779B97F4A7C15ull;
static double uniform() {                     // splitmix64 -> [0, 1)
    unsigned long long z = (rng_state += 0x9E3779B97F4A7C15ull);
    z = (z ^ (z >> 30)) * 0xBF58476D1CE4E5B9ull;
    z = (z ^ (z >> 27)) * 0x94D049BB133111EBull;
    z ^= z >> 31;
    return (double)(z >> 11) / 9007199254740992.0;
}

static void gram(int rows, const double *scale, double *A, double *g) {
    for (int i = 0; i < 21; ++i) A[i] = 0.0;
    for (int i = 0; i < 6; ++i) g[i] = 0.0;
    for (int r = 0; r < rows; ++r) {
        double row[6], res = 6.0 * uniform() - 3.0;
        for (int k = 0; k < 6; ++k) row[k] = (2.0 * uniform() - 1.0) * scale[k];
        for (int k = 0; k < 6; ++k) {
            for (int l = k; l < 6; ++l) A[calib_tri(k, l)] += row[k] * row[l];
            g[k] += row[k] * res;
        }
    }
}

static double residual(const double *A, const double *g, double lambda, const double *delta) {      // max |M delta + g| / scale
    double worst = 0.0;
    for (int k = 0; k < 6; ++k) {
        double s = g[k], mag = fabs(g[k]);
        for (int l = 0; l < 6; ++l) {
            double m = A[k <= l ? calib_tri(k, l) : calib_tri(l, k)];
            if (k == l) m += lambda * m;
            s += m * delta[l];
            mag += fabs(m * delta[l]);
        }
        if (mag > 0.0 && fabs(s) / mag > worst) worst = fabs(s) / mag;
    }
    return worst;
}

static void test_solver() {
    double A[21], g[6], delta[6];
    // diagonal: delta_k = -g_k / (d_k (1 + lambda)), exactly representable with lambda = 1
    for (int i = 0; i < 21; ++i) A[i] = 0.0;
    for (int k = 0; k < 6; ++k) A[calib_tri(k, k)] = (double)(1 << k), g[k] = -(double)(4 << k);
    check(calib_solve6(A, g, 1.0, delta) == 1, "diagonal system solves");
    for (int k = 0; k < 6; ++k) check(delta[k] == 2.0, "diagonal system: delta = 2");
    // M = L D L^T with small integers, lambda = 0: the elimination is exact and so is the answer
    {
        const double L[6][6] = {{1}, {2, 1}, {-1, 3, 1}, {0, 1, -2, 1}, {1, 0, 1, 2, 1}, {-2, 1, 0, 1, 3, 1}};
        const double D[6] = {2, 1, 4, 1, 2, 1}, want[6] = {1, -2, 3, 0, -1, 2};
        double M[6][6];
        for (int i = 0; i < 6; ++i)
            for (int j = 0; j < 6; ++j) {
                M[i][j] = 0.0;
                for (int k = 0; k < 6; ++k) M[i][j] += L[i][k] * D[k] * L[j][k];
            }
        for (int k = 0; k < 6; ++k) {
            for (int l = k; l < 6; ++l) A[calib_tri(k, l)] = M[k][l];
            g[k] = 0.0;
            for (int l = 0; l < 6; ++l) g[k] -= M[k][l] * want[l];
        }
        check(calib_solve6(A, g, 0.0, delta) == 1, "integer L D L^T system solves");
        for (int k = 0; k < 6; ++k) check(delta[k] == want[k], "integer L D L^T system: exact answer");
    }
    // random Gram matrices with a camera's column scales: the residual is at rounding level
    const double scale[6] = {3000., 3000., 3000., 400., 400., 400.};
    for (int t = 0; t < 200; ++t) {
        gram(30, scale, A, g);
        const double lambda = t % 2 ? 1e-3 : 1e-12;
        check(calib_solve6(A, g, lambda, delta) == 1, "random Gram system solves");
        check(residual(A, g, lambda, delta) < 1e-9, "random Gram system: residual");
    }
    // pivots that are not > 0
    gram(3, scale, A, g);                                    // rank 3
    int failed = 0;
    for (int t = 0; t < 50; ++t) {
        gram(3, scale, A, g);
        for (int k = 0; k < 3; ++k)                          // exact rank deficiency: columns 3..5 are zero
            for (int l = 3; l < 6; ++l) A[calib_tri(k, l)] = 0.0;
        for (int k = 3; k < 6; ++k)
            for (int l = k; l < 6; ++l) A[calib_tri(k, l)] = 0.0;
        failed += calib_solve6(A, g, 0.0, delta) == 0;
    }
    check(failed == 50, "a zero pivot fails the solve");
    gram(30, scale, A, g);
    A[calib_tri(2, 2)] = -A[calib_tri(2, 2)];
    check(calib_solve6(A, g, 1e-3, delta) == 0, "a negative diagonal fails the solve");
    gram(30, scale, A, g);
    A[calib_tri(1, 4)] = NAN;
    check(calib_solve6(A, g, 1e-3, delta) == 0, "a NaN entry fails the solve");
    gram(30, scale, A, g);
    g[5] = INFINITY;
    check(calib_solve6(A, g, 1e-3, delta) == 0, "a delta that is not finite fails the solve");
}

static void test_retry_cap() {
    const double E[12] = {1, 0, 0, 0.5, 0, 1, 0, -0.25, 0, 0, 1, 2};
    calib_cam c;
    calib_cam_start(&c, E);
    calib_cam_trial(&c);                                     // A = 0: every pivot is 0 whatever lambda is
    check((c.status & CALIB_STALLED) != 0, "A = 0 stalls");
    double want = 1e-3;
    for (int i = 0; i < CALIB_MAX_RETRIES; ++i) want = want * 10.0;
    check(c.lambda == want, "the retry cap: lambda multiplied eight times");
    check(memcmp(c.Et, c.Ea, sizeof c.Et) == 0, "a stalled camera's trial is its accepted state");
    // a system that needs exactly two retries
    calib_cam_start(&c, E);
    for (int k = 0; k < 6; ++k) c.Aa[calib_tri(k, k)] = 1.0, c.Aa[21 + k] = 1.0;
    c.Aa[calib_tri(0, 1)] = 1.0 + 2e-2;                      // D_1 = (1 + l) - (1.02)^2 / (1 + l) > 0 needs l > 0.02
    c.lambda = 1e-3;
    calib_cam_trial(&c);
    check(!(c.status & CALIB_STALLED) && c.lambda == (1e-3 * 10.0) * 10.0, "two retries, then a trial");
}

static void test_rodrigues() {
    const double mags[4] = {0.0, 1e-12, 1e-3, 3.0};
    const double axes[3][3] = {{1, 0, 0}, {0, 0, 1}, {2.0 / 7.0, -3.0 / 7.0, 6.0 / 7.0}};
    for (int m = 0; m < 4; ++m)
        for (int a = 0; a < 3; ++a) {
            double w[3], R[9];
            for (int i = 0; i < 3; ++i) w[i] = axes[a][i] * mags[m];
            calib_exp(w, R);
            const double c = cos(mags[m]), s = sin(mags[m]);
            double worst = 0.0;
            for (int i = 0; i < 3; ++i)
                for (int j = 0; j < 3; ++j) {
                    const double n[3] = {axes[a][0], axes[a][1], axes[a][2]};
                    const double cross = i == j ? 0.0 : ((j - i + 3) % 3 == 1 ? -n[3 - i - j] : n[3 - i - j]);
                    const double want = c * (i == j) + (1.0 - c) * n[i] * n[j] + s * cross;
                    worst = fmax(worst, fabs(R[3 * i + j] - want));
                }
            check(worst < 1e-15, "Rodrigues against the closed form");      // a few ulp of entries <= 2
            if (mags[m] == 0.0)
                for (int i = 0; i < 9; ++i) check(R[i] == (i % 4 == 0 ? 1.0 : 0.0), "exp(0) is the identity, exactly");
        }
    // exp(w) R stays orthonormal through many compositions
    double E[12] = {1, 0, 0, 0.1, 0, 1, 0, 0.2, 0, 0, 1, 0.3};
    double worst = 0.0;
    for (int t = 0; t < 200; ++t) {
        double xi[6], Et[12];
        const double mag = mags[t % 4];
        for (int i = 0; i < 3; ++i) xi[i] = 2.0 * uniform() - 1.0;
        const double n = calib_norm3(xi);
        for (int i = 0; i < 3; ++i) xi[i] = xi[i] / n * mag, xi[3 + i] = 0.01 * (2.0 * uniform() - 1.0);
        calib_compose(E, xi, Et);
        memcpy(E, Et, sizeof E);
        for (int i = 0; i < 3; ++i)
            for (int j = 0; j < 3; ++j) {
                double d = 0.0;
                for (int k = 0; k < 3; ++k) d += E[4 * i + k] * E[4 * j + k];
                worst = fmax(worst, fabs(d - (i == j)));
            }
    }
    check(worst < 1e-13, "exp(w) R is orthonormal after 200 compositions");
    // the translation: exp(w) t + tau with w = 0
    const double E0[12] = {0, -1, 0, 1.5, 1, 0, 0, -2.5, 0, 0, 1, 4}, xi0[6] = {0, 0, 0, 0.25, -0.5, 1};
    double Et[12];
    calib_compose(E0, xi0, Et);
    check(Et[3] == 1.75 && Et[7] == -3.0 && Et[11] == 5.0 && Et[1] == -1.0 && Et[4] == 1.0, "compose with w = 0");
}

static void test_step() {
    const double scale[6] = {3000., 3000., 3000., 400., 400., 400.};
    const double E[12] = {1, 0, 0, 0.5, 0, 1, 0, -0.25, 0, 0, 1, 2};
    double sums[CALIB_SUMS];
    calib_cam c;
    calib_cam_start(&c, E);
    gram(30, scale, sums, sums + 21);
    sums[27] = 100.0;
    check(calib_cam_step(&c, sums, 30, 0, 6, 0.0, 0.0) == 0 && (c.status & CALIB_ACCEPTED) && c.lambda == 1e-3 && c.cost_start == 100.0,
          "the first pass is accepted and keeps lambda");
    double Ea[12], Et[12];
    memcpy(Ea, c.Ea, sizeof Ea);
    memcpy(Et, c.Et, sizeof Et);
    check(memcmp(Ea, E, sizeof Ea) == 0 && memcmp(Et, E, sizeof Et) != 0, "the first trial moves");
    sums[27] = 100.0;                                        // not below: rejected (strict)
    calib_cam_step(&c, sums, 30, 0, 6, 0.0, 0.0);
    check((c.status & CALIB_REJECTED) && c.lambda == 1e-3 * 10.0 && memcmp(c.Ea, Ea, sizeof Ea) == 0 && c.Aa[27] == 100.0,
          "an equal cost is rejected, lambda grows, the accepted state stays");
    sums[27] = NAN;
    calib_cam_step(&c, sums, 30, 0, 6, 0.0, 0.0);
    check((c.status & CALIB_REJECTED) && c.Aa[27] == 100.0, "a NaN cost is rejected");
    memcpy(Et, c.Et, sizeof Et);
    sums[27] = 50.0;
    const double lam = c.lambda;
    calib_cam_step(&c, sums, 30, 0, 6, 0.0, 0.0);
    check((c.status & CALIB_ACCEPTED) && memcmp(c.Ea, Et, sizeof Et) == 0 && c.lambda == fmax(lam / 10.0, 1e-12) && c.Aa[27] == 50.0,
          "a lower cost is accepted: the trial becomes the accepted state");
    check(calib_cam_step(&c, sums, 29, 0, 6, 0.0, 0.0) == -1 && c.passes == 4, "another n_obs is refused and changes nothing");
    sums[27] = 25.0;
    calib_cam_step(&c, sums, 30, 0, 6, 1e9, 1e9);
    check((c.status & CALIB_CONVERGED) && calib_cam_done(&c), "a small accepted step converges");
    memcpy(Et, c.Et, sizeof Et);
    sums[27] = 1.0;
    calib_cam_step(&c, sums, 30, 0, 6, 1e9, 1e9);
    check(memcmp(c.Et, Et, sizeof Et) == 0 && c.Aa[27] == 25.0, "a camera that stopped is left alone");
    calib_cam_start(&c, E);
    calib_cam_step(&c, sums, 5, 0, 6, 0.0, 0.0);
    check(c.status == (CALIB_HELD | CALIB_FEW_OBS) && memcmp(c.Et, E, sizeof Et) == 0 && c.Aa[27] == 1.0, "fewer than min_obs observations: held");
    calib_cam_start(&c, E);
    calib_cam_step(&c, sums, 30, 1, 6, 0.0, 0.0);
    check(c.status == CALIB_HELD && memcmp(c.Et, E, sizeof Et) == 0, "hold_mask: held");
}

int main(int argc, char **argv) {
    test_solver();
    test_retry_cap();
    test_rodrigues();
    test_step();
    if (argc > 1) {
        FILE *fh = fopen(argv[1], "r");
        if (!fh) {
            printf("cannot open %s\n", argv[1]);
            return 2;
        }
        char tok[64];
        for (int n = 0;; ++n) {
            double v[40];
            int got = 0;
            while (got < 40 && fscanf(fh, "%63s", tok) == 1) v[got++] = strtod(tok, NULL);
            if (got < 40) break;
            calib_cam c;
            calib_cam_start(&c, v + 28);
            for (int i = 0; i < 27; ++i) c.Aa[i] = v[i];
            c.lambda = v[27];
            calib_cam_trial(&c);
            printf("sys %d %d %a", n, (c.status & CALIB_STALLED) != 0, c.lambda);
            for (int i = 0; i < 6; ++i) printf(" %a", c.delta[i]);
            for (int i = 0; i < 12; ++i) printf(" %a", c.Et[i]);
            printf("\n");
        }
        fclose(fh);
    }
    printf("tested %d bad %d\n", tested, bad);
    return bad ? 1 : 0;
}
