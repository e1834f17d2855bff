// csrc/camfit_solve.h on its own, built for the host with -fsanitize=address,undefined (tests/test_camfit_host.py):
//   * with only the pose group free camfit_solve gives calib_solve6's delta bit for bit, the held unknowns 0;
//   * a reduced solve leaves a small residual M delta + g on its rows; a pivot that is not > 0 fails and zeroes delta;
//   * the retry cap of camfit_cam_trial (A = 0: nine failed solves, STALLED, lambda multiplied eight times, trial = accepted);
//   * a step that would make fx negative counts as a failed solve;
//   * a trial that rounds back onto the accepted float32 numbers is CONVERGED;
//   * what a held group keeps.
// Prints `self-checks N bad M`.  With a file name as its argument it replays the cameras of that file -- `cam free_mask
// min_obs passes E[12] k[4] dist[5] tols[4]`, then per pass `pass n_obs sums[105]`, hex floats -- through
// camfit_cam_step and prints after every step `step status passes lambda delta[13] trial(E[12] k[4] dist[5])
// accepted(E[12] k[4] dist[5]) last_rot last_trans last_pix last_lens` as hex floats, for the comparison with the numpy
// statement.
#include <stdio.h>
#include <stdlib.h>
#include <string.h>

#include "camfit_solve.h"

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

static const double SCALE[CAMFIT_N] = {3000., 3000., 3000., 400., 400., 400., 0.3, 0.3, 1.0, 1.0, 40.0, 8.0, 2.0};

static void gram(int rows, double *sums) {
    for (int i = 0; i < CAMFIT_SUMS; ++i) sums[i] = 0.0;
    for (int r = 0; r < rows; ++r) {
        double row[CAMFIT_N], res = 6.0 * uniform() - 3.0;
        for (int k = 0; k < CAMFIT_N; ++k) row[k] = (2.0 * uniform() - 1.0) * SCALE[k];
        for (int k = 0; k < CAMFIT_N; ++k) {
            for (int l = k; l < CAMFIT_N; ++l) sums[camfit_tri(k, l)] += row[k] * row[l];
            sums[CAMFIT_G + k] += row[k] * res;
        }
        sums[CAMFIT_C] += res * res;
    }
}

static double residual(const double *sums, double lambda, unsigned mask, const double *delta) {      // max |M delta + g| / scale on the free rows
    int idx[CAMFIT_N];
    const int n = camfit_free(mask, idx);
    double worst = 0.0;
    for (int a = 0; a < n; ++a) {
        const int k = idx[a];
        double s = sums[CAMFIT_G + k], mag = fabs(s);
        for (int b = 0; b < n; ++b) {
            const int l = idx[b];
            double m = sums[k <= l ? camfit_tri(k, l) : camfit_tri(l, k)];
            if (k == l) m += lambda * m;
            s += m * delta[l];
            mag += fabs(m * delta[l]);
        }
        if (mag > 0.0 && fabs(s) / mag > worst) worst = fabs(s) / mag;
    }
    return worst;
}

static void start(camfit_cam *c) {
    const double E[12] = {1, 0, 0, 0.1, 0, 1, 0, -0.2, 0, 0, 1, 3.0};
    const float k[4] = {1400.0f, 1395.5f, 960.25f, 540.5f};
    const double dist[5] = {-0.27, 0.18, 0.009, 0.01, -0.03};
    camfit_cam_start(c, E, k, dist);
}

static void self_checks() {
    double sums[CAMFIT_SUMS], delta[CAMFIT_N], d6[6];
    for (int i = 0; i < 8; ++i) {
        gram(60, sums);
        // the pose block as calib_solve6 sees it
        double A6[21], g6[6];
        for (int k = 0; k < 6; ++k) {
            for (int l = k; l < 6; ++l) A6[calib_tri(k, l)] = sums[camfit_tri(k, l)];
            g6[k] = sums[CAMFIT_G + k];
        }
        const int ok6 = calib_solve6(A6, g6, 1e-3, d6), ok = camfit_solve(sums, sums + CAMFIT_G, 1e-3, CAMFIT_POSE, delta);
        check(ok6 && ok && !memcmp(d6, delta, sizeof d6), "pose only: calib_solve6's delta, bit for bit");
        int zeros = 1;
        for (int k = 6; k < CAMFIT_N; ++k) zeros &= delta[k] == 0.0;
        check(zeros, "pose only: the held unknowns stay 0");
        const unsigned masks[4] = {CAMFIT_ALL, CAMFIT_FOCAL | CAMFIT_CENTRE, CAMFIT_POSE | CAMFIT_K1 | CAMFIT_K3, CAMFIT_K2};
        for (int m = 0; m < 4; ++m) {
            check(camfit_solve(sums, sums + CAMFIT_G, 0.01, masks[m], delta) && residual(sums, 0.01, masks[m], delta) < 1e-9, "reduced solve: residual");
        }
    }
    gram(60, sums);
    sums[camfit_tri(6, 7)] = 1.02 * sqrt(sums[camfit_tri(6, 6)] * sums[camfit_tri(7, 7)]);
    delta[3] = 7.0;
    check(!camfit_solve(sums, sums + CAMFIT_G, 0.0, CAMFIT_FOCAL, delta) && delta[3] == 0.0 && delta[6] == 0.0, "a pivot that is not > 0: no step, delta zeroed");
    check(camfit_solve(sums, sums + CAMFIT_G, 0.0, CAMFIT_POSE, delta), "... and the held rows are left out");
    // the retry cap
    camfit_cam c;
    start(&c);
    for (int i = 0; i < CAMFIT_SUMS; ++i) c.Aa[i] = 0.0;
    camfit_cam_trial(&c, CAMFIT_ALL);
    check((c.status & CALIB_STALLED) && fabs(c.lambda - 1e5) < 1e-6 && !memcmp(&c.a, &c.t, sizeof c.a), "A = 0: STALLED after eight retries, trial = accepted");
    // a step to a negative focal length is a failed solve: A_66 = 1, g_6 = 2000 -> delta_6 = -2000 / (1 + lambda) until lambda grows
    start(&c);
    c.Aa[camfit_tri(6, 6)] = c.Aa[camfit_tri(7, 7)] = 1.0;
    c.Aa[CAMFIT_G + 6] = 2000.0;
    camfit_cam_trial(&c, CAMFIT_FOCAL);
    check(!(c.status & CALIB_STALLED) && c.t.k[0] > 0.0f && c.t.k[0] < 500.0f && fabs(c.lambda - 1.0) < 1e-12,
          "a trial with fx <= 0 is a failed solve: lambda grows to 1, fx = 1400 - 1000");
    // a step below half a float32 spacing rounds back: CONVERGED
    start(&c);
    c.Aa[camfit_tri(8, 8)] = c.Aa[camfit_tri(9, 9)] = 1.0;
    c.Aa[CAMFIT_G + 8] = 1e-6;                   // delta_8 ~ -1e-6 px on cx = 960.25 (spacing 6.1e-5)
    camfit_cam_trial(&c, CAMFIT_CENTRE);
    check((c.status & CALIB_CONVERGED) && c.t.k[2] == c.a.k[2] && c.delta[8] < 0.0 && c.last_pix > 0.0, "a trial equal to the accepted set: CONVERGED");
    start(&c);
    c.Aa[camfit_tri(10, 10)] = 1.0;
    c.Aa[CAMFIT_G + 10] = -0.5;
    camfit_cam_trial(&c, CAMFIT_K1);
    check(!(c.status & CALIB_CONVERGED) && c.t.dist[0] > c.a.dist[0] && c.t.dist[2] == c.a.dist[2] && c.t.dist[3] == c.a.dist[3] && c.t.k[0] == c.a.k[0] &&
              !memcmp(c.t.E, c.a.E, sizeof c.t.E),
          "K1 alone: kd0 moves, the tangential terms, K and the extrinsics are carried");
}

static int read_hex(FILE *fh, double *out, int n) {
    for (int i = 0; i < n; ++i) {
        char tok[64];
        if (fscanf(fh, "%63s", tok) != 1) return 0;
        out[i] = strtod(tok, NULL);
    }
    return 1;
}

static void print_set(const camfit_set *s) {
    for (int i = 0; i < 12; ++i) printf(" %a", s->E[i]);
    for (int i = 0; i < 4; ++i) printf(" %a", (double)s->k[i]);
    for (int i = 0; i < 5; ++i) printf(" %a", s->dist[i]);
}

static int replay(const char *path) {
    FILE *fh = fopen(path, "r");
    if (!fh) return 1;
    char word[16];
    while (fscanf(fh, "%15s", word) == 1) {
        if (strcmp(word, "cam")) return 1;
        unsigned mask;
        long long min_obs;
        int passes;
        double v[25];
        if (fscanf(fh, "%u %lld %d", &mask, &min_obs, &passes) != 3 || !read_hex(fh, v, 25)) return 1;
        float k[4] = {(float)v[12], (float)v[13], (float)v[14], (float)v[15]};
        camfit_cam c;
        camfit_cam_start(&c, v, k, v + 16);
        const camfit_rule rule = {v[21], v[22], v[23], v[24], min_obs, mask};
        for (int p = 0; p < passes; ++p) {
            long long n_obs;
            double sums[CAMFIT_SUMS];
            if (fscanf(fh, "%15s %lld", word, &n_obs) != 2 || strcmp(word, "pass") || !read_hex(fh, sums, CAMFIT_SUMS)) return 1;
            if (camfit_cam_step(&c, sums, n_obs, 0, &rule)) return 1;
            printf("step %d %d %a", c.status, c.passes, c.lambda);
            for (int i = 0; i < CAMFIT_N; ++i) printf(" %a", c.delta[i]);
            print_set(&c.t);
            print_set(&c.a);
            printf(" %a %a %a %a\n", c.last_rot, c.last_trans, c.last_pix, c.last_lens);
        }
    }
    fclose(fh);
    return 0;
}

int main(int argc, char **argv) {
    self_checks();
    printf("self-checks %d bad %d\n", tested, bad);
    if (argc > 1 && replay(argv[1])) {
        printf("could not replay %s\n", argv[1]);
        return 2;
    }
    return bad ? 1 : 0;
}
