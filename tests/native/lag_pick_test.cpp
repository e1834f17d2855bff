// csrc/lag_pick.h on the host (tests/test_lag_host.py builds this with -ffp-contract=off under the sanitizers and compares
// every output bit with harness/lag.py).  Reads one file of doubles, writes one, and prints every result as hex floats:
//
//   in:  n | n curves: W sub min_obs, cost[K], n_obs[K] (K = 2*W*sub + 1; counts as doubles)
//   out: per curve: status k_best lag_grid lag_refined cost_best cost_zero n_obs
#include <stdio.h>
#include <stdlib.h>

#include <vector>

#include "lag_pick.h"

int main(int argc, char **argv) {
    if (argc != 3) return 2;
    FILE *fh = fopen(argv[1], "rb");
    if (!fh) return 2;
    std::vector<double> in;
    double buf[1024];
    for (size_t n; (n = fread(buf, sizeof(double), 1024, fh)) > 0;) in.insert(in.end(), buf, buf + n);
    fclose(fh);
    size_t at = 0;
    auto next = [&]() {
        if (at >= in.size()) {
            fprintf(stderr, "input ends early\n");
            exit(3);
        }
        return in[at++];
    };
    const int n = (int)next();
    std::vector<double> out;
    for (int q = 0; q < n; ++q) {
        const int W = (int)next(), sub = (int)next();
        const int64_t min_obs = (int64_t)next();
        if (W < 0 || W > 8 || sub < 1 || sub > 8) return 3;
        const int K = 2 * W * sub + 1;
        std::vector<double> cost(K);
        std::vector<int64_t> cnt(K);
        for (double &v : cost) v = next();
        for (int64_t &v : cnt) v = (int64_t)next();
        const lag_pick_result r = lag_pick(cost.data(), cnt.data(), W, sub, min_obs);
        out.insert(out.end(), {(double)r.status, (double)r.k_best, r.lag_grid, r.lag_refined, r.cost_best, r.cost_zero, (double)r.n_obs});
        printf("curve %d: status %d k %d grid %a refined %a best %a zero %a n %lld\n", q, r.status, r.k_best, r.lag_grid, r.lag_refined,
               r.cost_best, r.cost_zero, (long long)r.n_obs);
    }
    if (at != in.size()) return 3;
    fh = fopen(argv[2], "wb");
    if (!fh || fwrite(out.data(), sizeof(double), out.size(), fh) != out.size()) return 2;
    fclose(fh);
    printf("done %d curves\n", n);
    return 0;
}
