// csrc/cov3.h on the host (tests/test_posecov_host.py builds this with -ffp-contract=off under the sanitizers and compares
// every output bit with harness/uncertainty.py).  Reads one file of doubles, writes one:
//
//   in:  nS | nS systems: A[6] (00 01 02 11 12 22) s2
//   out: per system: S[6] pivots cov[6] sigma finite
#include <stdio.h>
#include <stdlib.h>

#include <vector>

#include "cov3.h"

int main(int argc, char **argv) {
    if (argc != 3) return 2;
    FILE *fh = fopen(argv[1], "rb");
    if (!fh) return 2;
    std::vector<double> in;
    double buf[1024];
    for (size_t n; (n = fread(buf, sizeof(double), 1024, fh)) > 0;) in.insert(in.end(), buf, buf + n);
    fclose(fh);
    if (in.empty()) return 3;
    const size_t nS = (size_t)in[0];
    if (in.size() != 1 + 7 * nS) return 3;
    std::vector<double> out;
    for (size_t s = 0; s < nS; ++s) {
        // every system in a heap buffer of exactly its size: a read past A[5] is the sanitizer's
        double *A = new double[6];
        for (int q = 0; q < 6; ++q) A[q] = in[1 + 7 * s + q];
        double *S = new double[6], *cov = new double[6], sigma;
        const bool pivots = mpe::cov3_inverse(A, S);
        const bool finite = mpe::cov3_finish(S, in[1 + 7 * s + 6], cov, &sigma);
        out.insert(out.end(), S, S + 6);
        out.push_back(pivots ? 1.0 : 0.0);
        out.insert(out.end(), cov, cov + 6);
        out.push_back(sigma);
        out.push_back(finite ? 1.0 : 0.0);
        delete[] A;
        delete[] S;
        delete[] cov;
    }
    fh = fopen(argv[2], "wb");
    if (!fh || fwrite(out.data(), sizeof(double), out.size(), fh) != out.size()) return 2;
    fclose(fh);
    printf("done %zu systems\n", nS);
    return 0;
}
