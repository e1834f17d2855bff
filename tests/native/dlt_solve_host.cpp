// csrc/dlt_solve.h on the host (tests/test_dlt_solver_host.py builds this with the sanitizers and runs it as a child process).
//   dlt_solve_host solve IN OUT   IN: n x 28 f64 (P1[12], P2[12], x1, y1, x2, y2)   OUT: n x 4 f64 (X, Y, Z, sweeps used)
//   dlt_solve_host rot   IN OUT   IN: n x 3  f64 (al, be, ga)                       OUT: n x 2 f64 (c, s of dlt_rotation)
// -DMPE_DLT_COARSE_ESTIMATES: the rsq / rcp estimates rounded to 24 bits, so that the Newton steps have something to do.
#include <cstdio>
#include <cstring>
#include <vector>

#include "dlt_solve.h"

static bool read_all(const char *path, std::vector<double> *v) {
    FILE *f = fopen(path, "rb");
    if (!f) return false;
    fseek(f, 0, SEEK_END);
    const long bytes = ftell(f);
    fseek(f, 0, SEEK_SET);
    v->resize(bytes > 0 ? (size_t)bytes / sizeof(double) : 0);
    const size_t got = v->empty() ? 0 : fread(v->data(), sizeof(double), v->size(), f);
    fclose(f);
    return got == v->size();
}

static bool write_all(const char *path, const std::vector<double> &v) {
    FILE *f = fopen(path, "wb");
    if (!f) return false;
    const size_t put = v.empty() ? 0 : fwrite(v.data(), sizeof(double), v.size(), f);
    return fclose(f) == 0 && put == v.size();
}

int main(int argc, char **argv) {
    if (argc != 4) {
        fprintf(stderr, "usage: %s solve|rot IN OUT\n", argv[0]);
        return 2;
    }
    std::vector<double> in, out;
    if (!read_all(argv[2], &in)) {
        fprintf(stderr, "cannot read %s\n", argv[2]);
        return 2;
    }
    int worst = 0;
    size_t n = 0;
    if (!strcmp(argv[1], "solve")) {
        if (in.size() % 28) return 2;
        n = in.size() / 28;
        out.resize(n * 4);
        for (size_t i = 0; i < n; ++i) {
            const double *s = &in[i * 28];
            const int sweeps = mpe::dltc::dlt_solve(s, s + 12, s[24], s[25], s[26], s[27], &out[i * 4]);
            out[i * 4 + 3] = (double)sweeps;
            if (sweeps > worst) worst = sweeps;
        }
    } else if (!strcmp(argv[1], "rot")) {
        if (in.size() % 3) return 2;
        n = in.size() / 3;
        out.resize(n * 2);
        double t;
        for (size_t i = 0; i < n; ++i) mpe::dltc::dlt_rotation(in[i * 3], in[i * 3 + 1], in[i * 3 + 2], &out[i * 2], &out[i * 2 + 1], &t);
    } else {
        return 2;
    }
    if (!write_all(argv[3], out)) {
        fprintf(stderr, "cannot write %s\n", argv[3]);
        return 2;
    }
    printf("done %zu most sweeps %d cap %d\n", n, worst, mpe::dltc::DLT_MAX_SWEEPS);
    return 0;
}
