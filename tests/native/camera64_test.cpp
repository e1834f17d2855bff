// csrc/project64.h on the host (tests/test_camera64_host.py builds this with -ffp-contract=off under the sanitizers and
// compares every output bit with harness/refine.py).  Reads one file of doubles, writes one:
//
//   in:  nC nP nE nH nS | nC cameras: T[12] dist[5] K[9] (K float values, widened) | nP points X[3] | nE lengths e |
//        nH Huber thresholds | nS systems: X[3] lambda huber nObs nBones, nObs x (camera ox oy), nBones x (m[3] q)
//   out: per (camera, point): px py pc2 jx[3] jy[3] | per (huber, e): rho weight | per system: delta[3] ok
#include <stdio.h>
#include <stdlib.h>

#include <vector>

#include "project64.h"

struct Camera {
    double T[12], dist[5];
    float K[9];
};

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
    const int nC = (int)next(), nP = (int)next(), nE = (int)next(), nH = (int)next(), nS = (int)next();
    std::vector<Camera> cams(nC);
    for (Camera &c : cams) {
        for (double &v : c.T) v = next();
        for (double &v : c.dist) v = next();
        for (float &v : c.K) v = (float)next();
    }
    std::vector<double> pts(3 * (size_t)nP), es(nE), hubers(nH), out;
    for (double &v : pts) v = next();
    for (double &v : es) v = next();
    for (double &v : hubers) v = next();

    for (const Camera &c : cams)
        for (int i = 0; i < nP; ++i) {
            const mpe::Proj p = mpe::project(c.T, c.dist, c.K, pts[3 * i], pts[3 * i + 1], pts[3 * i + 2]);
            double jx[3], jy[3];
            mpe::point_jacobian(c.T, c.dist, c.K, p, jx, jy);
            out.insert(out.end(), {p.px, p.py, p.pc2, jx[0], jx[1], jx[2], jy[0], jy[1], jy[2]});
        }
    for (double h : hubers)
        for (double e : es) out.insert(out.end(), {mpe::rho(e, h), mpe::huber_weight(e, h)});
    for (int s = 0; s < nS; ++s) {
        const double X0 = next(), X1 = next(), X2 = next(), lambda = next(), huber = next();
        const int nObs = (int)next(), nBones = (int)next();
        mpe::Normal3 N;
        for (int o = 0; o < nObs; ++o) {
            const int ci = (int)next();
            const double ox = next(), oy = next();
            if (ci < 0 || ci >= nC) return 3;
            const Camera &c = cams[ci];
            const mpe::Proj p = mpe::project(c.T, c.dist, c.K, X0, X1, X2);
            const double rx = p.px - ox, ry = p.py - oy;
            double jx[3], jy[3];
            mpe::point_jacobian(c.T, c.dist, c.K, p, jx, jy);
            N.add_pixel(mpe::huber_weight(sqrt(rx * rx + ry * ry), huber), jx, jy, rx, ry);
        }
        for (int b = 0; b < nBones; ++b) {
            const double m[3] = {next(), next(), next()};
            N.add_bone(m, next());
        }
        double e[3];
        const bool ok = N.lm_step(lambda, e);
        out.insert(out.end(), {e[0], e[1], e[2], ok ? 1.0 : 0.0});
    }
    if (at != in.size()) return 3;
    // one finite3 and load3 for everyone: their answers on what was just computed
    double X[3];
    const float f3[3] = {1.5f, -2.25f, 3.0f};
    mpe::load3(f3, 0, 0, X);
    if (!(X[0] == 1.5 && X[1] == -2.25 && X[2] == 3.0) || !mpe::finite3(X[0], X[1], X[2]) || mpe::finite3(X[0], X[1] / 0.0, X[2]) ||
        mpe::finite3(X[0], X[1], (X[2] - 3.0) / 0.0))
        return 4;
    mpe::load3(pts.data(), 1, nP > 0 ? (size_t)nP - 1 : 0, X);
    if (nP > 0 && !(X[2] == pts[3 * (size_t)nP - 1] || X[2] != X[2])) return 4;
    static_assert(sizeof(mpe::Bits<float>::type) == 4 && sizeof(mpe::Bits<double>::type) == 8, "as wide as the coordinate");

    fh = fopen(argv[2], "wb");
    if (!fh || fwrite(out.data(), sizeof(double), out.size(), fh) != out.size()) return 2;
    fclose(fh);
    printf("done %d cameras %d points %d systems\n", nC, nP, nS);
    return 0;
}
