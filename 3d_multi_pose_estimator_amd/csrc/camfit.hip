// mpe_camfit_batch: one pass of the camera fit -- every observation of every camera reduced into the camera's 105 sums (the
// 13 x 13 normal equations of a rigid perturbation, fx, fy, cx, cy and the three radial lens terms, their right-hand side
// and the cost).  normal_sums.h at N = 13: the record is Jx[13], rx, w, Jy[13], ry, rho(e), 30 doubles at a stride of 31; a
// trial camera is E [12], dist [5], (fx, fy, cx, cy) widened.  The file turns contraction off.  DESIGN.md 7.9 has the
// sizing; profiles/camfit_resources.txt the compiler's figures.
#include "normal_sums.h"
#include "project64.h"

#pragma clang fp contract(off)

namespace mpe {

namespace {

struct CamfitSums {
    static constexpr int N = MPE_CAMFIT_UNKNOWNS;
    static constexpr int THREADS = 512;
    static constexpr int RECORDS = 180;       // records per tile: 44,820 bytes of LDS, three workgroups per CU

    // the record of (frame f, row p, joint j, camera c) -> REC_*
    __device__ static uint8_t observe(const NormalK &a, int f, int p, int j, int c, double *rec) {
        const long long fp = (long long)f * a.pcap + p;
        if (!sel_person(a.sel, f, p, fp)) return REC_ABSENT;
        uint32_t present = 0;
        const int head = sel_head(a.sel, f, fp, c, &present);
        if (!sel_joint(a.sel, fp, j, head, present)) return REC_ABSENT;
        double X[3], pc[3];
        load3(a.poses, a.pose_f64, (size_t)fp * a.J + j, X);
        if (!finite3(X[0], X[1], X[2])) return REC_SKIPPED;
        const double *cam = a.cams + CAMFIT_CAM * c, *dist = cam + 12;
        to_camera(cam, X[0], X[1], X[2], pc);
        if (!(pc[2] > 0.0)) return REC_SKIPPED;   // before the quotients: a skipped record computes nothing
        const float K[9] = {(float)cam[17], 0.0f, (float)cam[19], 0.0f, (float)cam[18], (float)cam[20], 0.0f, 0.0f, 1.0f};
        const Proj pr = project_pc(pc, dist, K);
        if (!finite3(pr.px, pr.py, 0.0)) return REC_SKIPPED;
        const double *o = a.xy + ((size_t)head * a.J + j) * 2;
        const double rx = pr.px - o[0], ry = pr.py - o[1];
        const double e = sqrt(rx * rx + ry * ry);
        double *jx = rec, *jy = rec + N + 2;
        rigid_jacobian(pr, K, radial_slope(dist, pr), pc, jx, jy);
        // fx, fy, cx, cy and the lens terms
        jx[6] = pr.h0 * pr.f, jy[6] = 0.0;
        jx[7] = 0.0, jy[7] = pr.h1 * pr.f;
        jx[8] = 1.0, jy[8] = 0.0;
        jx[9] = 0.0, jy[9] = 1.0;
        const double gx = (double)K[0] * pr.h0, gy = (double)K[4] * pr.h1;
        const double r2 = pr.r * pr.r, r3 = r2 * pr.r;
        jx[10] = gx * pr.r, jy[10] = gy * pr.r;
        jx[11] = gx * r2, jy[11] = gy * r2;
        jx[12] = gx * r3, jy[12] = gy * r3;
        jx[N] = rx;
        jx[N + 1] = huber_weight(e, a.huber);
        jy[N] = ry;
        jy[N + 1] = rho(e, a.huber);
        return REC_SUMMED;
    }
};
static_assert(normal_sums(CamfitSums::N) == MPE_CAMFIT_SUMS, "the sums of include/mpe.h");

}  // namespace

// the chains of a thread: 2 up to nine cameras, 5 up to twenty-four, 7 up to the cap
hipError_t launch_camfit(hipStream_t s, const DevCfg *cfg, normal_state *st, const mpe_batch &b, const mpe_calib_args &x) {
    return launch_normal_sums<CamfitSums, 2, 5, 7>(s, cfg, st, b, x);
}

}  // namespace mpe
