// mpe_calib_batch: one pass of the extrinsics calibration -- every observation of every camera reduced into the camera's 28
// sums (the 6 x 6 normal equations of a rigid perturbation, their right-hand side and the cost).  normal_sums.h at N = 6:
// the record is Jx[6], rx, w, Jy[6], ry, rho(e), 16 doubles at a stride of 17; a trial camera is its extrinsics [12], and
// the intrinsics and the lens terms are the context's.  The file turns contraction off.
#include "normal_sums.h"
#include "project64.h"

#pragma clang fp contract(off)

namespace mpe {

namespace {

struct CalibSums {
    static constexpr int N = 6;
    static constexpr int THREADS = 256;
    static constexpr int RECORDS = 384;       // records per tile: 51 KiB + 384 bytes of LDS, three workgroups per CU

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
        to_camera(a.cams + CALIB_CAM * c, X[0], X[1], X[2], pc);
        if (!(pc[2] > 0.0)) return REC_SKIPPED;   // before the quotients: a skipped record computes nothing
        const float *K = a.cfg->K[c];
        const Proj pr = project_pc(pc, a.cfg->dist[c], K);
        if (!finite3(pr.px, pr.py, 0.0)) return REC_SKIPPED;
        const double *o = a.xy + ((size_t)head * a.J + j) * 2;
        const double rx = pr.px - o[0], ry = pr.py - o[1];
        const double e = sqrt(rx * rx + ry * ry);
        rigid_jacobian(pr, K, radial_slope(a.cfg->dist[c], pr), pc, rec, rec + N + 2);
        rec[N] = rx;
        rec[N + 1] = huber_weight(e, a.huber);
        rec[2 * N + 2] = ry;
        rec[2 * N + 3] = rho(e, a.huber);
        return REC_SUMMED;
    }
};
static_assert(normal_sums(CalibSums::N) == MPE_CALIB_SUMS, "the sums of include/mpe.h");

}  // namespace

// the chains of a thread: 1 up to nine cameras, 3 up to twenty-seven, 4 up to the cap
hipError_t launch_calib(hipStream_t s, const DevCfg *cfg, normal_state *st, const mpe_batch &b, const mpe_calib_args &x) {
    return launch_normal_sums<CalibSums, 1, 3, 4>(s, cfg, st, b, x);
}

}  // namespace mpe
