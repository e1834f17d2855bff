// mpe_posecov_batch: the 3 x 3 covariance of every joint of every pose from the cameras that saw it, sigma_px^2 * A^-1 with
// A the normal matrix the refinement builds at that point -- binary64, in the order include/mpe.h gives.
//
// k_posecov: k_refine's shape (refine.hip).  A 32-lane half of a wave is one (frame, person): its lane 0 reads n_persons
// and the person flag once, lane c reads the head camera c has for the person and that head's joint mask once, and the
// camera loops fetch both from lane c (the loop index is uniform across the wave, so the DevCfg rows are uniform loads).
// Lane j owns joint j.  One pass over the cameras: projection, Jacobian and the six sums of A stay in registers, then
// cov3.h inverts.  Every lane reads and writes its own joint's flag only, so d_flags_out may be d_flags.  No LDS, no
// atomics.  The file turns contraction off; f64 quotients and roots are the language's correctly rounded ones.
#include "mpe_internal.h"
#include "project64.h"
#include "reproject_select.h"
#include "cov3.h"

#pragma clang fp contract(off)

namespace mpe {

namespace {

constexpr int PC_GROUPS = 8;                  // (frame, person) pairs per 256-thread workgroup
static_assert(MPE_MAX_CAMERAS <= 32 && MPE_MAX_JOINTS <= 32, "a half wave holds the cameras and the joints of a person");

struct PosecovK {
    int n_frames, pcap, V, J, pose_f64;
    double huber, s2, gate;
    Selection sel;                            // which cameras observe a joint (reproject_select.h)
    const double *xy;
    const void *poses;
    double *cov, *sigma;
    uint8_t *status, *n_views, *flags_out;
};

__global__ void __launch_bounds__(32 * PC_GROUPS) k_posecov(const DevCfg *__restrict__ cfg, PosecovK a) {
    const int j = threadIdx.x & 31;
    const long long n_groups = (long long)a.n_frames * a.pcap;
    for (long long fp = (long long)blockIdx.x * PC_GROUPS + (threadIdx.x >> 5); fp < n_groups; fp += (long long)gridDim.x * PC_GROUPS) {
        const int f = (int)(fp / a.pcap);
        int live = 0;
        if (j == 0) live = sel_person(a.sel, f, (int)(fp - (long long)f * a.pcap), fp);
        live = __shfl(live, 0, 32);
        int my_head = -1;                     // lane c: camera c's head for this person
        uint32_t my_present = 0;
        if (live && j < a.V) my_head = sel_head(a.sel, f, fp, j, &my_present);
        const bool mine = j < a.J;
        const size_t at = (size_t)fp * a.J + (mine ? j : 0);

        uint32_t obs = 0;                     // cameras that observe joint j
        for (int c = 0; c < a.V; ++c) {
            const int head = __shfl(my_head, c, 32);
            const uint32_t present = __shfl(my_present, c, 32);
            if (mine && sel_joint(a.sel, fp, j, head, present)) obs |= 1u << c;
        }
        const int views = __popc(obs);
        uint8_t flag = 0;                     // read before any lane of the row writes d_flags_out
        if (mine && a.flags_out) flag = a.sel.flags[at];

        double X[3] = {0.0, 0.0, 0.0};
        if (mine) load3(a.poses, a.pose_f64, at, X);
        const bool many = mine && views >= 2;
        bool good = finite3(X[0], X[1], X[2]);
        double A[6] = {0.0, 0.0, 0.0, 0.0, 0.0, 0.0};
        for (int c = 0; c < a.V; ++c) {
            const int head = __shfl(my_head, c, 32);
            if (!(many && ((obs >> c) & 1u))) continue;
            const Proj p = project(cfg->P[c], cfg->dist[c], cfg->K[c], X[0], X[1], X[2]);
            if (!(p.pc2 > 0.0)) good = false;
            const double *o = a.xy + ((size_t)head * a.J + j) * 2;
            const double rx = p.px - o[0], ry = p.py - o[1];
            const double w = huber_weight(sqrt(rx * rx + ry * ry), a.huber);
            double jx[3], jy[3];
            point_jacobian(cfg->P[c], cfg->dist[c], cfg->K[c], p, jx, jy);
            A[0] = A[0] + w * (jx[0] * jx[0] + jy[0] * jy[0]);
            A[1] = A[1] + w * (jx[0] * jx[1] + jy[0] * jy[1]);
            A[2] = A[2] + w * (jx[0] * jx[2] + jy[0] * jy[2]);
            A[3] = A[3] + w * (jx[1] * jx[1] + jy[1] * jy[1]);
            A[4] = A[4] + w * (jx[1] * jx[2] + jy[1] * jy[2]);
            A[5] = A[5] + w * (jx[2] * jx[2] + jy[2] * jy[2]);
        }
        if (!mine) continue;

        double S[6], cov[6], sigma;
        const bool pivots = cov3_inverse(A, S);
        const bool finite = cov3_finish(S, a.s2, cov, &sigma);
        unsigned st = 0;
        if (views == 1) st = MPE_POSECOV_FEW_VIEWS;
        else if (many && !good) st = MPE_POSECOV_BAD_POSE;
        else if (many && !(pivots && finite)) st = MPE_POSECOV_SINGULAR;
        else if (many) st = MPE_POSECOV_COMPUTED;
        const bool computed = st == MPE_POSECOV_COMPUTED;
        const bool gated = computed && a.gate > 0.0 && sigma > a.gate;
        if (gated) st |= MPE_POSECOV_GATED;
        double *q = a.cov + at * 6;
        for (int k = 0; k < 6; ++k) q[k] = computed ? cov[k] : 0.0;
        a.sigma[at] = computed ? sigma : -1.0;
        a.status[at] = (uint8_t)st;
        a.n_views[at] = (uint8_t)views;
        if (a.flags_out) a.flags_out[at] = gated ? (uint8_t)0 : flag;
    }
}

}  // namespace

hipError_t launch_posecov(hipStream_t s, const DevCfg *cfg, int V, const mpe_batch &b, const mpe_posecov_args &x) {
    PosecovK a{x.n_frames, x.pcap, V, x.n_joints, x.pose_f64, x.huber_px, x.sigma_px * x.sigma_px, x.gate_m,
               Selection{V, x.n_joints, x.joint_flags, x.joint_mask, x.threshold, b.d_frame_head_off, b.d_joint_mask, b.d_vp, x.d_persons,
                         x.d_n_persons, x.d_flags},
               b.d_xy, x.d_poses, x.d_cov, x.d_sigma, x.d_status, x.d_n_views, x.d_flags_out};
    const long long groups = (long long)x.n_frames * x.pcap;
    const long long blocks = (groups + PC_GROUPS - 1) / PC_GROUPS;
    hipLaunchKernelGGL(k_posecov, dim3((unsigned)(blocks < 65536 ? blocks : 65536)), dim3(32 * PC_GROUPS), 0, s, cfg, a);
    return hipGetLastError();
}

}  // namespace mpe
