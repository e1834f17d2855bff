// mpe_refine_batch: every joint moved to the minimum of its reprojection cost over the cameras that saw it -- one
// 3-unknown Levenberg-Marquardt problem per (frame, person, joint), binary64, in the order include/mpe.h gives.
//
// k_refine: one lane per (frame, person, joint).  A 32-lane half of a wave is one (frame, person), as in k_reproject: its
// lane 0 reads n_persons and the person flag once, lane c reads the head camera c has for the person and that head's
// joint mask once, and the camera loops fetch both from lane c (the loop index is uniform across the wave, so the DevCfg
// rows are uniform loads).  Lane j owns joint j: the observing cameras as a 32-bit mask, the point, lambda and the cost
// stay in registers; pose loads and stores are consecutive across the lanes.  The iteration loop is uniform: a lane
// that has stopped idles until no lane of its wave is active (no rebalancing).  No LDS, no atomics.  The file turns
// contraction off; f64 quotients and roots are the language's correctly rounded ones.
#include "mpe_internal.h"
#include "project64.h"
#include "reproject_select.h"

#pragma clang fp contract(off)

namespace mpe {

namespace {

constexpr int RF_GROUPS = 8;                  // (frame, person) pairs per 256-thread workgroup
static_assert(MPE_MAX_CAMERAS <= 32 && MPE_MAX_JOINTS <= 32, "a half wave holds the cameras and the joints of a person");

struct RefineK {
    int n_frames, pcap, V, J, pose_f64, max_iters;
    double step_tol, huber;
    Selection sel;                            // which cameras observe a joint (reproject_select.h)
    const double *xy;
    const void *poses;
    void *poses_out;
    uint8_t *status;
    double *cost0, *cost1;
    uint8_t *iters, *n_views;
};

__global__ void __launch_bounds__(32 * RF_GROUPS) k_refine(const DevCfg *__restrict__ cfg, RefineK a) {
    const int j = threadIdx.x & 31;
    const long long n_groups = (long long)a.n_frames * a.pcap;
    for (long long fp = (long long)blockIdx.x * RF_GROUPS + (threadIdx.x >> 5); fp < n_groups; fp += (long long)gridDim.x * RF_GROUPS) {
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

        double X0 = 0.0, X1 = 0.0, X2 = 0.0;
        float in32[3] = {0.0f, 0.0f, 0.0f};
        if (mine) {
            if (a.pose_f64) {
                const double *q = static_cast<const double *>(a.poses) + at * 3;
                X0 = q[0], X1 = q[1], X2 = q[2];
            } else {
                const float *q = static_cast<const float *>(a.poses) + at * 3;
                in32[0] = q[0], in32[1] = q[1], in32[2] = q[2];
                X0 = (double)in32[0], X1 = (double)in32[1], X2 = (double)in32[2];
            }
        }
        const double in0 = X0, in1 = X1, in2 = X2;

        // the cost at the start; a start behind an observing camera is not solved
        unsigned st = 0;
        bool active = mine && views >= 2;
        if (mine && views == 1) st = MPE_REFINE_FEW_VIEWS;
        bool start_ok = finite3(X0, X1, X2);
        double C = 0.0;
        for (int c = 0; c < a.V; ++c) {
            const int head = __shfl(my_head, c, 32);
            if (!(active && ((obs >> c) & 1u))) continue;
            const Proj p = project(cfg->P[c], cfg->dist[c], cfg->K[c], X0, X1, X2);
            if (!(p.pc2 > 0.0)) start_ok = false;
            const double *o = a.xy + ((size_t)head * a.J + j) * 2;
            const double rx = p.px - o[0], ry = p.py - o[1];
            C = C + rho(sqrt(rx * rx + ry * ry), a.huber);
        }
        if (active && !start_ok) {
            active = false;
            st = MPE_REFINE_BAD_START;
        }
        const bool solved = active;
        const double C0 = C;
        if (solved) st = MPE_REFINE_SOLVED;
        double lambda = 1e-3;
        int iters = 0;

        for (int it = 0; it < a.max_iters; ++it) {
            if (__ballot(active) == 0) break;
            // Normal3's lines (project64.h) written out: with Normal3 and point_jacobian both, this kernel drops under 128
            // registers, runs a fourth wave and is 1.1 % slower at 5x10 with 16 iterations
            double A00 = 0.0, A01 = 0.0, A02 = 0.0, A11 = 0.0, A12 = 0.0, A22 = 0.0, g0 = 0.0, g1 = 0.0, g2 = 0.0;
            for (int c = 0; c < a.V; ++c) {
                const int head = __shfl(my_head, c, 32);
                if (!(active && ((obs >> c) & 1u))) continue;
                const Proj p = project(cfg->P[c], cfg->dist[c], cfg->K[c], X0, X1, X2);
                const double *o = a.xy + ((size_t)head * a.J + j) * 2;
                const double rx = p.px - o[0], ry = p.py - o[1];
                const double e = sqrt(rx * rx + ry * ry);
                const double w = huber_weight(e, a.huber);
                double jx[3], jy[3];
                point_jacobian(cfg->P[c], cfg->dist[c], cfg->K[c], p, jx, jy);
                A00 = A00 + w * (jx[0] * jx[0] + jy[0] * jy[0]);
                A01 = A01 + w * (jx[0] * jx[1] + jy[0] * jy[1]);
                A02 = A02 + w * (jx[0] * jx[2] + jy[0] * jy[2]);
                A11 = A11 + w * (jx[1] * jx[1] + jy[1] * jy[1]);
                A12 = A12 + w * (jx[1] * jx[2] + jy[1] * jy[2]);
                A22 = A22 + w * (jx[2] * jx[2] + jy[2] * jy[2]);
                g0 = g0 + w * (jx[0] * rx + jy[0] * ry);
                g1 = g1 + w * (jx[1] * rx + jy[1] * ry);
                g2 = g2 + w * (jx[2] * rx + jy[2] * ry);
            }
            // (A + lambda diag A) delta = -g, LDL^T written out
            const double M00 = A00 + lambda * A00, M11 = A11 + lambda * A11, M22 = A22 + lambda * A22;
            const double D0 = M00;
            const double L10 = A01 / D0, L20 = A02 / D0;
            const double D1 = M11 - L10 * A01;
            const double t = A12 - L20 * A01;
            const double L21 = t / D1;
            const double D2 = (M22 - L20 * A02) - L21 * t;
            const double z0 = -g0;
            const double z1 = -g1 - L10 * z0;
            const double z2 = (-g2 - L20 * z0) - L21 * z1;
            const double e2 = z2 / D2;
            const double e1 = z1 / D1 - L21 * e2;
            const double e0 = (z0 / D0 - L10 * e1) - L20 * e2;
            bool ok = active && D0 > 0.0 && D1 > 0.0 && D2 > 0.0 && finite3(e0, e1, e2);
            const double Y0 = X0 + e0, Y1 = X1 + e1, Y2 = X2 + e2;
            double Ct = 0.0;
            for (int c = 0; c < a.V; ++c) {
                const int head = __shfl(my_head, c, 32);
                if (!(ok && ((obs >> c) & 1u))) continue;
                const Proj p = project(cfg->P[c], cfg->dist[c], cfg->K[c], Y0, Y1, Y2);
                if (!(p.pc2 > 0.0)) ok = false;
                const double *o = a.xy + ((size_t)head * a.J + j) * 2;
                const double rx = p.px - o[0], ry = p.py - o[1];
                Ct = Ct + rho(sqrt(rx * rx + ry * ry), a.huber);
            }
            if (active) {
                ++iters;
                if (ok && Ct < C) {
                    X0 = Y0, X1 = Y1, X2 = Y2;
                    C = Ct;
                    st |= MPE_REFINE_MOVED;
                    lambda = fmax(lambda / 10.0, 1e-12);
                    if (fmax(fmax(fabs(e0), fabs(e1)), fabs(e2)) < a.step_tol) {
                        st |= MPE_REFINE_CONVERGED;
                        active = false;
                    }
                } else {
                    lambda = lambda * 10.0;
                }
            }
        }

        if (!mine) continue;
        const bool moved = (st & MPE_REFINE_MOVED) != 0;
        if (a.pose_f64) {
            double *q = static_cast<double *>(a.poses_out) + at * 3;
            q[0] = moved ? X0 : in0, q[1] = moved ? X1 : in1, q[2] = moved ? X2 : in2;
        } else {
            float *q = static_cast<float *>(a.poses_out) + at * 3;
            q[0] = moved ? (float)X0 : in32[0], q[1] = moved ? (float)X1 : in32[1], q[2] = moved ? (float)X2 : in32[2];
        }
        a.status[at] = (uint8_t)st;
        a.cost0[at] = solved ? C0 : -1.0;
        a.cost1[at] = solved ? C : -1.0;
        a.iters[at] = (uint8_t)iters;
        a.n_views[at] = (uint8_t)views;
    }
}

}  // namespace

hipError_t launch_refine(hipStream_t s, const DevCfg *cfg, int V, const mpe_batch &b, const mpe_refine_args &x) {
    RefineK a{x.n_frames, x.pcap, V, x.n_joints, x.pose_f64, x.max_iters, x.step_tol, x.huber_px,
              Selection{V, x.n_joints, x.joint_flags, x.joint_mask, x.threshold, b.d_frame_head_off, b.d_joint_mask, b.d_vp, x.d_persons,
                        x.d_n_persons, x.d_flags},
              b.d_xy, x.d_poses, x.d_poses_out, x.d_status, x.d_cost0, x.d_cost1, x.d_iters, x.d_n_views};
    const long long groups = (long long)x.n_frames * x.pcap;
    const long long blocks = (groups + RF_GROUPS - 1) / RF_GROUPS;
    hipLaunchKernelGGL(k_refine, dim3((unsigned)(blocks < 65536 ? blocks : 65536)), dim3(32 * RF_GROUPS), 0, s, cfg, a);
    return hipGetLastError();
}

}  // namespace mpe
