// mpe_refine_timed_batch: mpe_refine_batch with every camera looking at the joint where the joint's track says it was at
// that camera's time -- one 3-unknown Levenberg-Marquardt problem per (frame, person, joint), binary64, in the order
// include/mpe.h gives.
//
// k_refine_timed keeps k_refine's shape (refine.hip): a 32-lane half of a wave is one (frame, person), lane j owns joint j,
// lane c holds camera c's head, the camera loops are uniform.  New is a prologue.  Lane c takes camera c's (s, alpha) --
// the host derives them from lag[] -- and scans at most pcap ids of table frames F+s and F+s+1 for the rows of the
// person's track; lane 0 does the same for frame F.  The joint lanes get the rows by shuffle, read their joint of the two
// or three rows from the table, test flags and finiteness, and write the camera's offset d_c into their own column of LDS,
// laid out [group][c][k][joint]: V * 3 doubles per lane are 138 registers at 23 cameras, and k_refine already sits at the
// 128-register edge.  A lane reads back only what it wrote, so there is no barrier anywhere.  Which cameras have an offset
// is a 32-bit mask in a register; a camera without one projects X itself, with no addition, so that with every lag zero
// the bits are k_refine's.  The LDS is dynamic, V * 3 * J doubles per group, and the groups per workgroup follow from it
// (8 while they fit 48 KiB, else 4, 2 or 1).  One workgroup per RT_GROUPS-or-fewer (frame, person) pairs, no stride
// loop.  The file turns contraction off; f64 quotients and roots are the language's correctly rounded ones.
#include "mpe_internal.h"
#include "pose_rows.h"
#include "project64.h"
#include "reproject_select.h"

#pragma clang fp contract(off)

namespace mpe {

namespace {

constexpr int RT_GROUPS = 8;                  // (frame, person) pairs per workgroup, at most
constexpr size_t RT_LDS = 48 * 1024;          // the offsets of a workgroup stay within this
static_assert(MPE_MAX_CAMERAS <= 32 && MPE_MAX_JOINTS <= 32, "a half wave holds the cameras and the joints of a person");
static_assert((size_t)MPE_MAX_CAMERAS * 3 * MPE_MAX_JOINTS * sizeof(double) <= RT_LDS, "one group's offsets fit");

struct RefineTimedK {
    int n_frames, frame_start, V, max_iters;
    double step_tol, huber;
    PoseRows rows;                            // the table: rows.n_frames = n_table
    Selection sel;                            // n_persons and flags point at frame_start of the table's
    const double *xy;
    void *poses_out;
    uint8_t *status;
    double *cost0, *cost1;
    uint8_t *iters, *n_views, *n_timed;
    int s[MPE_MAX_CAMERAS];                   // floor(lag[c])
    double alpha[MPE_MAX_CAMERAS];            // lag[c] - s[c]
    uint32_t lagged;                          // bit c: lag[c] != 0
};

// the row of (g, t) as mpe_lag_batch has it, -1 without one
__device__ inline int timed_row(const PoseRows &r, int g, int t) {
    if (g < 0 || g >= r.n_frames) return -1;
    const int n = rows_in_frame(r, g);
    for (int p = 0; p < n; ++p) {
        const size_t fp = (size_t)g * r.pcap + p;
        if (r.tid[fp] == t && (r.joint_flags || r.flags[fp] != 0)) return p;
    }
    return -1;
}

// joint j of row `row` (>= 0) of table frame g when it is flagged and finite
__device__ inline bool timed_joint(const PoseRows &r, int g, int row, int j, double *X) {
    const size_t fp = (size_t)g * r.pcap + row;
    load3(r.poses, r.pose_f64, fp * r.J + j, X);
    return joint_flag(r, fp, j) && finite3(X[0], X[1], X[2]);
}

__global__ void __launch_bounds__(32 * RT_GROUPS) k_refine_timed(const DevCfg *__restrict__ cfg, RefineTimedK a) {
    extern __shared__ double s_off[];         // [groups of the workgroup][V][3][J]
    const int j = threadIdx.x & 31, grp = threadIdx.x >> 5;
    const int pcap = a.rows.pcap, J = a.rows.J;
    const long long fp = (long long)blockIdx.x * (blockDim.x >> 5) + grp;
    if (fp >= (long long)a.n_frames * pcap) return;          // no barrier below
    const int f = (int)(fp / pcap), p = (int)(fp - (long long)f * pcap);
    const int F = a.frame_start + f;
    double *off = s_off + (size_t)grp * a.V * 3 * J + j;     // this lane's column: off[(c * 3 + k) * J]

    int live = 0;
    if (j == 0) live = sel_person(a.sel, f, p, fp);
    live = __shfl(live, 0, 32);
    int my_head = -1;                         // lane c: camera c's head for this person
    uint32_t my_present = 0;
    if (live && j < a.V) my_head = sel_head(a.sel, f, fp, j, &my_present);
    const bool mine = j < J;
    const size_t at_in = ((size_t)F * pcap + p) * J + (mine ? j : 0);
    const size_t at = (size_t)fp * J + (mine ? j : 0);

    // the prologue: the rows of the person's track, lane c those of camera c's frames, lane 0 the frame's own
    const int t = live ? a.rows.tid[(size_t)F * pcap + p] : -1;
    int my_ra = -1, my_rb = -1, row_f = -1;
    if (t >= 0 && j < a.V && ((a.lagged >> j) & 1u)) {
        my_ra = timed_row(a.rows, F + a.s[j], t);
        if (my_ra >= 0 && a.alpha[j] != 0.0) my_rb = timed_row(a.rows, F + a.s[j] + 1, t);
    }
    if (t >= 0 && j == 0 && a.lagged) row_f = timed_row(a.rows, F, t);
    row_f = __shfl(row_f, 0, 32);

    uint32_t obs = 0;                         // cameras that observe joint j
    for (int c = 0; c < a.V; ++c) {
        const int head = __shfl(my_head, c, 32);
        const uint32_t present = __shfl(my_present, c, 32);
        if (mine && sel_joint(a.sel, fp, j, head, present)) obs |= 1u << c;
    }
    const int views = __popc(obs);

    uint32_t timed = 0;                       // observing cameras with an offset in this lane's column
    double Xf[3] = {0.0, 0.0, 0.0};
    const bool have_f = mine && obs && row_f >= 0 && timed_joint(a.rows, F, row_f, j, Xf);
    for (int c = 0; c < a.V; ++c) {
        const int ra = __shfl(my_ra, c, 32), rb = __shfl(my_rb, c, 32);
        const double alpha = a.alpha[c];
        if (!(have_f && ((obs >> c) & 1u) && ra >= 0 && (alpha == 0.0 || rb >= 0))) continue;
        double Xl[3];
        if (!timed_joint(a.rows, F + a.s[c], ra, j, Xl)) continue;
        if (alpha != 0.0) {
            double Xb[3];
            if (!timed_joint(a.rows, F + a.s[c] + 1, rb, j, Xb)) continue;
            for (int k = 0; k < 3; ++k) Xl[k] = Xl[k] + alpha * (Xb[k] - Xl[k]);
        }
        for (int k = 0; k < 3; ++k) off[(size_t)(c * 3 + k) * J] = Xl[k] - Xf[k];
        timed |= 1u << c;
    }

    double X0 = 0.0, X1 = 0.0, X2 = 0.0;
    float in32[3] = {0.0f, 0.0f, 0.0f};
    if (mine) {
        if (a.rows.pose_f64) {
            const double *q = static_cast<const double *>(a.rows.poses) + at_in * 3;
            X0 = q[0], X1 = q[1], X2 = q[2];
        } else {
            const float *q = static_cast<const float *>(a.rows.poses) + at_in * 3;
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
        double Z0 = X0, Z1 = X1, Z2 = X2;
        if ((timed >> c) & 1u) Z0 = X0 + off[(size_t)(c * 3) * J], Z1 = X1 + off[(size_t)(c * 3 + 1) * J], Z2 = X2 + off[(size_t)(c * 3 + 2) * J];
        const Proj pr = project(cfg->P[c], cfg->dist[c], cfg->K[c], Z0, Z1, Z2);
        if (!(pr.pc2 > 0.0)) start_ok = false;
        const double *o = a.xy + ((size_t)head * J + j) * 2;
        const double rx = pr.px - o[0], ry = pr.py - o[1];
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
        // Normal3's lines (project64.h) written out, as in k_refine
        double A00 = 0.0, A01 = 0.0, A02 = 0.0, A11 = 0.0, A12 = 0.0, A22 = 0.0, g0 = 0.0, g1 = 0.0, g2 = 0.0;
        for (int c = 0; c < a.V; ++c) {
            const int head = __shfl(my_head, c, 32);
            if (!(active && ((obs >> c) & 1u))) continue;
            double Z0 = X0, Z1 = X1, Z2 = X2;
            if ((timed >> c) & 1u) Z0 = X0 + off[(size_t)(c * 3) * J], Z1 = X1 + off[(size_t)(c * 3 + 1) * J], Z2 = X2 + off[(size_t)(c * 3 + 2) * J];
            const Proj pr = project(cfg->P[c], cfg->dist[c], cfg->K[c], Z0, Z1, Z2);
            const double *o = a.xy + ((size_t)head * J + j) * 2;
            const double rx = pr.px - o[0], ry = pr.py - o[1];
            const double e = sqrt(rx * rx + ry * ry);
            const double w = huber_weight(e, a.huber);
            double jx[3], jy[3];
            point_jacobian(cfg->P[c], cfg->dist[c], cfg->K[c], pr, jx, jy);
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
        const double tt = A12 - L20 * A01;
        const double L21 = tt / D1;
        const double D2 = (M22 - L20 * A02) - L21 * tt;
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
            double Z0 = Y0, Z1 = Y1, Z2 = Y2;
            if ((timed >> c) & 1u) Z0 = Y0 + off[(size_t)(c * 3) * J], Z1 = Y1 + off[(size_t)(c * 3 + 1) * J], Z2 = Y2 + off[(size_t)(c * 3 + 2) * J];
            const Proj pr = project(cfg->P[c], cfg->dist[c], cfg->K[c], Z0, Z1, Z2);
            if (!(pr.pc2 > 0.0)) ok = false;
            const double *o = a.xy + ((size_t)head * J + j) * 2;
            const double rx = pr.px - o[0], ry = pr.py - o[1];
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

    if (!mine) return;
    const bool moved = (st & MPE_REFINE_MOVED) != 0;
    if (a.rows.pose_f64) {
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
    a.n_timed[at] = (uint8_t)__popc(timed);
}

// (frame, person) pairs per workgroup: as many of 8, 4, 2, 1 as keep the offsets within RT_LDS
int refine_timed_groups(int V, int J) {
    int g = RT_GROUPS;
    while (g > 1 && (size_t)g * V * 3 * J * sizeof(double) > RT_LDS) g >>= 1;
    return g;
}

}  // namespace

hipError_t launch_refine_timed(hipStream_t s, const DevCfg *cfg, int V, const mpe_batch &b, const mpe_refine_timed_args &x) {
    const size_t row0 = (size_t)x.frame_start * x.pcap;
    RefineTimedK a{x.n_frames, x.frame_start, V, x.max_iters, x.step_tol, x.huber_px,
                   PoseRows{x.n_table, x.pcap, x.n_joints, x.pose_f64, x.joint_flags, x.d_poses, x.d_flags, x.d_n_persons, x.d_tid},
                   Selection{V, x.n_joints, x.joint_flags, x.joint_mask, x.threshold, b.d_frame_head_off, b.d_joint_mask, b.d_vp, x.d_persons,
                             x.d_n_persons + x.frame_start, x.d_flags + row0 * (x.joint_flags ? x.n_joints : 1)},
                   b.d_xy, x.d_poses_out, x.d_status, x.d_cost0, x.d_cost1, x.d_iters, x.d_n_views, x.d_n_timed, {}, {}, 0u};
    for (int c = 0; c < V; ++c) {
        const double fl = floor(x.lag[c]);
        a.s[c] = (int)fl;
        a.alpha[c] = x.lag[c] - fl;
        if (x.lag[c] != 0.0) a.lagged |= 1u << c;
    }
    const int groups = refine_timed_groups(V, x.n_joints);
    const long long pairs = (long long)x.n_frames * x.pcap;
    const long long blocks = (pairs + groups - 1) / groups;
    if (blocks > 0x7FFFFFFFLL) return hipErrorInvalidConfiguration;
    hipLaunchKernelGGL(k_refine_timed, dim3((unsigned)blocks), dim3(32 * groups), (size_t)groups * V * 3 * x.n_joints * sizeof(double), s, cfg, a);
    return hipGetLastError();
}

}  // namespace mpe
