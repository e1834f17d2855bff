// mpe_body_refine_batch: the body-level fit (include/mpe.h words the rule; the numpy statement is
// harness/skeleton_refine.py).  One cost per tracked row -- the reprojection error of every joint over the cameras that saw
// it plus the deviation of every bone from the length of its track -- minimised joint by joint in binary64.
//
// k_skel_refine    one lane per (row, joint), 32 lanes per row, two rows per one-wave workgroup: a row never leaves its
//                  wave.  The working poses, the rows' lengths and the head every camera has for the row sit in LDS; lane j
//                  keeps joint j's observing cameras, lambda_j and its status in registers.  A colour step: the lanes
//                  whose joint is free and has the step's colour fold the cameras in increasing c (as k_refine does), then
//                  the joint's bones from the incident list the host built at create time, solve and score the trial --
//                  all of it reading the neighbours from LDS; a barrier; the lanes that accepted write their joint; a
//                  barrier.  Two joints of one colour share no bone, so no lane reads what the step writes.  Every lane
//                  of the workgroup reaches every barrier: rows that are not processed and the lanes past J guard their
//                  work, not their way.  No atomics.  The file turns contraction off; f64 quotients and roots are the
//                  language's correctly rounded ones.
#include "mpe_internal.h"
#include "project64.h"
#include "reproject_select.h"

#include <vector>

#pragma clang fp contract(off)

namespace mpe {

namespace {

constexpr int SRW = 32, SRR = 64 / SRW;      // lanes per row and rows per workgroup
static_assert(MPE_MAX_CAMERAS <= SRW && MPE_MAX_JOINTS <= SRW && MPE_SKEL_MAX_BONES <= SRW, "a row's 32 lanes hold its cameras, joints and bones");

struct SkelRefineK {
    int n_frames, pcap, V, J, n_bones, tid_cap, sweeps, n_colours, batch_frames;
    uint32_t jmask;
    double kappa, huber;
    Selection sel;                            // which cameras observe a joint (reproject_select.h); the rows' flags and n_persons
    const double *xy;
    const void *poses;
    const int32_t *tid, *frame;
    void *poses_out;
    uint8_t *status, *n_views, *n_bones_out;
    double *cost, *err;
    const int32_t *bones;
    const double *len;
    const uint32_t *tab;                      // skel_refine_tables
};

// the camera fold of the local cost at X; *front: pc_2 > 0 in every observing camera
__device__ inline double pixel_cost(const DevCfg *cfg, const SkelRefineK &a, const int *heads, int j, uint32_t obs, double X0, double X1, double X2,
                                    bool *front) {
    double C = 0.0;
    for (int c = 0; c < a.V; ++c) {
        if (!((obs >> c) & 1u)) continue;
        const Proj p = project(cfg->P[c], cfg->dist[c], cfg->K[c], X0, X1, X2);
        if (!(p.pc2 > 0.0)) *front = false;
        const double *o = a.xy + ((size_t)heads[c] * a.J + j) * 2;
        const double rx = p.px - o[0], ry = p.py - o[1];
        C = C + rho(sqrt(rx * rx + ry * ry), a.huber);
    }
    return C;
}

// q = kappa * (l - L) of the bone from N to Y; d and l for the caller
__device__ inline double bone_q(double Y0, double Y1, double Y2, const double *N, double kappa, double L, double *d, double *l) {
    d[0] = Y0 - N[0], d[1] = Y1 - N[1], d[2] = Y2 - N[2];
    const double s = (d[0] * d[0] + d[1] * d[1]) + d[2] * d[2];
    *l = sqrt(s);
    return kappa * (*l - L);
}

template <typename T>
__global__ void __launch_bounds__(64) k_skel_refine(const DevCfg *__restrict__ cfg, SkelRefineK a) {
    __shared__ double s_x[SRR][SRW * 3];      // the working poses
    __shared__ double s_len[SRR][SRW];        // the rows' lengths
    __shared__ double s_fold[SRR][SRW];       // a value per lane for the folds lane 0 of the row takes in order
    __shared__ int s_head[SRR][SRW];          // camera c's head for the row
    __shared__ uint32_t s_present[SRR][SRW];  // and the joints of that head that are asked for
    typedef typename Bits<T>::type B;
    const int g = threadIdx.x / SRW, j = threadIdx.x % SRW, J = a.J, nb = a.n_bones;
    const size_t row = (size_t)blockIdx.x * SRR + g;
    const bool valid = row < (size_t)a.n_frames * a.pcap;     // every lane stays to the end: ballots and barriers
    const size_t fp = valid ? row : 0;
    const int f = (int)(fp / a.pcap), p = (int)(fp - (size_t)f * a.pcap);
    const bool mine = valid && j < J;
    double *x = s_x[g], *Ls = s_len[g], *fold = s_fold[g];
    int *heads = s_head[g];

    // the row: a detection of a track the tables hold, in a frame the batch has
    const int bf = a.frame ? a.frame[f] : f;
    const bool bad_frame = bf < 0 || bf >= a.batch_frames;
    int32_t t = -1;
    if (valid && !bad_frame && p < min(max(a.sel.n_persons[f], 0), a.pcap)) {
        t = a.tid[fp];
        if (!a.sel.joint_flags && !a.sel.flags[fp]) t = -1;
    }
    const bool known = t >= 0 && t < a.tid_cap;

    const T *in = static_cast<const T *>(a.poses) + fp * J * 3;
    B in_bits[3] = {0, 0, 0};
    double X0 = 0.0, X1 = 0.0, X2 = 0.0;
    bool active = false;
    if (mine) {
        const B *q = reinterpret_cast<const B *>(in) + 3 * j;
        in_bits[0] = q[0], in_bits[1] = q[1], in_bits[2] = q[2];
        X0 = (double)in[3 * j], X1 = (double)in[3 * j + 1], X2 = (double)in[3 * j + 2];
        active = known && ((a.jmask >> j) & 1u) && (!a.sel.joint_flags || a.sel.flags[fp * J + j] != 0) && finite3(X0, X1, X2);
    }
    x[3 * j] = X0, x[3 * j + 1] = X1, x[3 * j + 2] = X2;
    const uint32_t act = (uint32_t)(__ballot(active) >> (SRW * g));

    // lane b: bone b of the row; lane c: camera c's head
    bool con_b = false;
    double L = 0.0;
    int bp = 0, bc = 0;
    if (known && j < nb) {
        bp = a.bones[2 * j], bc = a.bones[2 * j + 1];
        L = a.len[(size_t)t * nb + j];
        con_b = ((act >> bp) & (act >> bc) & 1u) && L > 0.0 && L < __builtin_inf();
    }
    Ls[j] = L;
    const uint32_t con = (uint32_t)(__ballot(con_b) >> (SRW * g));
    const bool processed = con != 0;           // known, by con_b
    uint32_t present = 0;
    int head = -1;
    if (processed && j < a.V) head = sel_head(a.sel, bf, (long long)fp, j, &present);
    heads[j] = head;
    s_present[g][j] = present;
    __syncthreads();

    // lane j again: the cameras that observe the joint, its bones, whether it is free
    const uint32_t inc0 = a.tab[SRW + j], inc1 = a.tab[SRW + j + 1];
    const int colour = (int)a.tab[j];
    uint32_t obs = 0;
    bool end = false;
    if (processed && active) {
        for (int c = 0; c < a.V; ++c)
            if (sel_joint(a.sel, (long long)fp, j, heads[c], s_present[g][c])) obs |= 1u << c;
        for (uint32_t i = inc0; i < inc1; ++i)
            if ((con >> (a.tab[2 * SRW + 1 + i] >> 8)) & 1u) end = true;
    }
    const int views = __popc(obs);
    bool front = true;
    double Cj = pixel_cost(cfg, a, heads, j, obs, X0, X1, X2, &front);
    const bool bad_start = processed && active && !front;
    const bool free_j = processed && active && front && (views >= 1 || end);
    unsigned st = 0;
    if (free_j) st |= MPE_BODY_REFINE_FREE;
    if (bad_start) st |= MPE_BODY_REFINE_BAD_START;
    if (processed && active && views == 1) st |= MPE_BODY_REFINE_ONE_VIEW;
    if (valid && bad_frame) st = MPE_BODY_REFINE_BAD_FRAME;

    // the row's cost at the working poses: lane 0 of the row folds in order -> pixel part, bone part, worst |l - L|
    const bool with_bones = a.kappa > 0.0;
    auto row_cost = [&](double Cj, double *out) {
        fold[j] = Cj;
        __syncthreads();
        if (processed && j == 0) {
            double s = 0.0;
            for (int i = 0; i < J; ++i)
                if ((act >> i) & 1u) s = s + fold[i];
            out[0] = s;
        }
        __syncthreads();
        double qq = 0.0, v = 0.0;
        if (con_b) {
            double d[3], l;
            const double q = bone_q(x[3 * bc], x[3 * bc + 1], x[3 * bc + 2], x + 3 * bp, a.kappa, L, d, &l);
            qq = q * q;
            v = fabs(l - L);
        }
        fold[j] = qq;
        __syncthreads();
        if (processed && j == 0) {
            double s = 0.0;
            if (with_bones)
                for (int i = 0; i < nb; ++i)
                    if ((con >> i) & 1u) s = s + fold[i];
            out[1] = s;
        }
        __syncthreads();
        fold[j] = v;
        __syncthreads();
        if (processed && j == 0) {
            double m = 0.0;
            for (int i = 0; i < nb; ++i)
                if (((con >> i) & 1u) && fold[i] > m) m = fold[i];
            out[2] = m;
        }
        __syncthreads();
    };
    double at_start[3] = {-1.0, -1.0, -1.0}, at_end[3] = {-1.0, -1.0, -1.0};
    row_cost(Cj, at_start);

    // the sweeps
    double lambda = 1e-3;
    for (int sweep = 0; sweep < a.sweeps; ++sweep)
        for (int col = 0; col < a.n_colours; ++col) {
            bool accept = false;
            double Y0 = X0, Y1 = X1, Y2 = X2;
            if (free_j && colour == col) {
                Normal3 N;
                double C = 0.0;
                for (int c = 0; c < a.V; ++c) {
                    if (!((obs >> c) & 1u)) continue;
                    const Proj pr = project(cfg->P[c], cfg->dist[c], cfg->K[c], X0, X1, X2);
                    const double *o = a.xy + ((size_t)heads[c] * J + j) * 2;
                    const double rx = pr.px - o[0], ry = pr.py - o[1];
                    const double e = sqrt(rx * rx + ry * ry);
                    C = C + rho(e, a.huber);
                    double jx[3], jy[3];
                    point_jacobian(cfg->P[c], cfg->dist[c], cfg->K[c], pr, jx, jy);
                    N.add_pixel(huber_weight(e, a.huber), jx, jy, rx, ry);
                }
                if (with_bones)
                    for (uint32_t i = inc0; i < inc1; ++i) {
                        const uint32_t code = a.tab[2 * SRW + 1 + i];          // bone << 8 | other end
                        const int b = (int)(code >> 8);
                        if (!((con >> b) & 1u)) continue;
                        double d[3], l;
                        const double q = bone_q(X0, X1, X2, x + 3 * (code & 255u), a.kappa, Ls[b], d, &l);
                        C = C + q * q;
                        if (!(l > 0.0)) continue;
                        const double m[3] = {a.kappa * (d[0] / l), a.kappa * (d[1] / l), a.kappa * (d[2] / l)};
                        N.add_bone(m, q);
                    }
                double e[3];
                bool ok = N.lm_step(lambda, e);
                if (ok) {
                    Y0 = X0 + e[0], Y1 = X1 + e[1], Y2 = X2 + e[2];
                    double Ct = pixel_cost(cfg, a, heads, j, obs, Y0, Y1, Y2, &ok);
                    if (with_bones)
                        for (uint32_t i = inc0; i < inc1; ++i) {
                            const uint32_t code = a.tab[2 * SRW + 1 + i];
                            const int b = (int)(code >> 8);
                            if (!((con >> b) & 1u)) continue;
                            double d[3], l;
                            const double q = bone_q(Y0, Y1, Y2, x + 3 * (code & 255u), a.kappa, Ls[b], d, &l);
                            Ct = Ct + q * q;
                        }
                    accept = ok && Ct < C;
                }
                lambda = accept ? fmax(lambda / 10.0, 1e-12) : lambda * 10.0;
            }
            __syncthreads();               // every read of the step is done
            if (accept) {
                X0 = Y0, X1 = Y1, X2 = Y2;
                x[3 * j] = X0, x[3 * j + 1] = X1, x[3 * j + 2] = X2;
                st |= MPE_BODY_REFINE_MOVED;
            }
            __syncthreads();
        }
    front = true;
    row_cost(pixel_cost(cfg, a, heads, j, obs, X0, X1, X2, &front), at_end);

    if (mine) {
        B *out = static_cast<B *>(a.poses_out) + (fp * J + j) * 3;
        const double X[3] = {X0, X1, X2};
        for (int c = 0; c < 3; ++c) {
            B bits = in_bits[c];
            if (st & MPE_BODY_REFINE_MOVED) {
                const T r = (T)X[c];
                __builtin_memcpy(&bits, &r, sizeof(T));
            }
            out[c] = bits;
        }
        a.status[fp * J + j] = (uint8_t)st;
        a.n_views[fp * J + j] = (uint8_t)views;
    }
    if (valid && j == 0) {
        a.cost[4 * fp] = at_start[0], a.cost[4 * fp + 1] = at_start[1], a.cost[4 * fp + 2] = at_end[0], a.cost[4 * fp + 3] = at_end[1];
        a.err[2 * fp] = at_start[2], a.err[2 * fp + 1] = at_end[2];
        a.n_bones_out[fp] = (uint8_t)__popc(con);
    }
}

}  // namespace

// What the kernel reads of the bone list, built once: [0, 32) the colour of every joint (over j increasing, the least
// colour no lower-numbered joint that shares a bone with j holds), [32, 65) where the incident bones of joint j begin,
// then the incident bones in list order as bone << 8 | other end.  -> the number of colours
int skel_refine_tables(const int32_t *bones, int n_bones, int J, std::vector<uint32_t> *tab) {
    tab->assign(2 * SRW + 1 + 2 * MPE_SKEL_MAX_BONES, 0u);
    uint32_t *colour = tab->data(), *begin = tab->data() + SRW, *inc = tab->data() + 2 * SRW + 1;
    int n_colours = 1, at = 0;
    for (int j = 0; j < SRW; ++j) {
        begin[j] = (uint32_t)at;
        uint32_t taken = 0;
        for (int b = 0; b < n_bones && j < J; ++b) {
            const int jp = bones[2 * b], jc = bones[2 * b + 1];
            if (jp != j && jc != j) continue;
            const int other = jp == j ? jc : jp;
            inc[at++] = (uint32_t)b << 8 | (uint32_t)other;
            if (other < j) taken |= 1u << colour[other];
        }
        int k = 0;
        while ((taken >> k) & 1u) ++k;
        colour[j] = (uint32_t)k;
        if (k + 1 > n_colours) n_colours = k + 1;
    }
    begin[SRW] = (uint32_t)at;
    return n_colours;
}

hipError_t launch_skel_refine(hipStream_t s, const DevCfg *cfg, int V, mpe_skel_state *st, const mpe_batch &b, const mpe_body_refine_args &x) {
    const int J = st->J;
    SkelRefineK a{};
    a.n_frames = x.n_frames; a.pcap = st->pcap; a.V = V; a.J = J; a.n_bones = st->n_bones;
    a.tid_cap = st->tid_cap; a.sweeps = x.sweeps; a.n_colours = st->n_colours; a.batch_frames = b.n_frames;
    a.jmask = x.joint_mask & (J >= 32 ? 0xFFFFFFFFu : (1u << J) - 1u);
    a.kappa = x.bone_weight; a.huber = x.huber_px;
    a.sel = Selection{V, J, x.joint_flags, x.joint_mask, x.threshold, b.d_frame_head_off, b.d_joint_mask, b.d_vp, x.d_persons, x.d_n_persons, x.d_flags};
    a.xy = b.d_xy;
    a.poses = x.d_poses; a.tid = x.d_track_id; a.frame = x.d_frame;
    a.poses_out = x.d_poses_out; a.status = x.d_status; a.n_views = x.d_n_views; a.n_bones_out = x.d_n_bones;
    a.cost = x.d_cost; a.err = x.d_err;
    a.bones = st->bones; a.len = st->len; a.tab = st->refine_tab;
    const size_t rows = (size_t)x.n_frames * st->pcap;       // <= 2^23 * 128
    const dim3 grid((unsigned)((rows + SRR - 1) / SRR));
    if (st->pose_f64) hipLaunchKernelGGL(k_skel_refine<double>, grid, dim3(64), 0, s, cfg, a);
    else hipLaunchKernelGGL(k_skel_refine<float>, grid, dim3(64), 0, s, cfg, a);
    const hipError_t e = hipGetLastError();
    if (e == hipSuccess) ++st->launches;
    return e;
}

}  // namespace mpe
