// mpe_lag_batch: one pass of the time-lag estimate -- every supported observation of every camera compared with the
// projection of its track's pose at the K grid lags, the Huber cost of each lag summed per camera, binary64, in the order
// include/mpe.h gives, so that the sums are the same bits however a recording is cut into batches.
//
// k_lag_frame: one workgroup per frame of the call.  First the row map: a thread per (row p, window frame w) looks up the
// row of p's track in table frame f - W + w (a search over at most pcap ids) and the joints of it that are flagged and
// finite; both go to LDS (2 bytes and 4 bytes per entry, 13 KiB at the caps), and a thread per row ANDs the joint words
// over the window into the row's support.  Then the folds: a thread per (camera c, grid entry i) walks (p, j) in order,
// selects by reproject_select.h, reads X_a (and X_b when the entry lies between frames) from the table in global memory,
// interpolates, projects through project64.h and adds rho(e).  Lanes of a wave share c except where a wave crosses a
// camera and differ in the grid entry, so they read the same selection words and the same one or two neighbouring poses:
// one cache line serves the wave, which is why the window is not staged in LDS ((2W+1) * pcap * J * 3 doubles would not fit
// beyond about ten rows anyway, and there is no tile border to cross).  V * K can exceed the workgroup (23 * 65 = 1495): a
// thread then takes (c, i) = id, id + 256, ... one after the other, each fold complete before the next begins.  The
// partials go to a workspace sized at create; the counts are added to the state with integer atomics (the only atomics:
// no f64 atomic anywhere); the thread of entry 0 counts the camera's supported and unsupported observations.
// k_lag_add: one thread per (c, i) adds the partials of the frames in increasing f onto the state; the loads of eight
// frames are issued ahead of the eight dependent additions.
// Two launches whatever the frame count.  The file turns contraction off; f64 quotients and roots are the language's
// correctly rounded ones.
#include "mpe_internal.h"
#include "pose_rows.h"
#include "project64.h"
#include "reproject_select.h"

#pragma clang fp contract(off)

namespace mpe {

namespace {

constexpr int LG_THREADS = 256;
constexpr int LG_WIN = 2 * MPE_LAG_MAX_WINDOW + 1;
constexpr int LG_ADD_THREADS = 128;

struct LagK {
    int n_frames, frame_start, V, K, W, sub;
    double huber;
    PoseRows rows;                            // the table: rows.n_frames = n_table
    Selection sel;                            // n_persons and flags point at frame_start of the table's
    const double *xy;
    double *S;                                // [n_frames][V][K] partials of the call
    double *cost;                             // [V][K]
    unsigned long long *n_obs, *n_skipped;    // [V][K]
    unsigned long long *n_support, *n_unsupported;   // [V]
};

// the row of (g, t), -1 without one
__device__ inline int track_row(const PoseRows &r, int g, int t) {
    if (g < 0 || g >= r.n_frames) return -1;
    const int n = rows_in_frame(r, g);
    for (int p = 0; p < n; ++p) {
        const size_t fp = (size_t)g * r.pcap + p;
        if (r.tid[fp] == t && (r.joint_flags || r.flags[fp] != 0)) return p;
    }
    return -1;
}

__global__ void __launch_bounds__(LG_THREADS) k_lag_frame(const DevCfg *__restrict__ cfg, LagK a) {
    __shared__ int16_t s_row[MPE_TRACK_MAX_PERSONS * LG_WIN];
    __shared__ uint32_t s_ok[MPE_TRACK_MAX_PERSONS * LG_WIN];
    __shared__ uint32_t s_sup[MPE_TRACK_MAX_PERSONS];
    const int fl = blockIdx.x, tid = threadIdx.x;
    const int g0 = a.frame_start + fl, win = 2 * a.W + 1, pcap = a.rows.pcap, J = a.rows.J;
    const int np = rows_in_frame(a.rows, g0);
    for (int at = tid; at < pcap * win; at += LG_THREADS) {
        const int p = at / win, w = at % win, g = g0 - a.W + w;
        const int t = p < np ? a.rows.tid[(size_t)g0 * pcap + p] : -1;
        const int row = t >= 0 ? track_row(a.rows, g, t) : -1;
        uint32_t ok = 0;
        if (row >= 0) {
            const size_t fp = (size_t)g * pcap + row;
            const uint32_t flagged = flag_mask(a.rows, fp);
            for (int j = 0; j < J; ++j) {
                double X[3];
                load3(a.rows.poses, a.rows.pose_f64, fp * J + j, X);
                if (((flagged >> j) & 1u) && finite3(X[0], X[1], X[2])) ok |= 1u << j;
            }
        }
        s_row[at] = (int16_t)row;
        s_ok[at] = ok;
    }
    __syncthreads();
    for (int p = tid; p < pcap; p += LG_THREADS) {
        uint32_t sup = 0xFFFFFFFFu;
        for (int w = 0; w < win; ++w) sup &= s_ok[p * win + w];
        s_sup[p] = sup;
    }
    __syncthreads();
    const int n = a.V * a.K, zero = a.W * a.sub;
    for (int id = tid; id < n; id += LG_THREADS) {
        const int c = id / a.K, i = id % a.K;
        const int k = i - zero;
        const int s = k >= 0 ? k / a.sub : -((-k + a.sub - 1) / a.sub);      // floor(k / sub)
        const int r = k - s * a.sub;
        const double alpha = (double)r / (double)a.sub;
        const int wa = s + a.W;               // the window entry of frame f + s; wa + 1 <= 2W whenever r != 0
        const double *T = cfg->P[c], *dist = cfg->dist[c];
        const float *Kc = cfg->K[c];
        double acc = 0.0;
        unsigned long long n_sum = 0, n_skip = 0, n_sup = 0, n_unsup = 0;
        for (int p = 0; p < pcap; ++p) {
            const long long fp = (long long)fl * pcap + p;
            if (!sel_person(a.sel, fl, p, fp)) continue;
            uint32_t present = 0;
            const int head = sel_head(a.sel, fl, fp, c, &present);
            if (head < 0) continue;
            const uint32_t sup = s_sup[p];
            const int ra = s_row[p * win + wa], rb = r ? s_row[p * win + wa + 1] : 0;
            for (int j = 0; j < J; ++j) {
                if (!sel_joint(a.sel, fp, j, head, present)) continue;
                if (!((sup >> j) & 1u)) {
                    ++n_unsup;
                    continue;
                }
                ++n_sup;
                double X[3], pc[3];
                load3(a.rows.poses, a.rows.pose_f64, ((size_t)(g0 + s) * pcap + ra) * J + j, X);
                if (r) {
                    double Xb[3];
                    load3(a.rows.poses, a.rows.pose_f64, ((size_t)(g0 + s + 1) * pcap + rb) * J + j, Xb);
                    for (int d = 0; d < 3; ++d) X[d] = X[d] + alpha * (Xb[d] - X[d]);
                }
                to_camera(T, X[0], X[1], X[2], pc);
                if (!(pc[2] > 0.0)) {         // before the quotients: a skipped term computes nothing
                    ++n_skip;
                    continue;
                }
                const Proj pr = project_pc(pc, dist, Kc);
                if (!finite3(pr.px, pr.py, 0.0)) {
                    ++n_skip;
                    continue;
                }
                const double *o = a.xy + ((size_t)head * J + j) * 2;
                const double rx = pr.px - o[0], ry = pr.py - o[1];
                acc = acc + rho(sqrt(rx * rx + ry * ry), a.huber);
                ++n_sum;
            }
        }
        a.S[(size_t)fl * n + id] = acc;
        if (n_sum) atomicAdd(a.n_obs + id, n_sum);
        if (n_skip) atomicAdd(a.n_skipped + id, n_skip);
        if (i == 0) {
            if (n_sup) atomicAdd(a.n_support + c, n_sup);
            if (n_unsup) atomicAdd(a.n_unsupported + c, n_unsup);
        }
    }
}

__global__ void __launch_bounds__(LG_ADD_THREADS) k_lag_add(LagK a) {
    const int id = blockIdx.x * LG_ADD_THREADS + threadIdx.x, n = a.V * a.K;
    if (id >= n) return;
    double t = a.cost[id];
    for (int f0 = 0; f0 < a.n_frames; f0 += 8) {
        double v[8];
        for (int k = 0; k < 8; ++k) v[k] = f0 + k < a.n_frames ? a.S[(size_t)(f0 + k) * n + id] : 0.0;
        for (int k = 0; k < 8; ++k)
            if (f0 + k < a.n_frames) t = t + v[k];
    }
    a.cost[id] = t;
}

}  // namespace

size_t lag_counter_words(int V, int K) { return 2 * (size_t)V * K + 2 * (size_t)V; }

hipError_t launch_lag(hipStream_t s, const DevCfg *cfg, mpe_lag_state *st, const mpe_batch &b, const mpe_lag_args &x) {
    const int V = st->V, K = st->K;
    const size_t row0 = (size_t)x.frame_start * x.pcap;
    LagK a{x.n_frames, x.frame_start, V, K, st->W, st->sub, x.huber_px,
           PoseRows{x.n_table, x.pcap, x.n_joints, x.pose_f64, x.joint_flags, x.d_poses, x.d_flags, x.d_n_persons, x.d_tid},
           Selection{V, x.n_joints, x.joint_flags, x.joint_mask, x.threshold, b.d_frame_head_off, b.d_joint_mask, b.d_vp, x.d_persons,
                     x.d_n_persons + x.frame_start, x.d_flags + row0 * (x.joint_flags ? x.n_joints : 1)},
           b.d_xy, st->S, st->cost, st->ctr, st->ctr + (size_t)V * K, st->ctr + 2 * (size_t)V * K, st->ctr + 2 * (size_t)V * K + V};
    hipLaunchKernelGGL(k_lag_frame, dim3((unsigned)x.n_frames), dim3(LG_THREADS), 0, s, cfg, a);
    hipError_t e = hipGetLastError();
    if (e != hipSuccess) return e;
    ++st->launches;
    hipLaunchKernelGGL(k_lag_add, dim3((V * K + LG_ADD_THREADS - 1) / LG_ADD_THREADS), dim3(LG_ADD_THREADS), 0, s, a);
    if ((e = hipGetLastError()) != hipSuccess) return e;
    ++st->launches;
    return hipSuccess;
}

// the sums and the counts back to zero; stream-ordered memsets, no kernel
hipError_t launch_lag_reset(hipStream_t s, mpe_lag_state *st) {
    hipError_t e = hipMemsetAsync(st->cost, 0, (size_t)st->V * st->K * sizeof(double), s);
    if (e == hipSuccess) e = hipMemsetAsync(st->ctr, 0, lag_counter_words(st->V, st->K) * sizeof(unsigned long long), s);
    return e;
}

}  // namespace mpe
