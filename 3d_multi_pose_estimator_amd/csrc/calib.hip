// mpe_calib_batch: one pass of the extrinsics calibration -- every observation of every camera reduced into the camera's 28
// sums (the 6 x 6 normal equations of a rigid perturbation, their right-hand side and the cost), binary64, in the order
// include/mpe.h gives, so that the sums are the same bits however a recording is cut into batches.
//
// k_calib_frame: one workgroup per frame.  A lane per (person, joint, camera) writes the observation's record to LDS --
// Jx[6], rx, w, Jy[6], ry, rho(e): 16 doubles at a stride of 17 -- and a byte that says whether it is summed, skipped or absent; then thread
// (c, q) folds the records of camera c in (p, j) order into S_f[c][q].  V * 28 threads fold (at most 896: up to four (c, q)
// per thread, held in registers).  CB_RECORDS records fit LDS; a frame with more is taken in tiles of whole (p, j) pairs
// and the folds are carried in registers from tile to tile, in the same order.  The partials go to a workspace sized at
// create; the (c, 27) thread counts the camera's summed and skipped records on the way and adds them to the state with two
// integer atomics (the only atomics: no f64 atomic anywhere).
// k_calib_add: one thread per (c, q) adds the partials of the frames in increasing f onto the state; the loads of eight
// frames are issued ahead of the eight dependent additions.
// Two launches whatever the frame count.  The file turns contraction off; f64 quotients and roots are the language's
// correctly rounded ones.
#include "mpe_internal.h"
#include "project64.h"
#include "reproject_select.h"

#pragma clang fp contract(off)

namespace mpe {

namespace {

constexpr int CB_THREADS = 256;
constexpr int CB_REC = 16;                    // doubles per record
constexpr int CB_STRIDE = CB_REC + 1;         // an odd record stride: the lanes of a wave write entry k of consecutive records two to a bank, not 32
constexpr int CB_RECORDS = 384;               // records per tile: 51 KiB + 384 bytes of LDS, three workgroups per CU
constexpr int CB_SLOTS = (MPE_MAX_CAMERAS * MPE_CALIB_SUMS + CB_THREADS - 1) / CB_THREADS;
constexpr int CB_ADD_THREADS = 128;
static_assert(CB_RECORDS >= MPE_MAX_CAMERAS, "a tile holds at least one (person, joint) pair of every camera");

enum : uint8_t { REC_ABSENT = 0, REC_SUMMED = 1, REC_SKIPPED = 2 };

struct CalibK {
    int n_frames, pcap, V, J, pose_f64;
    double huber;
    Selection sel;
    const double *xy;
    const void *poses;
    const double *E;                          // [V][12] trial extrinsics
    double *S;                                // [n_frames][V][28] partials of the call
    double *acc;                              // [V][28]
    unsigned long long *n_obs, *n_skipped;    // [V]
};

// the record of (frame f, row p, joint j, camera c) -> REC_*
__device__ inline uint8_t observe(const DevCfg *cfg, const CalibK &a, int f, int p, int j, int c, double *rec) {
    const long long fp = (long long)f * a.pcap + p;
    if (!sel_person(a.sel, f, p, fp)) return REC_ABSENT;
    uint32_t present = 0;
    const int head = sel_head(a.sel, f, fp, c, &present);
    if (!sel_joint(a.sel, fp, j, head, present)) return REC_ABSENT;
    double X[3], pc[3];
    load3(a.poses, a.pose_f64, (size_t)fp * a.J + j, X);
    if (!finite3(X[0], X[1], X[2])) return REC_SKIPPED;
    to_camera(a.E + 12 * c, X[0], X[1], X[2], pc);
    if (!(pc[2] > 0.0)) return REC_SKIPPED;   // before the quotients: a skipped record computes nothing
    const float *K = cfg->K[c];
    const Proj pr = project_pc(pc, cfg->dist[c], K);
    if (!finite3(pr.px, pr.py, 0.0)) return REC_SKIPPED;
    const double *o = a.xy + ((size_t)head * a.J + j) * 2;
    const double rx = pr.px - o[0], ry = pr.py - o[1];
    const double e = sqrt(rx * rx + ry * ry);
    // the derivatives of (h0, h1) by the camera-frame point, through the shared tail; then the six-vector of a rigid
    // perturbation (w, tau) of the camera: d pc = w x pc + tau
    const double fd = radial_slope(cfg->dist[c], pr);
    const double da[3] = {1.0 / pc[2], 0.0, (-pr.h0) / pc[2]}, db[3] = {0.0, 1.0 / pc[2], (-pr.h1) / pc[2]};
    double cx[3], cy[3];
    for (int k = 0; k < 3; ++k) jacobian_tail(pr, K, fd, da[k], db[k], cx + k, cy + k);
    rec[0] = cx[2] * pc[1] - cx[1] * pc[2];
    rec[1] = cx[0] * pc[2] - cx[2] * pc[0];
    rec[2] = cx[1] * pc[0] - cx[0] * pc[1];
    rec[3] = cx[0], rec[4] = cx[1], rec[5] = cx[2];
    rec[6] = rx;
    rec[7] = huber_weight(e, a.huber);
    rec[8] = cy[2] * pc[1] - cy[1] * pc[2];
    rec[9] = cy[0] * pc[2] - cy[2] * pc[0];
    rec[10] = cy[1] * pc[0] - cy[0] * pc[1];
    rec[11] = cy[0], rec[12] = cy[1], rec[13] = cy[2];
    rec[14] = ry;
    rec[15] = rho(e, a.huber);
    return REC_SUMMED;
}

__global__ void __launch_bounds__(CB_THREADS) k_calib_frame(const DevCfg *__restrict__ cfg, CalibK a) {
    __shared__ double s_rec[CB_RECORDS * CB_STRIDE];
    __shared__ uint8_t s_kind[CB_RECORDS];
    const int f = blockIdx.x, tid = threadIdx.x;
    // this thread's (c, q) and the two record entries q multiplies: A_kl = Jx_k*Jx_l + Jy_k*Jy_l, g_k = Jx_k*rx + Jy_k*ry
    // (rx and ry sit behind the Jacobian rows, at entry 6), C = rho
    int cam[CB_SLOTS], ek[CB_SLOTS], el[CB_SLOTS];
    double acc[CB_SLOTS];
    for (int s = 0; s < CB_SLOTS; ++s) {
        const int id = tid + s * CB_THREADS;
        const int q = id % MPE_CALIB_SUMS;
        cam[s] = id < a.V * MPE_CALIB_SUMS ? id / MPE_CALIB_SUMS : -1;
        int k = 0, l = q;
        if (q < 21) {
            while (l >= 6 - k) l -= 6 - k, ++k;
            l += k;
        } else {
            k = q - 21, l = 6;
        }
        ek[s] = q == 27 ? -1 : k;
        el[s] = l;
        acc[s] = 0.0;
    }
    unsigned long long n_sum = 0, n_skip = 0;
    int np = a.sel.n_persons[f];
    np = np < 0 ? 0 : np > a.pcap ? a.pcap : np;
    const int total = np * a.J;               // (p, j) pairs of the frame, in fold order
    const int tile = CB_RECORDS / a.V;
    for (int pj0 = 0; pj0 < total; pj0 += tile) {
        const int n = total - pj0 < tile ? total - pj0 : tile;
        for (int r = tid; r < n * a.V; r += CB_THREADS) {
            const int pj = pj0 + r / a.V;
            s_kind[r] = observe(cfg, a, f, pj / a.J, pj % a.J, r % a.V, s_rec + r * CB_STRIDE);
        }
        __syncthreads();
#pragma unroll
        for (int s = 0; s < CB_SLOTS; ++s) {
            if (cam[s] < 0) continue;
            for (int i = 0; i < n; ++i) {
                const int r = i * a.V + cam[s];
                const uint8_t kind = s_kind[r];
                const double *rec = s_rec + r * CB_STRIDE;
                if (ek[s] < 0) {
                    n_sum += kind == REC_SUMMED;
                    n_skip += kind == REC_SKIPPED;
                    if (kind == REC_SUMMED) acc[s] = acc[s] + rec[15];
                } else if (kind == REC_SUMMED) {
                    acc[s] = acc[s] + rec[7] * (rec[ek[s]] * rec[el[s]] + rec[8 + ek[s]] * rec[8 + el[s]]);
                }
            }
        }
        __syncthreads();
    }
#pragma unroll
    for (int s = 0; s < CB_SLOTS; ++s) {
        if (cam[s] < 0) continue;
        a.S[(size_t)f * a.V * MPE_CALIB_SUMS + tid + s * CB_THREADS] = acc[s];
        if (ek[s] < 0) {
            if (n_sum) atomicAdd(a.n_obs + cam[s], n_sum);
            if (n_skip) atomicAdd(a.n_skipped + cam[s], n_skip);
        }
    }
}

__global__ void __launch_bounds__(CB_ADD_THREADS) k_calib_add(CalibK a) {
    const int id = blockIdx.x * CB_ADD_THREADS + threadIdx.x, n = a.V * MPE_CALIB_SUMS;
    if (id >= n) return;
    double t = a.acc[id];
    for (int f0 = 0; f0 < a.n_frames; f0 += 8) {
        double v[8];
        for (int k = 0; k < 8; ++k) v[k] = f0 + k < a.n_frames ? a.S[(size_t)(f0 + k) * n + id] : 0.0;
        for (int k = 0; k < 8; ++k)
            if (f0 + k < a.n_frames) t = t + v[k];
    }
    a.acc[id] = t;
}

}  // namespace

size_t calib_workspace_doubles(int max_frames, int V) { return (size_t)max_frames * V * MPE_CALIB_SUMS; }

hipError_t launch_calib(hipStream_t s, const DevCfg *cfg, int V, mpe_calib_state *st, const mpe_batch &b, const mpe_calib_args &x) {
    CalibK a{x.n_frames, x.pcap, V, x.n_joints, x.pose_f64, x.huber_px,
             Selection{V, x.n_joints, x.joint_flags, x.joint_mask, x.threshold, b.d_frame_head_off, b.d_joint_mask, b.d_vp, x.d_persons,
                       x.d_n_persons, x.d_flags},
             b.d_xy, x.d_poses, st->E, st->S, st->acc, st->n_obs, st->n_skipped};
    hipLaunchKernelGGL(k_calib_frame, dim3((unsigned)x.n_frames), dim3(CB_THREADS), 0, s, cfg, a);
    hipError_t e = hipGetLastError();
    if (e != hipSuccess) return e;
    ++st->launches;
    hipLaunchKernelGGL(k_calib_add, dim3((V * MPE_CALIB_SUMS + CB_ADD_THREADS - 1) / CB_ADD_THREADS), dim3(CB_ADD_THREADS), 0, s, a);
    if ((e = hipGetLastError()) != hipSuccess) return e;
    ++st->launches;
    return hipSuccess;
}

// the sums and the counts back to zero; stream-ordered memsets, no kernel
hipError_t launch_calib_clear(hipStream_t s, mpe_calib_state *st, int V) {
    hipError_t e = hipMemsetAsync(st->acc, 0, (size_t)V * MPE_CALIB_SUMS * sizeof(double), s);
    if (e == hipSuccess) e = hipMemsetAsync(st->n_obs, 0, (size_t)V * sizeof(unsigned long long), s);
    if (e == hipSuccess) e = hipMemsetAsync(st->n_skipped, 0, (size_t)V * sizeof(unsigned long long), s);
    return e;
}

}  // namespace mpe
