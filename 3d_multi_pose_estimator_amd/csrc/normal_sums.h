// One pass of a per-camera Levenberg-Marquardt fit whose points are held fixed: every observation of every camera reduced
// into the camera's SUMS = N(N+1)/2 + N + 1 sums (the upper triangle of the N x N normal equations row by row, their
// right-hand side and the cost), binary64, in the order include/mpe.h gives, so that the sums are the same bits however a
// recording is cut into batches.  calib.hip (N = 6) and camfit.hip (N = 13) instantiate it; each brings a family F:
//   F::N, F::THREADS (the workgroup), F::RECORDS (records per LDS tile) and
//   F::observe(a, f, p, j, c, rec) -> REC_*: the record of (frame f, row p, joint j, camera c).  a.cams is F's alone.
//
// The record is Jx[N], rx, w, Jy[N], ry, rho(e): 2N + 4 doubles, the weight at W = N + 1, the y half from Y = N + 2, so
// that every term is rec[W] * (rec[k]*rec[l] + rec[Y+k]*rec[Y+l]) with l = N for the right-hand side and the fold has one
// form.  The records lie at an odd stride, 2N + 5: the lanes of a wave write entry k of consecutive records two to a
// bank, not 32.
//
// k_normal_frame: one workgroup per frame.  A lane per (person, joint, camera) writes the observation's record to LDS and
// a byte that says whether it is summed, skipped or absent; then thread (c, q) folds the records of camera c in (p, j)
// order into S_f[c][q].  V * SUMS chains over F::THREADS threads: SLOTS chains per thread, held in registers, SLOTS a
// template argument picked by V so that five cameras do not carry the registers of thirty-two.  The chains of a thread
// advance together record by record (they are independent, so their latencies overlap); each chain is still a left fold.
// F::RECORDS records fit LDS; a frame with more is taken in tiles of whole (p, j) pairs and the folds are carried in
// registers from tile to tile, in the same order.  The partials go to a workspace sized at create; the (c, SUMS - 1)
// thread counts the camera's summed and skipped records on the way and adds them to the state with two integer atomics
// (the only atomics: no f64 atomic anywhere).
// k_normal_add: one thread per (c, q) adds the partials of the frames in increasing f onto the state; the loads of eight
// frames are issued ahead of the eight dependent additions.
// Two launches whatever the frame count.  Contraction is off from this header on; f64 quotients and roots are the
// language's correctly rounded ones.  DESIGN.md 7.9 has the sizing of the two instantiations.
#pragma once
#include "mpe_internal.h"
#include "project64.h"
#include "reproject_select.h"

#pragma clang fp contract(off)                // the folds below are written out: from here to the end of the including file

namespace mpe {

enum : uint8_t { REC_ABSENT = 0, REC_SUMMED = 1, REC_SKIPPED = 2 };

struct NormalK {
    int n_frames, pcap, V, J, pose_f64;
    double huber;
    Selection sel;
    const double *xy;
    const void *poses;
    const DevCfg *cfg;                        // the context's cameras, for a family that does not fit all of them
    const double *cams;                       // [V][cam_width] the trial cameras
    double *S;                                // [n_frames][V][SUMS] partials of the call
    double *acc;                              // [V][SUMS]
    unsigned long long *n_obs, *n_skipped;    // [V]
};

constexpr int NORMAL_ADD_THREADS = 128;

constexpr int normal_sums(int N) { return N * (N + 1) / 2 + N + 1; }

template <class F>
constexpr int normal_slots(int V) { return (V * normal_sums(F::N) + F::THREADS - 1) / F::THREADS; }

template <class F, int SLOTS>
__global__ void __launch_bounds__(F::THREADS) k_normal_frame(NormalK a) {
    constexpr int N = F::N, TRI = N * (N + 1) / 2, SUMS = normal_sums(N), REC = 2 * N + 4, STRIDE = REC + 1, W = N + 1, Y = N + 2;
    static_assert(F::RECORDS >= MPE_MAX_CAMERAS, "a tile holds at least one (person, joint) pair of every camera");
    __shared__ double s_rec[F::RECORDS * STRIDE];
    __shared__ uint8_t s_kind[F::RECORDS];
    const int f = blockIdx.x, tid = threadIdx.x;
    // this thread's (c, q) and the two record entries q multiplies: A_kl = Jx_k*Jx_l + Jy_k*Jy_l, g_k = Jx_k*rx + Jy_k*ry
    // (rx and ry sit behind the Jacobian rows, at entry N), C = rho
    int cam[SLOTS], ek[SLOTS], el[SLOTS];
    double acc[SLOTS];
#pragma unroll
    for (int s = 0; s < SLOTS; ++s) {
        const int id = tid + s * F::THREADS;
        const int q = id % SUMS;
        cam[s] = id < a.V * SUMS ? id / SUMS : -1;
        int k = 0, l = q;
        if (q < TRI) {
            while (l >= N - k) l -= N - k, ++k;
            l += k;
        } else {
            k = q - TRI, l = N;
        }
        ek[s] = q == SUMS - 1 ? -1 : k;
        el[s] = l;
        acc[s] = 0.0;
    }
    unsigned long long n_sum = 0, n_skip = 0;
    int np = a.sel.n_persons[f];
    np = np < 0 ? 0 : np > a.pcap ? a.pcap : np;
    const int total = np * a.J;               // (p, j) pairs of the frame, in fold order
    const int tile = F::RECORDS / a.V;
    for (int pj0 = 0; pj0 < total; pj0 += tile) {
        const int n = total - pj0 < tile ? total - pj0 : tile;
        for (int r = tid; r < n * a.V; r += F::THREADS) {
            const int pj = pj0 + r / a.V;
            s_kind[r] = F::observe(a, f, pj / a.J, pj % a.J, r % a.V, s_rec + r * STRIDE);
        }
        __syncthreads();
        const int n_fold = SLOTS == 1 && cam[0] < 0 ? 0 : n;      // an only chain: the test for a thread without one is the bound
        for (int i = 0; i < n_fold; ++i) {
#pragma unroll
            for (int s = 0; s < SLOTS; ++s) {
                if (SLOTS > 1 && cam[s] < 0) continue;
                const int r = i * a.V + cam[s];
                const uint8_t kind = s_kind[r];
                const double *rec = s_rec + r * STRIDE;
                if (ek[s] < 0) {
                    n_sum += kind == REC_SUMMED;
                    n_skip += kind == REC_SKIPPED;
                    if (kind == REC_SUMMED) acc[s] = acc[s] + rec[REC - 1];
                } else if (kind == REC_SUMMED) {
                    acc[s] = acc[s] + rec[W] * (rec[ek[s]] * rec[el[s]] + rec[Y + ek[s]] * rec[Y + el[s]]);
                }
            }
        }
        __syncthreads();
    }
#pragma unroll
    for (int s = 0; s < SLOTS; ++s) {
        if (cam[s] < 0) continue;
        a.S[(size_t)f * a.V * SUMS + tid + s * F::THREADS] = acc[s];
        if (ek[s] < 0) {
            if (n_sum) atomicAdd(a.n_obs + cam[s], n_sum);
            if (n_skip) atomicAdd(a.n_skipped + cam[s], n_skip);
        }
    }
}

template <int SUMS>
__global__ void __launch_bounds__(NORMAL_ADD_THREADS) k_normal_add(NormalK a) {
    const int id = blockIdx.x * NORMAL_ADD_THREADS + threadIdx.x, n = a.V * SUMS;
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

// One pass over the frames of a call onto the state: the frame kernel with the least of the chain counts S0 < S1 < S2
// that covers the state's cameras (S2 covers the cap), then the add kernel
template <class F, int S0, int S1, int S2>
hipError_t launch_normal_sums(hipStream_t s, const DevCfg *cfg, normal_state *st, const mpe_batch &b, const mpe_calib_args &x) {
    static_assert(S0 < S1 && S1 < S2 && S2 == normal_slots<F>(MPE_MAX_CAMERAS), "the last chain count is the cap's");
    const int V = st->V, slots = normal_slots<F>(V), sums = normal_sums(F::N);
    const NormalK a{x.n_frames, x.pcap, V, x.n_joints, x.pose_f64, x.huber_px,
                    Selection{V, x.n_joints, x.joint_flags, x.joint_mask, x.threshold, b.d_frame_head_off, b.d_joint_mask, b.d_vp, x.d_persons,
                              x.d_n_persons, x.d_flags},
                    b.d_xy, x.d_poses, cfg, st->cams, st->S, st->acc, st->n_obs, st->n_skipped};
    const dim3 grid((unsigned)x.n_frames), block(F::THREADS);
    if (slots <= S0)
        hipLaunchKernelGGL((k_normal_frame<F, S0>), grid, block, 0, s, a);
    else if (slots <= S1)
        hipLaunchKernelGGL((k_normal_frame<F, S1>), grid, block, 0, s, a);
    else
        hipLaunchKernelGGL((k_normal_frame<F, S2>), grid, block, 0, s, a);
    hipError_t e = hipGetLastError();
    if (e != hipSuccess) return e;
    ++st->launches;
    hipLaunchKernelGGL(k_normal_add<sums>, dim3((V * sums + NORMAL_ADD_THREADS - 1) / NORMAL_ADD_THREADS), dim3(NORMAL_ADD_THREADS), 0, s, a);
    if ((e = hipGetLastError()) != hipSuccess) return e;
    ++st->launches;
    return hipSuccess;
}

inline size_t normal_workspace_doubles(const normal_state *st) { return (size_t)st->max_frames * st->V * st->n_sums; }

// the sums and the counts back to zero; stream-ordered memsets, no kernel
inline hipError_t launch_normal_clear(hipStream_t s, normal_state *st) {
    hipError_t e = hipMemsetAsync(st->acc, 0, (size_t)st->V * st->n_sums * sizeof(double), s);
    if (e == hipSuccess) e = hipMemsetAsync(st->n_obs, 0, (size_t)st->V * sizeof(unsigned long long), s);
    if (e == hipSuccess) e = hipMemsetAsync(st->n_skipped, 0, (size_t)st->V * sizeof(unsigned long long), s);
    return e;
}

}  // namespace mpe
