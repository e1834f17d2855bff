// mpe_regroup_batch: the person proposals of a frame checked against the 3D poses they led to -- the cost of every
// (head, person) pair of the frame by mpe_refine_batch's projection lines, then heads released from rows they do not fit
// and free heads attached to rows that lack their camera, binary64, in the order include/mpe.h gives.
//
// k_regroup: ONE launch, one 256-thread workgroup per frame.  The rows [pcap][V], one named-bit per head and the persons'
// pose flags live in LDS (20.6 KB at the compiled caps pcap = 128, V = 32, 32767 heads); the cost table is the caller's
// d_cost, written by the workgroup that reads it back after a barrier.  Cost table: one lane per (head, person) pair, p
// fastest (the d_cost stores are consecutive); a lane reads its head's camera and joint mask once and folds the joints in
// increasing j.  Row check and release: one lane per row entry.  Attach: one wave per camera (cameras beyond four take
// turns); a round is a scan of the camera's free heads x open persons, lane per head, and a wave reduction over (cost,
// head, person); no barrier inside the rounds (the waves run different numbers of them).  Every count is an integer.
#include "mpe_internal.h"
#include "project64.h"
#include "frame_rows.h"

#pragma clang fp contract(off)

namespace mpe {

namespace {

constexpr int RG_THREADS = 256;
constexpr int RG_WAVES = RG_THREADS / 64;
static_assert(FRAME_ROWS_LDS + 32 <= 64 * 1024, "the rows, the named bits and the pose flags of a frame fit LDS");

struct RegroupK {
    int pcap, pose_f64, min_joints, min_views, hmax;
    uint32_t flags;
    double gate, clip;
    Selection sel;                            // the batch's heads and the rows with their flags (reproject_select.h)
    const int32_t *head_cam;
    const double *xy;
    const void *poses;
    int32_t *persons_out;                     // may be `persons`: an entry is read and written by the same lane
    uint8_t *change;
    int32_t *n_views;
    double *cost;
    int32_t *counts, *status, *sticky;
};

// the cost of head h (index into the batch's per-head arrays) against person p of frame f, -1 when unscored
__device__ inline double pair_cost(const DevCfg *cfg, const RegroupK &a, size_t fp, int h) {
    const double inf = __builtin_huge_val();
    const Selection &s = a.sel;
    const int c = a.head_cam[h];
    if (c < 0 || c >= s.V) return -1.0;
    const uint32_t present = s.head_joint_mask[h] & s.joint_mask;
    double sum = 0.0;
    int n = 0;
    for (int j = 0; j < s.J; ++j) {
        if (!((present >> j) & 1u)) continue;
        const size_t hj = (size_t)h * s.J + j, pj = fp * s.J + j;
        if (!(s.vp[hj * 2] > s.threshold)) continue;
        if (s.joint_flags && s.flags[pj] == 0) continue;
        double X[3];
        load3(a.poses, a.pose_f64, pj, X);
        const double X0 = X[0], X1 = X[1], X2 = X[2];
        if (!finite3(X0, X1, X2)) continue;
        const Proj p = project(cfg->P[c], cfg->dist[c], cfg->K[c], X0, X1, X2);
        if (!(p.pc2 > 0.0)) continue;
        const double rx = p.px - a.xy[hj * 2], ry = p.py - a.xy[hj * 2 + 1];
        double e = sqrt(rx * rx + ry * ry);
        if (!(e < inf)) continue;
        if (a.clip > 0.0 && e > a.clip) e = a.clip;
        sum = sum + e;
        ++n;
    }
    if (n < a.min_joints) return -1.0;
    const double cost = sum / (double)n;
    return cost < inf ? cost : -1.0;
}

// (c1, h1, p1) orders before (c0, h0, p0): least cost, then the lowest head, then the lowest person
__device__ inline bool before(double c1, int h1, int p1, double c0, int h0, int p0) {
    return c1 < c0 || (c1 == c0 && (h1 < h0 || (h1 == h0 && p1 < p0)));
}

__global__ void __launch_bounds__(RG_THREADS) k_regroup(const DevCfg *__restrict__ cfg, RegroupK a) {
    __shared__ int32_t s_row[MPE_REGROUP_MAX_PERSONS * MPE_MAX_CAMERAS];      // [pcap][V], as the rows stand now
    __shared__ uint32_t s_named[NAMED_WORDS];                                // bit h: a row names head h now
    __shared__ uint8_t s_pose[MPE_REGROUP_MAX_PERSONS];                      // person p has a pose
    __shared__ int32_t s_cnt[4];
    __shared__ int32_t s_bad;
    const int f = blockIdx.x, tid = threadIdx.x, V = a.sel.V, pcap = a.pcap;
    const FrameRows fr = frame_rows_load<RG_THREADS>(a.sel, pcap, a.hmax, f, s_row, s_pose, s_named, &s_bad);
    const int h0 = fr.h0, H = fr.H, np = fr.np;
    const bool over = fr.over;
    const size_t fp0 = fr.fp0;
    const int entries = pcap * V;
    if (tid < 4) s_cnt[tid] = 0;
    __syncthreads();

    // the cost table: every head of the frame against every row
    const long long pairs = (long long)H * pcap;
    for (long long i = tid; i < pairs; i += RG_THREADS) {
        const int hh = (int)(i / pcap), p = (int)(i - (long long)hh * pcap);
        a.cost[(size_t)(h0 + hh) * pcap + p] = s_pose[p] ? pair_cost(cfg, a, fp0 + p, h0 + hh) : -1.0;
    }

    frame_rows_mark<RG_THREADS>(fr, V, a.head_cam, s_row, s_named, &s_bad);
    __syncthreads();                          // also: this workgroup's d_cost stores are visible to it from here on
    const bool copy = frame_rows_copy(fr, &s_bad);

    if (!copy && (a.flags & MPE_REGROUP_RELEASE)) {
        for (int i = tid; i < np * V; i += RG_THREADS) {
            const int h = s_row[i], p = i / V;
            if (h < 0 || !s_pose[p]) continue;
            const double x = a.cost[(size_t)(h0 + h) * pcap + p];
            if (x >= 0.0 && !(x < a.gate)) {
                s_row[i] = -1;
                atomicAnd(&s_named[h >> 5], ~(1u << (h & 31)));
            }
        }
    }
    __syncthreads();

    if (!copy && (a.flags & MPE_REGROUP_ATTACH)) {
        const int lane = tid & 63;
        for (int c = tid >> 6; c < V; c += RG_WAVES) {
            for (;;) {
                double bc = __builtin_huge_val();
                int bh = 0x7fffffff, bp = 0x7fffffff;
                for (int hh = lane; hh < H; hh += 64) {
                    if (a.head_cam[h0 + hh] != c || ((s_named[hh >> 5] >> (hh & 31)) & 1u)) continue;
                    const double *row = a.cost + (size_t)(h0 + hh) * pcap;
                    for (int p = 0; p < np; ++p) {
                        if (!s_pose[p] || s_row[p * V + c] >= 0) continue;
                        const double x = row[p];
                        if (x >= 0.0 && x < a.gate && before(x, hh, p, bc, bh, bp)) bc = x, bh = hh, bp = p;
                    }
                }
                for (int off = 32; off; off >>= 1) {
                    const double oc = __shfl_xor(bc, off);
                    const int oh = __shfl_xor(bh, off), op = __shfl_xor(bp, off);
                    if (before(oc, oh, op, bc, bh, bp)) bc = oc, bh = oh, bp = op;
                }
                if (bh == 0x7fffffff) break;  // the same in every lane: no linkable pair is left
                if (lane == 0) {
                    s_row[bp * V + c] = bh;
                    atomicOr(&s_named[bh >> 5], 1u << (bh & 31));
                }
                __threadfence_block();
            }
        }
    }
    __syncthreads();

    for (int i = tid; i < entries; i += RG_THREADS) {
        const int was = a.sel.persons[fp0 * V + i], now = s_row[i];
        int code = 0;
        if (now != was) code = (was >= 0 ? 1 : 0) | (now >= 0 ? 2 : 0);
        a.persons_out[fp0 * V + i] = now;
        a.change[fp0 * V + i] = (uint8_t)code;
        if (code & 1) atomicAdd(&s_cnt[0], 1);
        if (code & 2) atomicAdd(&s_cnt[1], 1);
    }
    for (int p = tid; p < pcap; p += RG_THREADS) {
        int nv = 0;
        if (p < np)
            for (int c = 0; c < V; ++c) nv += s_row[p * V + c] >= 0;
        a.n_views[fp0 + p] = nv;
        if (!copy && s_pose[p] && nv < a.min_views) atomicAdd(&s_cnt[3], 1);
    }
    if (!copy)
        for (int hh = tid; hh < H; hh += RG_THREADS)
            if (!((s_named[hh >> 5] >> (hh & 31)) & 1u)) atomicAdd(&s_cnt[2], 1);
    __syncthreads();
    if (tid < 4) a.counts[(size_t)f * 4 + tid] = s_cnt[tid];
    if (tid == 0) {
        a.status[f] = over ? MPE_REGROUP_OVER_CAP : s_bad ? MPE_REGROUP_BAD_ROWS : 0;
        if (over && a.sticky) atomicOr(a.sticky, 1);
    }
}

}  // namespace

hipError_t launch_regroup(hipStream_t s, const DevCfg *cfg, int V, int min_views, int hmax, int32_t *sticky, const mpe_batch &b,
                          const mpe_regroup_args &x) {
    RegroupK a{x.pcap, x.pose_f64, x.min_joints, min_views, hmax, x.flags, x.gate_px, x.clip_px,
               Selection{V, x.n_joints, x.joint_flags, x.joint_mask, x.threshold, b.d_frame_head_off, b.d_joint_mask, b.d_vp, x.d_persons,
                         x.d_n_persons, x.d_flags},
               b.d_head_cam, b.d_xy, x.d_poses, x.d_persons_out, x.d_change, x.d_n_views, x.d_cost, x.d_counts, x.d_status, sticky};
    hipLaunchKernelGGL(k_regroup, dim3((unsigned)x.n_frames), dim3(RG_THREADS), 0, s, cfg, a);
    return hipGetLastError();
}

}  // namespace mpe
