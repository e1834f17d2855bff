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

#pragma clang fp contract(off)

namespace mpe {

namespace {

constexpr int RG_THREADS = 256;
constexpr int RG_WAVES = RG_THREADS / 64;
constexpr int RG_NAMED_WORDS = 1024;          // one bit per head of a frame: max_heads_per_frame <= 32767 (mpe_create)
static_assert(MPE_REGROUP_MAX_PERSONS * MPE_MAX_CAMERAS * 4 + RG_NAMED_WORDS * 4 + MPE_REGROUP_MAX_PERSONS + 32 <= 64 * 1024,
              "the rows, the named bits and the pose flags of a frame fit LDS");

struct RegroupK {
    int pcap, V, J, pose_f64, joint_flags, min_joints, min_views, hmax;
    uint32_t joint_mask, flags;
    float threshold;
    double gate, clip;
    const int32_t *frame_head_off, *head_cam;
    const uint32_t *head_joint_mask;
    const float *vp;
    const double *xy;
    const int32_t *persons, *n_persons;
    const void *poses;
    const uint8_t *pflags;
    int32_t *persons_out;                     // may be `persons`: an entry is read and written by the same lane
    uint8_t *change;
    int32_t *n_views;
    double *cost;
    int32_t *counts, *status, *sticky;
};

// the cost of head h (index into the batch's per-head arrays) against person p of frame f, -1 when unscored
__device__ inline double pair_cost(const DevCfg *cfg, const RegroupK &a, size_t fp, int h) {
    const double inf = __builtin_huge_val();
    const int c = a.head_cam[h];
    if (c < 0 || c >= a.V) return -1.0;
    const uint32_t present = a.head_joint_mask[h] & a.joint_mask;
    double sum = 0.0;
    int n = 0;
    for (int j = 0; j < a.J; ++j) {
        if (!((present >> j) & 1u)) continue;
        const size_t hj = (size_t)h * a.J + j, pj = fp * a.J + j;
        if (!(a.vp[hj * 2] > a.threshold)) continue;
        if (a.joint_flags && a.pflags[pj] == 0) continue;
        double X0, X1, X2;
        if (a.pose_f64) {
            const double *q = static_cast<const double *>(a.poses) + pj * 3;
            X0 = q[0], X1 = q[1], X2 = q[2];
        } else {
            const float *q = static_cast<const float *>(a.poses) + pj * 3;
            X0 = (double)q[0], X1 = (double)q[1], X2 = (double)q[2];
        }
        if (!finite3(X0, X1, X2)) continue;
        const Proj p = project(cfg, c, X0, X1, X2);
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
    __shared__ uint32_t s_named[RG_NAMED_WORDS];                             // bit h: a row names head h now
    __shared__ uint8_t s_pose[MPE_REGROUP_MAX_PERSONS];                      // person p has a pose
    __shared__ int32_t s_cnt[4];
    __shared__ int32_t s_bad;
    const int f = blockIdx.x, tid = threadIdx.x, V = a.V, pcap = a.pcap;
    const int h0 = a.frame_head_off[f], H = a.frame_head_off[f + 1] - h0;
    int np = a.n_persons[f];
    np = np < 0 ? 0 : np > pcap ? pcap : np;
    const bool over = H > a.hmax;
    const size_t fp0 = (size_t)f * pcap;
    const int entries = pcap * V;

    for (int i = tid; i < entries; i += RG_THREADS) s_row[i] = a.persons[fp0 * V + i];
    for (int p = tid; p < pcap; p += RG_THREADS) s_pose[p] = p < np && (a.joint_flags || a.pflags[fp0 + p] != 0);
    if (!over)
        for (int w = tid; w < (H + 31) / 32; w += RG_THREADS) s_named[w] = 0;
    if (tid < 4) s_cnt[tid] = 0;
    if (tid == 0) s_bad = 0;
    __syncthreads();

    // the cost table: every head of the frame against every row
    const long long pairs = (long long)H * pcap;
    for (long long i = tid; i < pairs; i += RG_THREADS) {
        const int hh = (int)(i / pcap), p = (int)(i - (long long)hh * pcap);
        a.cost[(size_t)(h0 + hh) * pcap + p] = s_pose[p] ? pair_cost(cfg, a, fp0 + p, h0 + hh) : -1.0;
    }

    // the rows checked, every named head marked
    if (!over)
        for (int i = tid; i < np * V; i += RG_THREADS) {
            const int e = s_row[i], c = i % V;
            if (e < 0) continue;
            bool bad = e >= H || a.head_cam[h0 + e] != c;
            if (!bad) bad = ((atomicOr(&s_named[e >> 5], 1u << (e & 31)) >> (e & 31)) & 1u) != 0;
            if (bad) s_bad = 1;
        }
    __syncthreads();                          // also: this workgroup's d_cost stores are visible to it from here on
    const bool copy = over || s_bad != 0;

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
        const int was = a.persons[fp0 * V + i], now = s_row[i];
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
    RegroupK a{x.pcap, V, x.n_joints, x.pose_f64, x.joint_flags, x.min_joints, min_views, hmax, x.joint_mask, x.flags, x.threshold,
               x.gate_px, x.clip_px, b.d_frame_head_off, b.d_head_cam, b.d_joint_mask, b.d_vp, b.d_xy, x.d_persons, x.d_n_persons,
               x.d_poses, x.d_flags, x.d_persons_out, x.d_change, x.d_n_views, x.d_cost, x.d_counts, x.d_status, sticky};
    hipLaunchKernelGGL(k_regroup, dim3((unsigned)x.n_frames), dim3(RG_THREADS), 0, s, cfg, a);
    return hipGetLastError();
}

}  // namespace mpe
