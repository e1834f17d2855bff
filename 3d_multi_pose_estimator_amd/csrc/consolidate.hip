// mpe_consolidate_batch: the two repairs mpe_regroup_batch leaves open -- rows whose poses lie on one body are merged, and
// the skeletons no row names found new rows where their rays meet -- binary64, in the order include/mpe.h gives.
//
// k_consolidate: ONE launch, one 256-thread workgroup per frame.  The rows [pcap][V], one named-bit per head, the persons'
// pose flags and camera sets, the free heads (at most 64) with their cameras, vote words and unit rays live in LDS (49.6 KB
// at the compiled caps); the two tables are the caller's d_dist and d_pair, written by the workgroup that reads them back
// after a barrier.  Parallel: the row check (lane per entry), the pose distances (lane per (p, q)), the free heads in head
// order (wave 0: a ballot and a prefix per 64 heads, no atomics), their rays (lane per (head, joint), rays64.h's lines),
// the pair costs (lane per (a, b)).  The two greedy passes run in wave 0 while the other waves wait at the next barrier: a
// round is a lane-strided scan and a wave reduction over the key tuple; the growth of a tentative row has one lane per free
// head.  Every lane reaches every workgroup barrier.  Every count is an integer.
#include "mpe_internal.h"
#include "project64.h"
#include "frame_rows.h"
#include "rays64.h"

#pragma clang fp contract(off)

namespace mpe {

namespace {

constexpr int CS_THREADS = 256;
constexpr int CS_NONE = 0x7fffffff;
static_assert(MPE_CONSOLIDATE_MAX_FREE == 64, "the free heads of a frame are the lanes of a wave and the bits of a word");
static_assert(FRAME_ROWS_LDS + MPE_REGROUP_MAX_PERSONS * 5 + MPE_CONSOLIDATE_RAY_DOUBLES * 8 + MPE_CONSOLIDATE_MAX_FREE * 12 +
                      MPE_MAX_CAMERAS * 24 + 64 <= 64 * 1024,
              "the rows, the named bits, the pose flags and the rays of the free heads of a frame fit LDS");

struct ConsolidateK {
    int pcap, V, J, pose_f64, joint_flags, min_joints, found_min_views, fcap, hmax;
    uint32_t joint_mask, flags;
    float threshold;
    double merge_m, found_m, clip;
    const int32_t *frame_head_off, *head_cam;
    const uint32_t *head_joint_mask;
    const float *vp;
    const double *xy;
    const int32_t *persons, *n_persons;
    const void *poses;
    const uint8_t *pflags;
    int32_t *persons_out, *n_persons_out;     // may be `persons` / `n_persons`: read before the first barrier or by the lane that writes
    uint8_t *change;
    int32_t *n_views;
    double *dist, *pair;
    int32_t *free_heads, *counts, *status, *sticky;
};

// joint j of row fp (f * pcap + p, a row with a pose) is present: asked for, flagged, finite; its coordinates widened
__device__ inline bool joint_of(const ConsolidateK &a, size_t fp, int j, double *X) {
    const size_t pj = fp * a.J + j;
    if (a.joint_flags && a.pflags[pj] == 0) return false;
    load3(a.poses, a.pose_f64, pj, X);
    return finite3(X[0], X[1], X[2]);
}

// the tracker's cost of rows p (in the role of a) and q, both with a pose: -1 when unscored
__device__ inline double pose_distance(const ConsolidateK &a, size_t fp, size_t fq) {
    const double inf = __builtin_huge_val();
    double sum = 0.0;
    int n = 0;
    for (int j = 0; j < a.J; ++j) {
        if (!((a.joint_mask >> j) & 1u)) continue;
        double A[3], B[3];
        if (!joint_of(a, fp, j, A) || !joint_of(a, fq, j, B)) continue;
        const double dx = A[0] - B[0], dy = A[1] - B[1], dz = A[2] - B[2];
        double s = dx * dx;
        s = s + dy * dy;
        s = s + dz * dz;
        sum = sum + sqrt(s);
        ++n;
    }
    if (n < a.min_joints) return -1.0;
    const double d = sum / (double)n;
    return d < inf ? d : -1.0;
}

// (c1, a1, b1) orders before (c0, a0, b0)
__device__ inline bool before(double c1, int a1, int b1, double c0, int a0, int b0) {
    return c1 < c0 || (c1 == c0 && (a1 < a0 || (a1 == a0 && b1 < b0)));
}

__global__ void __launch_bounds__(CS_THREADS) k_consolidate(const DevCfg *__restrict__ cfg, ConsolidateK a) {
    __shared__ int32_t s_row[MPE_REGROUP_MAX_PERSONS * MPE_MAX_CAMERAS];      // [pcap][V], as the rows stand now
    __shared__ uint32_t s_named[NAMED_WORDS];                                // bit h: a row names head h
    __shared__ uint32_t s_cams[MPE_REGROUP_MAX_PERSONS];                     // bit c: row p holds a head of camera c now
    __shared__ uint8_t s_pose[MPE_REGROUP_MAX_PERSONS];                      // person p has a pose
    __shared__ uint8_t s_gone[MPE_REGROUP_MAX_PERSONS];                      // row p was merged away
    __shared__ double s_ray[MPE_CONSOLIDATE_RAY_DOUBLES];                    // [K][J][3], the unit rays of the free heads
    __shared__ double s_o[MPE_MAX_CAMERAS][3];
    __shared__ int32_t s_free[MPE_CONSOLIDATE_MAX_FREE], s_fcam[MPE_CONSOLIDATE_MAX_FREE];
    __shared__ uint32_t s_fmask[MPE_CONSOLIDATE_MAX_FREE];                   // the joints of a free head that may vote
    __shared__ int32_t s_res[6];                                             // merged, founded, placed, K, rows now, rows full
    __shared__ int32_t s_bad;
    const int f = blockIdx.x, tid = threadIdx.x, V = a.V, pcap = a.pcap, J = a.J, fcap = a.fcap;
    // the rows of the frame (frame_rows.h).  The Selection is put together here from the flat argument fields: as a member of
    // ConsolidateK it cost this kernel 20 more spilled scalar registers and 6 % at 5x4
    const Selection sel{V, J, a.joint_flags, a.joint_mask, a.threshold, a.frame_head_off, a.head_joint_mask, a.vp, a.persons, a.n_persons, a.pflags};
    const FrameRows fr = frame_rows_load<CS_THREADS>(sel, pcap, a.hmax, f, s_row, s_pose, s_named, &s_bad);
    const int h0 = fr.h0, H = fr.H, np_raw = fr.np_raw, np = fr.np;
    const bool over = fr.over;
    const size_t fp0 = fr.fp0;
    const int entries = pcap * V;
    for (int p = tid; p < pcap; p += CS_THREADS) s_gone[p] = 0;
    if (tid < 6) s_res[tid] = tid == 4 ? np : 0;
    if (tid < V) camera_centre(cfg, tid, s_o[tid]);
    __syncthreads();

    frame_rows_mark<CS_THREADS>(fr, V, a.head_cam, s_row, s_named, &s_bad);
    __syncthreads();
    const bool copy = frame_rows_copy(fr, &s_bad);

    // the pose distances; the camera set of every row
    for (int i = tid; i < pcap * pcap; i += CS_THREADS) {
        const int p = i / pcap, q = i - p * pcap;
        double d = -1.0;
        if (!copy && p < q && q < np && s_pose[p] && s_pose[q]) d = pose_distance(a, fp0 + p, fp0 + q);
        a.dist[fp0 * pcap + i] = d;
    }
    for (int p = tid; p < pcap; p += CS_THREADS) {
        uint32_t m = 0;
        if (p < np)
            for (int c = 0; c < V; ++c) m |= s_row[p * V + c] >= 0 ? 1u << c : 0u;
        s_cams[p] = m;
    }
    // the free heads in head order: rank = the free heads before it
    if (!copy && tid < 64) {
        int K = 0;
        for (int base = 0; base < H; base += 64) {
            const int hh = base + tid;
            const bool is_free = hh < H && !((s_named[hh >> 5] >> (hh & 31)) & 1u);
            const unsigned long long b = __ballot(is_free);
            const int rank = K + __popcll(b & ((1ull << tid) - 1ull));
            if (is_free && rank < fcap) s_free[rank] = hh;
            K += __popcll(b);
        }
        if (tid == 0) s_res[3] = K;
    }
    __syncthreads();
    const int K = s_res[3];
    const bool free_over = K > fcap;
    const int Kc = copy || free_over ? 0 : K;                    // the free heads the founding pass works on

    // per free head the camera and the joints that may vote, per (head, joint) the unit ray
    if (tid < Kc) {
        const int h = h0 + s_free[tid], c = a.head_cam[h];
        uint32_t ok = (unsigned)c < (unsigned)V ? a.head_joint_mask[h] & a.joint_mask : 0u;
        const float *conf = a.vp + (size_t)h * J * 2;
        for (int j = 0; j < J; ++j)
            if (!(conf[2 * j] > a.threshold)) ok &= ~(1u << j);
        s_fcam[tid] = c;
        s_fmask[tid] = ok;
    }
    __syncthreads();
    for (int i = tid; i < Kc * J; i += CS_THREADS) {
        const int r = i / J, j = i - r * J;
        if (!((s_fmask[r] >> j) & 1u)) continue;
        const double *px = a.xy + ((size_t)(h0 + s_free[r]) * J + j) * 2;
        unit_ray(cfg, s_fcam[r], px[0], px[1], s_ray + ((size_t)r * J + j) * 3);
    }
    __syncthreads();

    // the pair costs of the free heads, by rank
    for (int i = tid; i < fcap * fcap; i += CS_THREADS) {
        const int x = i / fcap, y = i - x * fcap;
        double cost = -1.0;
        if (x < y && y < Kc && s_fcam[x] != s_fcam[y]) {
            const uint32_t votes = s_fmask[x] & s_fmask[y];
            const int c1 = s_fcam[x], c2 = s_fcam[y];
            double sum = 0.0;
            int n = 0;
            for (int j = 0; j < J; ++j) {
                if (!((votes >> j) & 1u)) continue;
                sum = sum + ray_distance(s_ray + ((size_t)x * J + j) * 3, s_ray + ((size_t)y * J + j) * 3, s_o[c1], s_o[c2], a.clip);
                ++n;
            }
            if (n >= a.min_joints) {
                const double mean = sum / (double)n;
                if (mean < __builtin_huge_val()) cost = mean;
            }
        }
        a.pair[(size_t)f * fcap * fcap + i] = cost;
    }
    for (int r = tid; r < fcap; r += CS_THREADS) a.free_heads[(size_t)f * fcap + r] = !copy && r < (K < fcap ? K : fcap) ? s_free[r] : -1;
    __syncthreads();                          // also: this workgroup's d_dist and d_pair stores are visible to it from here on

    // the merge pass
    if (!copy && (a.flags & MPE_CONSOLIDATE_MERGE) && tid < 64) {
        const double *tab = a.dist + fp0 * pcap;
        int merged = 0;
        for (;;) {
            double bc = __builtin_huge_val();
            int bp = CS_NONE, bq = CS_NONE;
            for (int i = tid; i < np * np; i += 64) {
                const int p = i / np, q = i - p * np;
                if (p >= q || s_gone[p] || s_gone[q] || (s_cams[p] & s_cams[q])) continue;
                const double x = tab[p * pcap + q];
                if (x >= 0.0 && x < a.merge_m && before(x, p, q, bc, bp, bq)) bc = x, bp = p, bq = q;
            }
            for (int off = 32; off; off >>= 1) {
                const double oc = __shfl_xor(bc, off);
                const int op = __shfl_xor(bp, off), oq = __shfl_xor(bq, off);
                if (before(oc, op, oq, bc, bp, bq)) bc = oc, bp = op, bq = oq;
            }
            if (bp == CS_NONE) break;         // the same in every lane: no mergeable pair is left
            if (tid < V) {
                const int e = s_row[bq * V + tid];
                if (e >= 0) s_row[bp * V + tid] = e, s_row[bq * V + tid] = -1;
            }
            if (tid == 0) {
                s_cams[bp] |= s_cams[bq];
                s_cams[bq] = 0;
                s_gone[bq] = 1;
            }
            ++merged;
            __threadfence_block();
        }
        if (tid == 0) s_res[0] = merged;
    }
    __syncthreads();

    // the found pass: seeds in increasing (cost, a, b), each grown by complete linkage; lane r is free head r
    if ((a.flags & MPE_CONSOLIDATE_FOUND) && Kc > 0 && tid < 64) {
        const double *tab = a.pair + (size_t)f * fcap * fcap;
        unsigned long long placed = 0;
        int n_now = np, founded = 0, n_placed = 0, full = 0;
        double cur_c = -1.0;                  // below every scored cost
        int cur_a = -1, cur_b = -1;
        const int my_cam = tid < Kc && (unsigned)s_fcam[tid] < (unsigned)V ? s_fcam[tid] : 0;      // (a head of no camera has no scored pair)
        for (;;) {
            double bc = __builtin_huge_val();
            int ba = CS_NONE, bb = CS_NONE;
            for (int i = tid; i < Kc * Kc; i += 64) {
                const int x = i / Kc, y = i - x * Kc;
                if (x >= y || ((placed >> x) & 1ull) || ((placed >> y) & 1ull)) continue;
                const double c = tab[x * fcap + y];
                if (c >= 0.0 && c < a.found_m && before(cur_c, cur_a, cur_b, c, x, y) && before(c, x, y, bc, ba, bb)) bc = c, ba = x, bb = y;
            }
            for (int off = 32; off; off >>= 1) {
                const double oc = __shfl_xor(bc, off);
                const int oa = __shfl_xor(ba, off), ob = __shfl_xor(bb, off);
                if (before(oc, oa, ob, bc, ba, bb)) bc = oc, ba = oa, bb = ob;
            }
            if (ba == CS_NONE) break;
            if (n_now == pcap) {
                full = 1;
                break;
            }
            cur_c = bc, cur_a = ba, cur_b = bb;
            unsigned long long members = (1ull << ba) | (1ull << bb);
            uint32_t cams = (1u << s_fcam[ba]) | (1u << s_fcam[bb]);
            for (;;) {
                double key = __builtin_huge_val();
                int who = CS_NONE;
                if (tid < Kc && !(((placed | members) >> tid) & 1ull) && !((cams >> my_cam) & 1u)) {
                    double worst = 0.0;
                    bool ok = true;
                    for (unsigned long long m = members; m && ok; m &= m - 1ull) {
                        const int r = __ffsll((long long)m) - 1;
                        const double c = r < tid ? tab[r * fcap + tid] : tab[tid * fcap + r];
                        ok = c >= 0.0 && c < a.found_m;
                        if (ok && c > worst) worst = c;
                    }
                    if (ok) key = worst, who = tid;
                }
                for (int off = 32; off; off >>= 1) {
                    const double ok_ = __shfl_xor(key, off);
                    const int ow = __shfl_xor(who, off);
                    if (ow != CS_NONE && (who == CS_NONE || ok_ < key || (ok_ == key && ow < who))) key = ok_, who = ow;
                }
                if (who == CS_NONE) break;
                members |= 1ull << who;
                cams |= 1u << s_fcam[who];
            }
            const int size = __popcll(members);
            if (size < a.found_min_views) continue;                  // dissolved: the heads stay free, the cursor has moved on
            if (tid < V) s_row[n_now * V + tid] = -1;
            __threadfence_block();
            if ((members >> tid) & 1ull) s_row[n_now * V + my_cam] = s_free[tid];
            __threadfence_block();
            placed |= members;
            ++n_now, ++founded, n_placed += size;
        }
        if (tid == 0) s_res[1] = founded, s_res[2] = n_placed, s_res[4] = n_now, s_res[5] = full;
    }
    __syncthreads();

    const int n_now = s_res[4];
    for (int i = tid; i < entries; i += CS_THREADS) {
        const int was = a.persons[fp0 * V + i], now = s_row[i];
        int code = 0;
        if (now != was) code = (was >= 0 ? 1 : 0) | (now >= 0 ? 2 : 0);
        a.persons_out[fp0 * V + i] = now;
        a.change[fp0 * V + i] = (uint8_t)code;
    }
    for (int p = tid; p < pcap; p += CS_THREADS) {
        int nv = 0;
        if (p < n_now)
            for (int c = 0; c < V; ++c) nv += s_row[p * V + c] >= 0;
        a.n_views[fp0 + p] = nv;
    }
    if (tid < 4) a.counts[(size_t)f * 4 + tid] = copy ? 0 : tid < 3 ? s_res[tid] : s_res[3] - s_res[2];
    if (tid == 0) {
        a.status[f] = over ? MPE_CONSOLIDATE_OVER_CAP
                           : s_bad ? MPE_CONSOLIDATE_BAD_ROWS : (free_over ? MPE_CONSOLIDATE_FREE_OVER_CAP : 0) | (s_res[5] ? MPE_CONSOLIDATE_ROWS_FULL : 0);
        a.n_persons_out[f] = copy ? np_raw : n_now;
        if (over && a.sticky) atomicOr(a.sticky, 1);
    }
}

}  // namespace

hipError_t launch_consolidate(hipStream_t s, const DevCfg *cfg, int V, int hmax, int32_t *sticky, const mpe_batch &b,
                              const mpe_consolidate_args &x) {
    ConsolidateK a{x.pcap, V, x.n_joints, x.pose_f64, x.joint_flags, x.min_joints, x.found_min_views, x.fcap, hmax, x.joint_mask, x.flags,
                   x.threshold, x.merge_m, x.found_m, x.clip_m, b.d_frame_head_off, b.d_head_cam, b.d_joint_mask, b.d_vp, b.d_xy, x.d_persons,
                   x.d_n_persons, x.d_poses, x.d_flags, x.d_persons_out, x.d_n_persons_out, x.d_change, x.d_n_views, x.d_dist, x.d_pair,
                   x.d_free, x.d_counts, x.d_status, sticky};
    hipLaunchKernelGGL(k_consolidate, dim3((unsigned)x.n_frames), dim3(CS_THREADS), 0, s, cfg, a);
    return hipGetLastError();
}

}  // namespace mpe
