// Relink: a newborn track takes the id of a lost track with the same bone lengths (include/mpe.h: mpe_relink_*; the numpy
// statement is harness/relink.py).  Two kernels per call whatever the frame count and whatever the data:
//
// k_relink_rows    one thread per (frame, row, bone): reads the pose rows once through PoseRows and writes, per row, the
//                  id (-1: no detection), the active-joint mask and the accepted bone lengths in f64 (0.0: none).  All the
//                  arithmetic and all the traffic that scale with the batch are here.
// k_relink_walk    ONE workgroup of RLT threads walks the frames of the call in order.  canon, last_frame and the presence
//                  stamps of the tid_cap ids sit in LDS for the whole call.  Per frame: the rows mark their records
//                  present; when the frame has a birth (a workgroup-wide OR, so the common frame pays nothing more) the
//                  threads fill births x tid_cap costs into the state's table and the greedy takes the least of them, ties
//                  to the lowest (row, column), at most once per birth; then the first row of every canonical id adds its
//                  lengths to its record, one thread per (row, bone) -- different rows, different records, no atomics, and
//                  a record's sum is a left fold in frame order.  Every barrier sits in code the whole workgroup runs: the
//                  conditions around them are read from LDS after a barrier or come from __syncthreads_or.  Every loop is
//                  bounded by n_frames, pcap, tid_cap, n_bones or J.
#include "mpe_internal.h"
#include "pose_rows.h"

#pragma clang fp contract(off)

namespace mpe {

namespace {

constexpr int RLT = 256;                                     // threads of the walker
constexpr int RLP = MPE_TRACK_MAX_PERSONS;                   // rows per frame, at most

struct RelinkK {
    PoseRows r;
    int n_bones, tid_cap, min_gap, max_gap, min_samples, min_bones, frame0;
    uint32_t jmask, umask;
    double gate, max_bone, reach, speed;
    const int32_t *bones;
    double *row_len;                 // scratch [n_frames * pcap][n_bones]: accepted lengths, 0.0: none
    uint32_t *row_act;               // scratch [n_frames * pcap]: active joints
    int32_t *row_id;                 // scratch [n_frames * pcap]: the id of a detection, -1: none
    double *table;                   // scratch [pcap][tid_cap]: the costs of a frame's births
    int32_t *canon, *last_frame, *seen;
    double *last_pose;
    uint32_t *last_mask;
    double *sum;
    int32_t *cnt;
    unsigned long long *ctr;         // births, linked, over_ids, status
    int32_t *ids_out;
    double *cost_out;
    int32_t *gap_out;
};

enum { RL_NONE = 0, RL_OVER = 1, RL_KNOWN = 2, RL_BIRTH = 3, RL_REPEAT = 4 };

template <typename T>
__global__ void __launch_bounds__(256) k_relink_rows(RelinkK a) {
    const size_t i = (size_t)blockIdx.x * 256 + threadIdx.x;
    const size_t total = (size_t)a.r.n_frames * a.r.pcap * a.n_bones;
    if (i >= total) return;
    const size_t fp = i / a.n_bones;
    const int b = (int)(i - fp * a.n_bones);
    const size_t f = fp / a.r.pcap;
    const int p = (int)(fp - f * a.r.pcap);
    int32_t t = -1;
    if (p < rows_in_frame(a.r, (int)f)) {
        t = a.r.tid[fp];
        if (t < 0 || (!a.r.joint_flags && !a.r.flags[fp])) t = -1;
    }
    const T *x = static_cast<const T *>(a.r.poses) + fp * a.r.J * 3;
    const uint32_t on = t >= 0 ? flag_mask(a.r, fp) & a.jmask : 0u;
    double l = 0.0;
    const int jp = a.bones[2 * b], jc = a.bones[2 * b + 1];
    if ((on >> jp) & (on >> jc) & 1u) {
        const double px = (double)x[3 * jp], py = (double)x[3 * jp + 1], pz = (double)x[3 * jp + 2];
        const double cx = (double)x[3 * jc], cy = (double)x[3 * jc + 1], cz = (double)x[3 * jc + 2];
        if (finite3(px, py, pz) && finite3(cx, cy, cz)) {
            const double dx = cx - px, dy = cy - py, dz = cz - pz;
            const double s = (dx * dx + dy * dy) + dz * dz;
            const double v = sqrt(s);
            if (v > 0.0 && v <= a.max_bone) l = v;
        }
    }
    a.row_len[i] = l;
    if (b == 0) {
        uint32_t act = 0;
        for (int j = 0; j < a.r.J; ++j)
            if (((on >> j) & 1u) && finite3((double)x[3 * j], (double)x[3 * j + 1], (double)x[3 * j + 2])) act |= 1u << j;
        a.row_act[fp] = act;
        a.row_id[fp] = t;
    }
}

// steps 4 to 6 of the statement for the birth in row fp against record c seen g frames ago -> the cost of a linkable
// pair, +inf for any other
template <typename T>
__device__ inline double relink_pair(const RelinkK &a, size_t fp, int c, int g) {
    const double inf = __builtin_inf();
    const double *lb = a.row_len + fp * a.n_bones;
    const double *rs = a.sum + (size_t)c * a.n_bones;
    const int32_t *rc = a.cnt + (size_t)c * a.n_bones;
    double tot = 0.0;
    int n = 0;
    for (int b = 0; b < a.n_bones; ++b) {
        const double l = lb[b];
        const int32_t k = rc[b];
        if (l > 0.0 && k >= a.min_samples) {
            const double m = rs[b] / (double)k;
            tot = tot + fabs(l - m);
            ++n;
        }
    }
    if (n < a.min_bones) return inf;
    const double v = tot / (double)n;
    if (!(v < a.gate)) return inf;
    if (a.reach > 0.0) {
        const uint32_t both = a.row_act[fp] & a.last_mask[c] & a.umask;
        const T *x = static_cast<const T *>(a.r.poses) + fp * a.r.J * 3;
        const double *y = a.last_pose + (size_t)c * a.r.J * 3;
        double dt = 0.0;
        int k = 0;
        for (int j = 0; j < a.r.J; ++j) {
            if (!((both >> j) & 1u)) continue;
            const double dx = (double)x[3 * j] - y[3 * j], dy = (double)x[3 * j + 1] - y[3 * j + 1], dz = (double)x[3 * j + 2] - y[3 * j + 2];
            double s = dx * dx;
            s = s + dy * dy;
            s = s + dz * dz;
            dt = dt + sqrt(s);
            ++k;
        }
        if (k == 0) return inf;
        const double d = dt / (double)k;
        const double lim = a.reach + a.speed * (double)g;
        if (!(d < lim)) return inf;
    }
    return v;
}

template <typename T>
__global__ void __launch_bounds__(RLT) k_relink_walk(RelinkK a) {
    extern __shared__ int32_t s_ids[];                       // canon, last_frame, seen: [tid_cap] each
    __shared__ int32_t s_t[RLP], s_upd[RLP], s_gap[RLP], s_brow[RLP];
    __shared__ double s_cost[RLP];
    __shared__ int s_wn[2];
    __shared__ double s_rv[RLT / 64];
    __shared__ uint32_t s_rk[RLT / 64];
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const int cap = a.tid_cap, pcap = a.r.pcap, nb = a.n_bones, J = a.r.J;
    int32_t *s_canon = s_ids, *s_last = s_ids + cap, *s_seen = s_ids + 2 * cap;
    const double inf = __builtin_inf();
    for (int c = tid; c < cap; c += RLT) {
        s_canon[c] = a.canon[c];
        s_last[c] = a.last_frame[c];
        s_seen[c] = a.seen[c];
    }
    unsigned long long n_births = 0, n_linked = 0, n_over = 0;   // thread 0 links; the rows' threads count their own
    // the id of this thread's row in the next frame is fetched while the current frame waits for its stores anyway
    int32_t t_next = tid < pcap && a.r.n_frames > 0 ? a.row_id[tid] : -1;
    __syncthreads();

    for (int fl = 0; fl < a.r.n_frames; ++fl) {
        const int f = a.frame0 + fl;
        const size_t fp0 = (size_t)fl * pcap;
        // the rows: what each is, and the records that are present
        int kind = RL_NONE;
        int32_t t = -1;
        if (tid < pcap) {
            t = t_next;
            if (t >= cap) {
                kind = RL_OVER;
                ++n_over;
            } else if (t >= 0) {
                const int32_t c = s_canon[t];
                kind = c >= 0 ? RL_KNOWN : RL_BIRTH;
                if (c >= 0) s_seen[c] = f;                   // several rows may: the same value
            }
            s_t[tid] = t;
            s_cost[tid] = -1.0;
            s_gap[tid] = kind == RL_NONE ? -1 : 0;
        }
        if (__syncthreads_or(kind == RL_BIRTH)) {
            // a later row that repeats a birth's id is no birth; the births in row order
            if (kind == RL_BIRTH)
                for (int q = 0; q < tid; ++q)
                    if (s_t[q] == t) kind = RL_REPEAT;
            const unsigned long long bal = __ballot(kind == RL_BIRTH);
            if (wave < 2 && lane == 0) s_wn[wave] = __popcll(bal);
            __syncthreads();
            const int n_rows = s_wn[0] + s_wn[1];
            if (kind == RL_BIRTH) s_brow[(wave ? s_wn[0] : 0) + __popcll(bal & ((1ull << lane) - 1ull))] = tid;
            __syncthreads();
            const int total = n_rows * cap;                  // <= 128 * 4096
            for (int i = tid; i < total; i += RLT) {
                const int r = i / cap, c = i - r * cap;
                double v = inf;
                const int32_t lf = s_last[c];
                if (lf >= 0 && s_seen[c] != f) {
                    const int g = f - lf;
                    if (g >= a.min_gap && g <= a.max_gap) v = relink_pair<T>(a, fp0 + s_brow[r], c, g);
                }
                a.table[i] = v;
            }
            __syncthreads();
            for (int it = 0; it < n_rows; ++it) {
                double best = inf;
                uint32_t key = 0xFFFFFFFFu;
                for (int i = tid; i < total; i += RLT) {     // i = row * cap + column: the first of equals is the lowest (row, column)
                    const double v = a.table[i];
                    if (v < best) {
                        best = v;
                        key = (uint32_t)i;
                    }
                }
                for (int off = 32; off; off >>= 1) {
                    const double ov = __shfl_xor(best, off);
                    const uint32_t ok = __shfl_xor(key, off);
                    if (ov < best || (ov == best && ok < key)) {
                        best = ov;
                        key = ok;
                    }
                }
                if (lane == 0) {
                    s_rv[wave] = best;
                    s_rk[wave] = key;
                }
                __syncthreads();
                best = s_rv[0];
                key = s_rk[0];
                for (int w = 1; w < RLT / 64; ++w)
                    if (s_rv[w] < best || (s_rv[w] == best && s_rk[w] < key)) {
                        best = s_rv[w];
                        key = s_rk[w];
                    }
                if (!(best < inf)) break;                    // the same for every thread: read from LDS after the barrier
                const int r = (int)key / cap, c = (int)key - r * cap;
                if (tid == 0) {
                    const int p = s_brow[r];
                    s_canon[s_t[p]] = c;
                    s_cost[p] = best;
                    s_gap[p] = f - s_last[c];
                    ++n_linked;
                }
                for (int i = tid; i < cap; i += RLT) a.table[(size_t)r * cap + i] = inf;
                for (int i = tid; i < n_rows; i += RLT) a.table[(size_t)i * cap + c] = inf;
                __syncthreads();
            }
            __syncthreads();                                 // the break leaves before the loop's last barrier
            if (kind == RL_BIRTH && s_canon[t] < 0) {
                s_canon[t] = t;
                ++n_births;
            }
            __syncthreads();
        }
        // the ids, and the first row of every canonical id
        int32_t out = t;
        if (tid < pcap) {
            int32_t c = -1;
            if (kind >= RL_KNOWN) {
                out = c = s_canon[t];
                for (int q = 0; q < tid; ++q) {
                    const int32_t tq = s_t[q];
                    if (tq >= 0 && tq < cap && s_canon[tq] == out) c = -1;
                }
            }
            s_upd[tid] = c;
        }
        __syncthreads();
        // the outputs go with the records' stores: one wait at the closing barrier for all of them
        if (tid < pcap) {
            if (fl + 1 < a.r.n_frames) t_next = a.row_id[fp0 + pcap + tid];
            a.ids_out[fp0 + tid] = out;
            a.cost_out[fp0 + tid] = s_cost[tid];
            a.gap_out[fp0 + tid] = s_gap[tid];
        }
        for (int i = tid; i < pcap * nb; i += RLT) {
            const int p = i / nb, b = i - p * nb;
            const int32_t c = s_upd[p];
            if (c < 0) continue;
            const double l = a.row_len[(fp0 + p) * nb + b];
            if (l > 0.0) {
                a.sum[(size_t)c * nb + b] = a.sum[(size_t)c * nb + b] + l;
                a.cnt[(size_t)c * nb + b] += 1;
            }
        }
        for (int i = tid; i < pcap * J; i += RLT) {
            const int p = i / J, j = i - p * J;
            const int32_t c = s_upd[p];
            if (c < 0) continue;
            const T *x = static_cast<const T *>(a.r.poses) + ((fp0 + p) * J + j) * 3;
            double *y = a.last_pose + ((size_t)c * J + j) * 3;
            const bool on = (a.row_act[fp0 + p] >> j) & 1u;
            y[0] = on ? (double)x[0] : 0.0;
            y[1] = on ? (double)x[1] : 0.0;
            y[2] = on ? (double)x[2] : 0.0;
        }
        if (tid < pcap && s_upd[tid] >= 0) {
            a.last_mask[s_upd[tid]] = a.row_act[fp0 + tid];
            s_last[s_upd[tid]] = f;
        }
        __syncthreads();
    }

    for (int c = tid; c < cap; c += RLT) {
        a.canon[c] = s_canon[c];
        a.last_frame[c] = s_last[c];
        a.seen[c] = s_seen[c];
    }
    if (n_births) atomicAdd(&a.ctr[0], n_births);
    if (n_linked) atomicAdd(&a.ctr[1], n_linked);
    if (n_over) {
        atomicAdd(&a.ctr[2], n_over);
        atomicOr(&a.ctr[3], (unsigned long long)MPE_RELINK_OVER_IDS);
    }
}

size_t walk_lds_bytes(int tid_cap) { return (size_t)3 * tid_cap * sizeof(int32_t); }

}  // namespace

hipError_t launch_relink_reset(hipStream_t s, mpe_relink_state *st) {
    const size_t cap = (size_t)st->tid_cap;
    hipError_t e = hipMemsetAsync(st->canon, 0xFF, 3 * cap * sizeof(int32_t), s);      // canon, last_frame, seen: -1
    if (e == hipSuccess) e = hipMemsetAsync(st->last_pose, 0, cap * st->J * 3 * sizeof(double), s);
    if (e == hipSuccess) e = hipMemsetAsync(st->last_mask, 0, cap * sizeof(uint32_t), s);
    if (e == hipSuccess) e = hipMemsetAsync(st->sum, 0, cap * st->n_bones * sizeof(double), s);
    if (e == hipSuccess) e = hipMemsetAsync(st->cnt, 0, cap * st->n_bones * sizeof(int32_t), s);
    if (e == hipSuccess) e = hipMemsetAsync(st->ctr, 0, 4 * sizeof(unsigned long long), s);
    if (e == hipSuccess) st->frame = 0;
    return e;
}

hipError_t launch_relink(hipStream_t s, mpe_relink_state *st, const mpe_relink_args &x) {
    RelinkK a{};
    a.r.n_frames = x.n_frames; a.r.pcap = st->pcap; a.r.J = st->J; a.r.pose_f64 = st->pose_f64; a.r.joint_flags = x.joint_flags;
    a.r.poses = x.d_poses; a.r.flags = x.d_flags; a.r.n_persons = x.d_n_persons; a.r.tid = x.d_track_id;
    a.n_bones = st->n_bones; a.tid_cap = st->tid_cap;
    a.min_gap = st->cfg.min_gap; a.max_gap = st->cfg.max_gap; a.min_samples = st->cfg.min_samples; a.min_bones = st->cfg.min_bones;
    a.frame0 = (int)st->frame;
    a.jmask = st->cfg.joint_mask & joint_bits(st->J);
    a.umask = st->cfg.used_joint_mask & joint_bits(st->J);
    a.gate = st->cfg.gate_m; a.max_bone = st->cfg.max_bone_m; a.reach = st->cfg.reach_m; a.speed = st->cfg.reach_per_frame_m;
    a.bones = st->bones;
    a.row_len = st->row_len; a.row_act = st->row_act; a.row_id = st->row_id; a.table = st->table;
    a.canon = st->canon; a.last_frame = st->canon + st->tid_cap; a.seen = st->canon + 2 * (size_t)st->tid_cap;
    a.last_pose = st->last_pose; a.last_mask = st->last_mask; a.sum = st->sum; a.cnt = st->cnt; a.ctr = st->ctr;
    a.ids_out = x.d_ids; a.cost_out = x.d_link_cost; a.gap_out = x.d_link_gap;
    const size_t total = (size_t)x.n_frames * st->pcap * st->n_bones;          // <= max_frames * 128 * 32, checked at create
    const dim3 grid((unsigned)((total + 255) / 256));
    if (st->pose_f64) hipLaunchKernelGGL(k_relink_rows<double>, grid, dim3(256), 0, s, a);
    else hipLaunchKernelGGL(k_relink_rows<float>, grid, dim3(256), 0, s, a);
    hipError_t e = hipGetLastError();
    if (e != hipSuccess) return e;
    ++st->launches;
    const size_t lds = walk_lds_bytes(st->tid_cap);          // <= 48 KiB: within what a kernel has without asking
    if (st->pose_f64) hipLaunchKernelGGL(k_relink_walk<double>, dim3(1), dim3(RLT), lds, s, a);
    else hipLaunchKernelGGL(k_relink_walk<float>, dim3(1), dim3(RLT), lds, s, a);
    e = hipGetLastError();
    if (e != hipSuccess) return e;
    ++st->launches;
    st->frame += x.n_frames;
    return hipSuccess;
}

}  // namespace mpe
