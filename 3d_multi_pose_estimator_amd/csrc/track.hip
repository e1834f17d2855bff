// Tracking: person identities carried from frame to frame of a batch (include/mpe.h: mpe_track_batch; the numpy
// statement is harness/tracking.py).  The history kept in the state stands in front of the batch as the virtual frames
// 0 .. H-1 (H = max_gap + 1), batch frame f is virtual frame H + f; everything is addressed by person row, and
// "detection order" is row order among the rows that are detections.
//
// While a call runs, the outputs are the working storage (nothing is allocated, nothing sized by n_frames is kept):
//   d_link_gap    -1 not a detection, 0 no parent yet, g > 0 linked at stage g
//   d_track_id    -1 not a detection; else bits 0-6 the parent's row in virtual frame v - g, bit 8 "has a child"
//                 (both set with atomic ORs: frame t writes its rows' parents while frame t + g marks the same rows)
// k_track_init    fills them; k_track_stage (once per g, one workgroup per frame) builds the table of linkable costs
//                 of the frame's parentless rows against the childless rows of frame v - g in LDS and lets wave 0 pick
//                 pairs greedily: a wave-wide arg-min over (cost, row, column) of the rows' best columns.
//                 A link into a history frame sets that row's child mark in the history copy the call READS (o_child, the
//                 one field of the old copy that is written): k_track_carry, which runs after the last stage, takes
//                 the marks over from there.
// k_track_carry   writes the next history (rows, poses widened to f64, joint masks, child marks; ids of rows that come
//                 from the old history) into the other half of the state.
// k_track_births  (count per block of frames, then scan and number) gives every parentless detection its id in frame,
//                 then row order, and advances the counter.
// k_track_resolve turns the links of a segment of frames into ids or into pointers that leave the segment (pointer
//                 jumping in LDS, a pointer is -2 - (virtual frame * 128 + row)); k_track_finish follows what is left
//                 from segment to segment (a value read there is final or a pointer further back: either serves) and
//                 hands the ids of the last H frames to the next history.
#include "mpe_internal.h"
#include "pose_rows.h"

#pragma clang fp contract(off)

namespace mpe {

namespace {

constexpr int TRK_PCAP = MPE_TRACK_MAX_PERSONS;      // 128: parent rows take 7 bits, the row lists two waves
constexpr int TRK_CHILD = 0x100;
constexpr int TRK_ROW = 0x7f;
constexpr int TRK_SEG_WORDS = 8192;                  // rows of one k_track_resolve segment (32 KB of LDS)

struct TrackK : PoseRows {           // PoseRows::tid stays null: the ids are this stage's output
    int H;
    uint32_t used;                   // used_joint_mask, cut to the J joints
    double gate;
    int32_t *ids;                    // d_track_id, the working storage described above
    double *cost;
    int32_t *gap;
    int32_t *issued_out;
    // the state: the history read (o_; its child marks are also set, see above) and the one written (n_), [H][pcap] each
    const double *o_pose;
    const uint32_t *o_mask;
    const int32_t *o_id;
    uint8_t *o_child;
    const int32_t *o_count;
    double *n_pose;
    uint32_t *n_mask;
    int32_t *n_id;
    uint8_t *n_child;
    int32_t *n_count;
    int32_t *ws;                     // [TRK_BIRTH_BLOCKS] births per block of frames
    int fpt, seg;                    // frames per thread of the birth pass; frames per segment of k_track_resolve
};

constexpr int TRK_BIRTH_BLOCKS = 1024;

// used joints present in row p of batch frame f; 0: not a detection
__device__ inline uint32_t row_mask(const TrackK &a, int f, int p) {
    if (p >= rows_in_frame(a, f)) return 0u;
    return flag_mask(a, (size_t)f * a.pcap + p) & a.used;
}

template <typename TA, typename TB>
__device__ double pair_cost(const TA *pa, const TB *pb, uint32_t m, int J) {
    if (!m) return INFINITY;
    double tot = 0.0;
    int n = 0;
    for (int j = 0; j < J; ++j) {
        if (!((m >> j) & 1u)) continue;
        const double dx = (double)pa[3 * j] - (double)pb[3 * j];
        const double dy = (double)pa[3 * j + 1] - (double)pb[3 * j + 1];
        const double dz = (double)pa[3 * j + 2] - (double)pb[3 * j + 2];
        double s = dx * dx;
        s = s + dy * dy;
        s = s + dz * dz;
        tot = tot + sqrt(s);
        ++n;
    }
    return tot / (double)n;
}

__global__ void __launch_bounds__(256) k_track_init(TrackK a) {
    const int i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= a.n_frames * a.pcap) return;
    const int f = i / a.pcap, p = i - f * a.pcap;
    const bool det = row_mask(a, f, p) != 0;
    a.ids[i] = det ? 0 : -1;
    a.gap[i] = det ? 0 : -1;
    a.cost[i] = -1.0;
}

// position of a set flag among the set flags of threads 0 .. 127 (row order), and their number
__device__ inline int compact_rows(bool on, int32_t *s_cnt, int *total) {
    const unsigned long long b = __ballot(on);
    const int lane = threadIdx.x & 63, w = threadIdx.x >> 6;
    if (lane == 0) s_cnt[w] = __popcll(b);
    __syncthreads();
    int before = 0;
    for (int k = 0; k < w; ++k) before += s_cnt[k];
    *total = s_cnt[0] + s_cnt[1];
    const int at = before + __popcll(b & ((1ull << lane) - 1ull));
    __syncthreads();
    return at;
}

template <typename T>
__global__ void __launch_bounds__(256) k_track_stage(TrackK a, int g) {
    extern __shared__ double s_t[];                      // [R][C] cost where linkable, +inf otherwise
    __shared__ uint32_t s_rmask[TRK_PCAP], s_cmask[TRK_PCAP];
    __shared__ int32_t s_rows[TRK_PCAP], s_cols[TRK_PCAP], s_cnt[4];
    const int f = blockIdx.x, tx = threadIdx.x;
    const int v = a.H + f, u = v - g;                    // u >= 0: g <= H
    const bool hist = u < a.H;
    uint32_t rm = 0, cm = 0;
    if (tx < a.pcap) {
        if (a.gap[(size_t)f * a.pcap + tx] == 0) rm = row_mask(a, f, tx);
        if (hist) {
            const size_t o = (size_t)u * a.pcap + tx;
            if (!a.o_child[o]) cm = a.o_mask[o];
        } else {
            const int32_t w = a.ids[(size_t)(u - a.H) * a.pcap + tx];
            if (w >= 0 && !(w & TRK_CHILD)) cm = row_mask(a, u - a.H, tx);
        }
    }
    int R, C;
    const int ri = compact_rows(rm != 0, s_cnt, &R);
    const int ci = compact_rows(cm != 0, s_cnt, &C);
    if (rm) { s_rows[ri] = tx; s_rmask[ri] = rm; }
    if (cm) { s_cols[ci] = tx; s_cmask[ci] = cm; }
    __syncthreads();
    if (R == 0 || C == 0) return;                        // the whole workgroup: R and C are the same in every thread
    const T *pa = static_cast<const T *>(a.poses) + (size_t)f * a.pcap * a.J * 3;
    for (int i = tx; i < R * C; i += 256) {
        const int r = i / C, c = i - r * C;
        const uint32_t m = s_rmask[r] & s_cmask[c];
        const T *ra = pa + (size_t)s_rows[r] * a.J * 3;
        const double d = hist ? pair_cost(ra, a.o_pose + ((size_t)u * a.pcap + s_cols[c]) * a.J * 3, m, a.J)
                              : pair_cost(ra, static_cast<const T *>(a.poses) + ((size_t)(u - a.H) * a.pcap + s_cols[c]) * a.J * 3, m, a.J);
        s_t[i] = d < a.gate ? d : INFINITY;              // a NaN never links
    }
    __syncthreads();                                     // the last barrier: waves 1-3 are done
    if (tx >= 64) return;

    // lane l keeps the best remaining column of rows l and l + 64
    unsigned long long taken[2] = {0ull, 0ull};
    double bc[2];
    int bi[2];
    auto scan = [&](int r, double *best, int *col) {
        double m = INFINITY;
        int at = -1;
        for (int c = 0; c < C; ++c) {
            if ((taken[c >> 6] >> (c & 63)) & 1ull) continue;
            const double d = s_t[r * C + c];
            if (d < m) { m = d; at = c; }
        }
        *best = m;
        *col = at;
    };
    for (int k = 0; k < 2; ++k) {
        bc[k] = INFINITY;
        bi[k] = -1;
        if (tx + 64 * k < R) scan(tx + 64 * k, &bc[k], &bi[k]);
    }
    while (true) {
        const int k0 = bc[1] < bc[0] ? 1 : 0;            // a tie stays with the lower row
        double m = bc[k0];
        int r = tx + 64 * k0, c = bi[k0];
        for (int off = 32; off; off >>= 1) {
            const double om = __shfl_xor(m, off);
            const int orow = __shfl_xor(r, off), oc = __shfl_xor(c, off);
            if (om < m || (om == m && orow < r)) { m = om; r = orow; c = oc; }
        }
        if (!(m < INFINITY)) break;
        taken[c >> 6] |= 1ull << (c & 63);
        if ((r & 63) == tx) {
            const int k = r >> 6, p = s_rows[r], q = s_cols[c];
            const size_t o = (size_t)f * a.pcap + p;
            a.gap[o] = g;
            a.cost[o] = m;
            atomicOr(&a.ids[o], q);
            if (hist) a.o_child[(size_t)u * a.pcap + q] = 1;
            else atomicOr(&a.ids[(size_t)(u - a.H) * a.pcap + q], TRK_CHILD);
            bc[k] = INFINITY;
            bi[k] = -1;
        }
        for (int k = 0; k < 2; ++k)
            if (bi[k] == c) scan(tx + 64 * k, &bc[k], &bi[k]);
    }
}

// next history slot k = virtual frame n_frames + k of this call
__global__ void __launch_bounds__(256) k_track_carry(TrackK a) {
    const int k = blockIdx.x, vf = a.n_frames + k, JJ = a.J * 3;
    for (int p = threadIdx.x; p < a.pcap; p += blockDim.x) {
        const size_t n = (size_t)k * a.pcap + p;
        if (vf < a.H) {
            const size_t o = (size_t)vf * a.pcap + p;
            a.n_mask[n] = a.o_mask[o];
            a.n_child[n] = a.o_child[o];
            a.n_id[n] = a.o_id[o];
        } else {
            const int32_t w = a.ids[(size_t)(vf - a.H) * a.pcap + p];
            a.n_mask[n] = row_mask(a, vf - a.H, p);
            a.n_child[n] = w >= 0 && (w & TRK_CHILD) ? 1 : 0;
            a.n_id[n] = -1;                              // detections: k_track_finish
        }
    }
    for (int i = threadIdx.x; i < a.pcap * JJ; i += blockDim.x) {
        const size_t n = (size_t)k * a.pcap * JJ + i;
        if (vf < a.H) a.n_pose[n] = a.o_pose[(size_t)vf * a.pcap * JJ + i];
        else if (a.pose_f64) a.n_pose[n] = static_cast<const double *>(a.poses)[(size_t)(vf - a.H) * a.pcap * JJ + i];
        else a.n_pose[n] = (double)static_cast<const float *>(a.poses)[(size_t)(vf - a.H) * a.pcap * JJ + i];
    }
}

// inclusive sum over the 256 threads of a workgroup
__device__ inline int block_scan(int x, int32_t *s) {
    s[threadIdx.x] = x;
    __syncthreads();
    for (int off = 1; off < 256; off <<= 1) {
        const int y = threadIdx.x >= off ? s[threadIdx.x - off] : 0;
        __syncthreads();
        s[threadIdx.x] += y;
        __syncthreads();
    }
    return s[threadIdx.x];
}

__device__ inline int births_of(const TrackK &a, int f0, int f1) {
    int n = 0;
    for (size_t i = (size_t)f0 * a.pcap; i < (size_t)f1 * a.pcap; ++i) n += a.gap[i] == 0;
    return n;
}

// thread t of block b owns frames [(b * 256 + t) * fpt, + fpt)
__global__ void __launch_bounds__(256) k_track_birth_count(TrackK a) {
    __shared__ int32_t s[256];
    const long long first = ((long long)blockIdx.x * 256 + threadIdx.x) * a.fpt;
    const int f0 = (int)min(first, (long long)a.n_frames), f1 = (int)min(first + a.fpt, (long long)a.n_frames);
    const int tot = block_scan(births_of(a, f0, f1), s);
    if (threadIdx.x == 255) a.ws[blockIdx.x] = tot;
}

__global__ void __launch_bounds__(256) k_track_birth_number(TrackK a) {
    __shared__ int32_t s[256];
    __shared__ int32_t s_base;
    int part = 0;
    for (int b = threadIdx.x; b < (int)blockIdx.x; b += 256) part += a.ws[b];
    const int before_blocks = block_scan(part, s);
    if (threadIdx.x == 255) s_base = *a.o_count + before_blocks;
    __syncthreads();                                     // also: s is free again
    const long long first = ((long long)blockIdx.x * 256 + threadIdx.x) * a.fpt;
    const int f0 = (int)min(first, (long long)a.n_frames), f1 = (int)min(first + a.fpt, (long long)a.n_frames);
    const int mine = births_of(a, f0, f1);
    const int incl = block_scan(mine, s);
    int id = s_base + incl - mine;
    for (size_t i = (size_t)f0 * a.pcap; i < (size_t)f1 * a.pcap; ++i)
        if (a.gap[i] == 0) a.ids[i] = id++;
    if (blockIdx.x == gridDim.x - 1 && threadIdx.x == 255) {
        *a.n_count = s_base + incl;
        *a.issued_out = s_base + incl;
    }
}

__global__ void __launch_bounds__(256) k_track_resolve(TrackK a) {
    __shared__ int32_t s_v[TRK_SEG_WORDS];
    const int f0 = blockIdx.x * a.seg, nf = min(a.seg, a.n_frames - f0), n = nf * a.pcap;
    const int v0 = a.H + f0;
    for (int i = threadIdx.x; i < n; i += 256) {
        const size_t o = (size_t)f0 * a.pcap + i;
        const int g = a.gap[o], w = a.ids[o];
        s_v[i] = g > 0 ? -2 - ((v0 + i / a.pcap - g) * TRK_PCAP + (w & TRK_ROW)) : w;
    }
    __syncthreads();
    while (true) {
        int moved = 0;
        for (int i = threadIdx.x; i < n; i += 256) {
            const int w = s_v[i];
            if (w >= -1) continue;
            const int t = -2 - w, vf = t / TRK_PCAP;
            if (vf < v0) continue;                       // leaves the segment
            s_v[i] = s_v[(vf - v0) * a.pcap + (t & TRK_ROW)];      // the value there is final or a pointer further back
            moved = 1;
        }
        if (!__syncthreads_or(moved)) break;
    }
    for (int i = threadIdx.x; i < n; i += 256) a.ids[(size_t)f0 * a.pcap + i] = s_v[i];
}

__global__ void __launch_bounds__(256) k_track_finish(TrackK a) {
    const int i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= a.n_frames * a.pcap) return;
    int w = a.ids[i];
    if (w < -1) {
        while (w < -1) {
            const int t = -2 - w, vf = t / TRK_PCAP, row = t & TRK_ROW;
            w = vf < a.H ? a.o_id[(size_t)vf * a.pcap + row]
                         : __hip_atomic_load(&a.ids[(size_t)(vf - a.H) * a.pcap + row], __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
        }
        __hip_atomic_store(&a.ids[i], w, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
    }
    const int f = i / a.pcap, k = f + a.H - a.n_frames;
    if (k >= 0 && w >= 0) a.n_id[(size_t)k * a.pcap + (i - f * a.pcap)] = w;
}

__global__ void __launch_bounds__(256) k_track_reset(uint32_t *mask, int n, int32_t *count) {
    const int i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i < n) mask[i] = 0u;
    if (i == 0) *count = 0;
}

template <typename K>
hipError_t opt_in_lds(K kernel, size_t bytes) {
    return bytes > 64 * 1024 ? hipFuncSetAttribute(reinterpret_cast<const void *>(kernel), hipFuncAttributeMaxDynamicSharedMemorySize, (int)bytes)
                             : hipSuccess;
}

}  // namespace

hipError_t track_prepare(int pcap) {
    const size_t lds = (size_t)pcap * pcap * sizeof(double);
    hipError_t e = opt_in_lds(k_track_stage<float>, lds);
    return e != hipSuccess ? e : opt_in_lds(k_track_stage<double>, lds);
}

hipError_t launch_track_reset(hipStream_t s, mpe_track_state *st) {
    const int n = st->H * st->pcap;
    hipLaunchKernelGGL(k_track_reset, dim3((n + 255) / 256), dim3(256), 0, s, st->mask[st->cur], n, st->count + st->cur);
    const hipError_t e = hipGetLastError();
    if (e == hipSuccess) ++st->launches;
    return e;
}

hipError_t launch_track(hipStream_t s, mpe_track_state *st, const mpe_track_args &x) {
    const int o = st->cur, n = o ^ 1, J = st->J;
    TrackK a{};
    a.n_frames = x.n_frames; a.pcap = st->pcap; a.J = J; a.H = st->H; a.pose_f64 = st->pose_f64; a.joint_flags = x.joint_flags;
    a.used = x.used_joint_mask & joint_bits(J);
    a.gate = x.gate;
    a.poses = x.d_poses; a.flags = x.d_flags; a.n_persons = x.d_n_persons;
    a.ids = x.d_track_id; a.cost = x.d_link_cost; a.gap = x.d_link_gap; a.issued_out = x.d_issued;
    a.o_pose = st->pose[o]; a.o_mask = st->mask[o]; a.o_id = st->id[o]; a.o_child = st->child[o]; a.o_count = st->count + o;
    a.n_pose = st->pose[n]; a.n_mask = st->mask[n]; a.n_id = st->id[n]; a.n_child = st->child[n]; a.n_count = st->count + n;
    a.ws = st->ws;
    const long long per_block = 256ll * TRK_BIRTH_BLOCKS;
    a.fpt = (int)((x.n_frames + per_block - 1) / per_block);
    a.seg = max(1, min(256, TRK_SEG_WORDS / st->pcap));
    const int rows = x.n_frames * st->pcap;
    const size_t lds = (size_t)st->pcap * st->pcap * sizeof(double);
    hipError_t e;
#define TRK_LAUNCH(...)                                  \
    hipLaunchKernelGGL(__VA_ARGS__);                     \
    if ((e = hipGetLastError()) != hipSuccess) return e; \
    ++st->launches
    TRK_LAUNCH(k_track_init, dim3((rows + 255) / 256), dim3(256), 0, s, a);
    for (int g = 1; g <= st->H; ++g) {
        if (st->pose_f64) { TRK_LAUNCH(k_track_stage<double>, dim3(x.n_frames), dim3(256), lds, s, a, g); }
        else { TRK_LAUNCH(k_track_stage<float>, dim3(x.n_frames), dim3(256), lds, s, a, g); }
    }
    TRK_LAUNCH(k_track_carry, dim3(st->H), dim3(256), 0, s, a);
    const int nb = (int)((x.n_frames + 256ll * a.fpt - 1) / (256ll * a.fpt));
    TRK_LAUNCH(k_track_birth_count, dim3(nb), dim3(256), 0, s, a);
    TRK_LAUNCH(k_track_birth_number, dim3(nb), dim3(256), 0, s, a);
    TRK_LAUNCH(k_track_resolve, dim3((x.n_frames + a.seg - 1) / a.seg), dim3(256), 0, s, a);
    TRK_LAUNCH(k_track_finish, dim3((rows + 255) / 256), dim3(256), 0, s, a);
#undef TRK_LAUNCH
    st->cur = n;
    return hipSuccess;
}

}  // namespace mpe
