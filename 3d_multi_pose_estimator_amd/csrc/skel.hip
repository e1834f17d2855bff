// Skeleton: bone lengths held constant along a track (include/mpe.h: mpe_skel_*; the numpy statement is
// harness/skeleton.py).  Three kernels, one per call whatever the frame count:
//
// k_skel_observe   one thread per (frame, row, bone): the length of a live bone of a detection goes into the histogram of
//                  its (track id, bone) with one integer atomicAdd whose result nobody reads.  Integer additions commute,
//                  so the state does not depend on chunking or frame order.
// k_skel_update    one wave per (track id, bone): each lane sums eight bins, a wave prefix sum finds the lane that holds
//                  the lower median, that lane finds the bin.
// k_skel_fit       SKW lanes per (frame, row), SKR rows per one-wave workgroup.  The working poses (f64) and the rows'
//                  lengths sit in LDS row-minor ([value][row]): a bone's joints are indexed at run time, which registers
//                  cannot do without scratch.  Two bones that share no joint commute exactly, so the sequence of
//                  iters * n_bones bone updates is cut at create time into steps (skel_schedule): an update goes one step
//                  after the later of the last updates that touch its joints, whatever their sweep, and the updates of a
//                  step run side by side, one per lane, with a barrier of the workgroup between steps.  The dependent
//                  chain of (sqrt, /) pairs is then as long as the bone list is deep, not as long as it is: one lane
//                  per row walking the list in order gave the same bits in 2.65 times the time.
#include "mpe_internal.h"

#include <algorithm>
#include <vector>

#pragma clang fp contract(off)

namespace mpe {

namespace {

struct SkelK {
    int n_frames, pcap, J, n_bones, joint_flags, iters, tid_cap;
    uint32_t jmask;                  // joint_mask, cut to the J joints
    double bin_width;
    const void *poses;
    const uint8_t *flags;
    const int32_t *n_persons;
    const int32_t *tid;
    void *poses_out;
    double *err;
    uint8_t *n_bones_out;
    const int32_t *bones;
    uint32_t *hist;
    const double *len;
    unsigned long long *ctr;         // out_of_range, over_ids, status
    const uint32_t *sched;           // [n_steps + 1][SKW] bone updates, SK_NONE: none
    int n_steps;
};

constexpr int SKW = 8, SKR = 64 / SKW;                       // lanes per row and rows per wave of the fit
constexpr uint32_t SK_NONE = 0xFFFFFFFFu;                    // else sweep << 15 | bone << 10 | parent << 5 | child

// the id of row fp = f * pcap + p when it is a detection, else -1
__device__ inline int32_t row_id(const SkelK &a, size_t fp) {
    const size_t f = fp / a.pcap;
    const int p = (int)(fp - f * a.pcap);
    if (p >= min(max(a.n_persons[f], 0), a.pcap)) return -1;
    const int32_t t = a.tid[fp];
    if (t < 0) return -1;
    if (!a.joint_flags && !a.flags[fp]) return -1;
    return t;
}

// joint j of a detection: present and inside the mask (its coordinates are looked at by the caller)
__device__ inline bool joint_on(const SkelK &a, size_t fp, int j) {
    if (!((a.jmask >> j) & 1u)) return false;
    return !a.joint_flags || a.flags[fp * a.J + j] != 0;
}

__device__ inline bool finite3(double x, double y, double z) {
    return __builtin_isfinite(x) && __builtin_isfinite(y) && __builtin_isfinite(z);
}

__device__ inline double length3(double dx, double dy, double dz) {
    const double s = (dx * dx + dy * dy) + dz * dz;
    return sqrt(s);
}

template <typename T>
__global__ void __launch_bounds__(256) k_skel_observe(SkelK a) {
    const size_t i = (size_t)blockIdx.x * 256 + threadIdx.x;
    const size_t total = (size_t)a.n_frames * a.pcap * a.n_bones;
    if (i >= total) return;
    const size_t fp = i / a.n_bones;
    const int b = (int)(i - fp * a.n_bones);
    const int32_t t = row_id(a, fp);
    if (t < 0) return;
    if (t >= a.tid_cap) {
        if (b == 0) {
            atomicAdd(&a.ctr[1], 1ull);
            atomicOr(&a.ctr[2], (unsigned long long)MPE_SKEL_OVER_IDS);
        }
        return;
    }
    const int jp = a.bones[2 * b], jc = a.bones[2 * b + 1];
    if (!joint_on(a, fp, jp) || !joint_on(a, fp, jc)) return;
    const T *x = static_cast<const T *>(a.poses) + fp * a.J * 3;
    const double px = (double)x[3 * jp], py = (double)x[3 * jp + 1], pz = (double)x[3 * jp + 2];
    const double cx = (double)x[3 * jc], cy = (double)x[3 * jc + 1], cz = (double)x[3 * jc + 2];
    if (!finite3(px, py, pz) || !finite3(cx, cy, cz)) return;
    const double l = length3(cx - px, cy - py, cz - pz);
    const double q = l / a.bin_width;
    if (l > 0.0 && q < (double)MPE_SKEL_BINS)
        atomicAdd(&a.hist[((size_t)t * a.n_bones + b) * MPE_SKEL_BINS + (int)q], 1u);
    else
        atomicAdd(&a.ctr[0], 1ull);
}

__global__ void __launch_bounds__(256) k_skel_update(const uint32_t *hist, double *len, int32_t *count, int n_pairs, int min_samples,
                                                     double bin_width) {
    const int lane = threadIdx.x & 63;
    const int pair = blockIdx.x * 4 + (threadIdx.x >> 6);
    if (pair >= n_pairs) return;                             // the whole wave
    const uint4 *h = reinterpret_cast<const uint4 *>(hist + (size_t)pair * MPE_SKEL_BINS) + 2 * lane;
    const uint4 u = h[0], v = h[1];
    const uint32_t c[8] = {u.x, u.y, u.z, u.w, v.x, v.y, v.z, v.w};
    unsigned long long own = 0;
#pragma unroll
    for (int i = 0; i < 8; ++i) own += c[i];
    unsigned long long incl = own;
    for (int d = 1; d < 64; d <<= 1) {
        const unsigned long long o = __shfl_up(incl, d, 64);
        if (lane >= d) incl += o;
    }
    const unsigned long long n = __shfl(incl, 63, 64);
    if (lane == 0) count[pair] = n > 0x7FFFFFFFull ? 0x7FFFFFFF : (int32_t)n;
    if (n < (unsigned long long)max(min_samples, 1)) {
        if (lane == 0) len[pair] = 0.0;
        return;
    }
    const unsigned long long excl = incl - own;
    if (2 * incl >= n && 2 * excl < n) {                     // one lane: the bins before it hold less than half
        unsigned long long cum = excl;
        int k = -1;
#pragma unroll
        for (int i = 0; i < 8; ++i) {
            cum += c[i];
            if (k < 0 && 2 * cum >= n) k = 8 * lane + i;
        }
        len[pair] = ((double)k + 0.5) * bin_width;
    }
}

template <typename T>
struct Bits;
template <>
struct Bits<float> { typedef uint32_t type; };
template <>
struct Bits<double> { typedef uint64_t type; };

// x: the row's column of the working pose, value v at x[v * S]
template <int S>
__device__ inline double bone_length(const double *x, int jp, int jc) {
    return length3(x[(3 * jc) * S] - x[(3 * jp) * S], x[(3 * jc + 1) * S] - x[(3 * jp + 1) * S], x[(3 * jc + 2) * S] - x[(3 * jp + 2) * S]);
}

// one bone update of a sweep on the working pose (stride S between values), L > 0 its length
template <int S>
__device__ inline void bone_update(double *x, int jp, int jc, double L) {
    double *xp = x + (3 * jp) * S, *xc = x + (3 * jc) * S;
    const double dx = xc[0] - xp[0], dy = xc[S] - xp[S], dz = xc[2 * S] - xp[2 * S];
    const double l = length3(dx, dy, dz);
    if (!(l > 0.0)) return;
    const double e = (l - L) / l;
    const double h = 0.5 * e;
    const double mx = h * dx, my = h * dy, mz = h * dz;
    xp[0] = xp[0] + mx;
    xc[0] = xc[0] - mx;
    xp[S] = xp[S] + my;
    xc[S] = xc[S] - my;
    xp[2 * S] = xp[2 * S] + mz;
    xc[2 * S] = xc[2 * S] - mz;
}

template <typename T>
__global__ void __launch_bounds__(64) k_skel_fit(SkelK a) {
    extern __shared__ double s_skel[];                       // [J * 3][SKR] working poses, then [n_bones][SKR] lengths
    typedef typename Bits<T>::type B;
    const int lane = threadIdx.x, g = lane / SKW, k = lane % SKW, J = a.J, nb = a.n_bones;
    const size_t row = (size_t)blockIdx.x * SKR + g;
    const bool valid = row < (size_t)a.n_frames * a.pcap;    // every lane stays to the end: shuffles and barriers
    const size_t fp = valid ? row : 0;
    double *x = s_skel + g, *Ls = s_skel + (size_t)J * 3 * SKR + g;
    const T *in = static_cast<const T *>(a.poses) + fp * J * 3;
    const B *in_bits = reinterpret_cast<const B *>(in);
    B *out = static_cast<B *>(a.poses_out) + fp * J * 3;
    const int32_t t = valid ? row_id(a, fp) : -1;
    const bool known = t >= 0 && t < a.tid_cap;

    uint32_t active = 0, constrained = 0, ends = 0;
    int n_con = 0;
    double e0 = 0.0, e1 = 0.0;
    if (known)
        for (int j = k; j < J; j += SKW) {
            const double v0 = (double)in[3 * j], v1 = (double)in[3 * j + 1], v2 = (double)in[3 * j + 2];
            x[(3 * j) * SKR] = v0;
            x[(3 * j + 1) * SKR] = v1;
            x[(3 * j + 2) * SKR] = v2;
            if (joint_on(a, fp, j) && finite3(v0, v1, v2)) active |= 1u << j;
        }
    for (int d = 1; d < SKW; d <<= 1) active |= __shfl_xor(active, d, 64);
    __syncthreads();
    if (known)
        for (int b = 0; b < nb; ++b) {
            const int jp = a.bones[2 * b], jc = a.bones[2 * b + 1];
            const double L = a.len[(size_t)t * nb + b];
            if (((active >> jp) & (active >> jc) & 1u) && L > 0.0 && L < __builtin_inf()) {
                constrained |= 1u << b;
                ends |= (1u << jp) | (1u << jc);
                ++n_con;
                if (b % SKW == k) {                          // the maximum does not depend on the order it is taken in
                    Ls[b * SKR] = L;
                    const double v = fabs(bone_length<SKR>(x, jp, jc) - L);
                    if (v > e0) e0 = v;
                }
            }
        }
    __syncthreads();
    if (__any(constrained != 0)) {
        uint32_t code = a.sched[k];
        for (int s = 0; s < a.n_steps; ++s) {
            const uint32_t next = a.sched[(size_t)(s + 1) * SKW + k];       // the table has one step more than n_steps can be
            const int b = (code >> 10) & 31;
            if (code != SK_NONE && (int)(code >> 15) < a.iters && ((constrained >> b) & 1u))
                bone_update<SKR>(x, (code >> 5) & 31, code & 31, Ls[b * SKR]);
            __syncthreads();
            code = next;
        }
        for (int b = k; b < nb; b += SKW) {
            if (!((constrained >> b) & 1u)) continue;
            const double v = fabs(bone_length<SKR>(x, a.bones[2 * b], a.bones[2 * b + 1]) - Ls[b * SKR]);
            if (v > e1) e1 = v;
        }
    }
    for (int d = 1; d < SKW; d <<= 1) {
        const double o0 = __shfl_xor(e0, d, 64), o1 = __shfl_xor(e1, d, 64);
        if (o0 > e0) e0 = o0;
        if (o1 > e1) e1 = o1;
    }
    if (!valid) return;
    if (!constrained) e0 = e1 = -1.0;
    for (int j = k; j < J; j += SKW) {
        const bool moved = (ends >> j) & 1u;
        for (int c = 0; c < 3; ++c) {
            B bits = in_bits[3 * j + c];
            if (moved) {
                const T r = (T)x[(3 * j + c) * SKR];
                __builtin_memcpy(&bits, &r, sizeof(T));
            }
            out[3 * j + c] = bits;
        }
    }
    if (k == 0) {
        a.err[2 * fp] = e0;
        a.err[2 * fp + 1] = e1;
        a.n_bones_out[fp] = (uint8_t)n_con;
    }
}

SkelK skel_args(const mpe_skel_state *st, const mpe_skel_args &x) {
    const int J = st->J;
    SkelK a{};
    a.n_frames = x.n_frames; a.pcap = st->pcap; a.J = J; a.n_bones = st->n_bones; a.joint_flags = x.joint_flags; a.iters = x.iters;
    a.tid_cap = st->tid_cap;
    a.jmask = x.joint_mask & (J >= 32 ? 0xFFFFFFFFu : (1u << J) - 1u);
    a.bin_width = st->bin_width;
    a.poses = x.d_poses; a.flags = x.d_flags; a.n_persons = x.d_n_persons; a.tid = x.d_track_id;
    a.poses_out = x.d_poses_out; a.err = x.d_err; a.n_bones_out = x.d_n_bones;
    a.bones = st->bones; a.hist = st->hist; a.len = st->len; a.ctr = st->ctr;
    a.sched = st->sched;
    a.n_steps = x.iters >= 1 && x.iters <= MPE_SKEL_MAX_ITERS ? st->steps_upto[x.iters] : 0;
    return a;
}

}  // namespace

// The steps of MPE_SKEL_MAX_ITERS sweeps over the bone list: an update goes one level after the later
// of the last updates that touch its two joints; a level is cut into steps of SKW updates.  -> the table [steps + 1][SKW]
// (the last step is empty: the kernel reads one step ahead) and, per iters, the steps that hold every update of the first
// `iters` sweeps.  Updates of later sweeps in those steps are left out by the kernel.
void skel_schedule(const int32_t *bones, int n_bones, std::vector<uint32_t> *table, int *steps_upto) {
    const int n_ops = MPE_SKEL_MAX_ITERS * n_bones;
    std::vector<int> level(n_ops), last(MPE_MAX_JOINTS, 0);
    int n_levels = 0;
    for (int i = 0; i < n_ops; ++i) {
        const int jp = bones[2 * (i % n_bones)], jc = bones[2 * (i % n_bones) + 1];
        level[i] = last[jp] = last[jc] = 1 + std::max(last[jp], last[jc]);
        n_levels = std::max(n_levels, level[i]);
    }
    std::vector<std::vector<int>> by_level(n_levels + 1);
    for (int i = 0; i < n_ops; ++i) by_level[level[i]].push_back(i);
    table->clear();
    for (int it = 0; it <= MPE_SKEL_MAX_ITERS; ++it) steps_upto[it] = 0;
    for (int lv = 1; lv <= n_levels; ++lv)
        for (size_t at = 0; at < by_level[lv].size(); at += SKW) {
            const int step = (int)(table->size() / SKW);
            for (int k = 0; k < SKW; ++k) {
                uint32_t code = SK_NONE;
                if (at + k < by_level[lv].size()) {
                    const int i = by_level[lv][at + k], sweep = i / n_bones, b = i % n_bones;
                    code = (uint32_t)sweep << 15 | (uint32_t)b << 10 | (uint32_t)bones[2 * b] << 5 | (uint32_t)bones[2 * b + 1];
                    for (int it = sweep + 1; it <= MPE_SKEL_MAX_ITERS; ++it) steps_upto[it] = std::max(steps_upto[it], step + 1);
                }
                table->push_back(code);
            }
        }
    table->insert(table->end(), SKW, SK_NONE);
}

static size_t skel_fit_lds_bytes(int J, int n_bones) { return ((size_t)J * 3 + n_bones) * SKR * sizeof(double); }

hipError_t launch_skel_reset(hipStream_t s, mpe_skel_state *st) {
    const size_t pairs = (size_t)st->tid_cap * st->n_bones;
    hipError_t e = hipMemsetAsync(st->hist, 0, pairs * MPE_SKEL_BINS * sizeof(uint32_t), s);
    if (e == hipSuccess) e = hipMemsetAsync(st->len, 0, pairs * sizeof(double), s);
    if (e == hipSuccess) e = hipMemsetAsync(st->count, 0, pairs * sizeof(int32_t), s);
    if (e == hipSuccess) e = hipMemsetAsync(st->ctr, 0, 3 * sizeof(unsigned long long), s);
    return e;
}

hipError_t launch_skel_observe(hipStream_t s, mpe_skel_state *st, const mpe_skel_args &x) {
    const SkelK a = skel_args(st, x);
    const size_t total = (size_t)x.n_frames * st->pcap * st->n_bones;          // <= 2^23 * 128 * 32 = 2^35
    const dim3 grid((unsigned)((total + 255) / 256));
    if (st->pose_f64) hipLaunchKernelGGL(k_skel_observe<double>, grid, dim3(256), 0, s, a);
    else hipLaunchKernelGGL(k_skel_observe<float>, grid, dim3(256), 0, s, a);
    const hipError_t e = hipGetLastError();
    if (e == hipSuccess) ++st->launches;
    return e;
}

hipError_t launch_skel_update(hipStream_t s, mpe_skel_state *st, int min_samples) {
    const int pairs = st->tid_cap * st->n_bones;             // <= 2^17 by the cap on the histogram's bytes
    hipLaunchKernelGGL(k_skel_update, dim3((pairs + 3) / 4), dim3(256), 0, s, st->hist, st->len, st->count, pairs, min_samples, st->bin_width);
    const hipError_t e = hipGetLastError();
    if (e == hipSuccess) ++st->launches;
    return e;
}

hipError_t launch_skel_fit(hipStream_t s, mpe_skel_state *st, const mpe_skel_args &x) {
    const SkelK a = skel_args(st, x);
    const size_t rows = (size_t)x.n_frames * st->pcap;
    const size_t lds = skel_fit_lds_bytes(st->J, st->n_bones);
    const dim3 grid((unsigned)((rows + SKR - 1) / SKR));
    if (st->pose_f64) hipLaunchKernelGGL(k_skel_fit<double>, grid, dim3(64), lds, s, a);
    else hipLaunchKernelGGL(k_skel_fit<float>, grid, dim3(64), lds, s, a);
    const hipError_t e = hipGetLastError();
    if (e == hipSuccess) ++st->launches;
    return e;
}

}  // namespace mpe
