// Reprojection residuals and their per-camera statistics (test/reprojection_error.py:89-107, 350-430), batched.
//
// k_reproject: one lane per (frame, person, camera, joint).  A 32-lane half of a wave is one (frame, person, camera):
// its lane 0 reads the person slot, the head id, the head's joint mask and the per-person flag once and broadcasts
// them; lane j then reads its own joint (xy 16 bytes, valid 8, the pose 12 or 24: consecutive lanes, consecutive
// addresses) and stores d_res[f][p][c][j], J consecutive doubles per half and the halves back to back.  The arithmetic
// is get_projected_coordinates in fp32 in the order include/mpe.h gives, every operation rounded on its own: the file
// turns contraction off; fp32 quotients and roots are taken in f64 and rounded once (correctly rounded: 53 >= 2*24+2).
//
// mpe_residual_stats: per camera over any number of residual buffers, the count of entries >= 0, their sum, the two
// middle order statistics and the count of non-finite entries.  Non-negative doubles order like their 64-bit patterns,
// (-0.0 is keyed as +0), so a radix select over the patterns returns the very elements a sort would put in the middle: six passes of 11-bit
// digits from the top (the last one 9 bits), each k_res_hist (a 2 x 2048-bin LDS histogram per workgroup, one per
// wanted rank, merged into global memory with integer atomics) followed by k_res_pick (finds the bin that holds the
// rank, narrows the prefix, clears the bins).  The sum is reduced in a fixed order (k_res_sum: a fixed stride per
// thread, an LDS tree per workgroup, the partials folded by one wave): same input, same bits.
#include "mpe_internal.h"
#include "reproject_select.h"

#pragma clang fp contract(off)

namespace mpe {

namespace {

constexpr int RP_GROUPS = 8;                  // (frame, person, camera) triples per 256-thread workgroup

__device__ inline float div_rn(float a, float b) { return (float)((double)a / (double)b); }
__device__ inline float sqrt_rn(float a) { return (float)sqrt((double)a); }

struct ReprojK {
    int n_frames, pcap, V, J, pose_f64;
    Selection sel;                            // which entries count (reproject_select.h)
    const double *xy;
    const void *poses;
    double *res;
};

__global__ void __launch_bounds__(32 * RP_GROUPS) k_reproject(const DevCfg *__restrict__ cfg, ReprojK a) {
    const int j = threadIdx.x & 31;
    const long long n_groups = (long long)a.n_frames * a.pcap * a.V;
    for (long long g = (long long)blockIdx.x * RP_GROUPS + (threadIdx.x >> 5); g < n_groups; g += (long long)gridDim.x * RP_GROUPS) {
        const int c = (int)(g % a.V);
        const long long fp = g / a.V;
        const int f = (int)(fp / a.pcap);
        int head = -1;
        uint32_t present = 0;
        if (j == 0 && sel_person(a.sel, f, (int)(fp - (long long)f * a.pcap), fp)) head = sel_head(a.sel, f, fp, c, &present);
        head = __shfl(head, 0, 32);
        present = __shfl(present, 0, 32);
        if (j >= a.J) continue;
        double out = -1.0;
        if (sel_joint(a.sel, fp, j, head, present)) {
            float X, Y, Z;
            if (a.pose_f64) {
                const double *q = static_cast<const double *>(a.poses) + ((size_t)fp * a.J + j) * 3;
                X = (float)q[0], Y = (float)q[1], Z = (float)q[2];
            } else {
                const float *q = static_cast<const float *>(a.poses) + ((size_t)fp * a.J + j) * 3;
                X = q[0], Y = q[1], Z = q[2];
            }
            const double *P = cfg->P[c];
            float pc[3];
            for (int i = 0; i < 3; ++i)
                pc[i] = (((float)P[4 * i] * X + (float)P[4 * i + 1] * Y) + (float)P[4 * i + 2] * Z) + (float)P[4 * i + 3];
            const float kd0 = (float)cfg->dist[c][0], kd1 = (float)cfg->dist[c][1], kd2 = (float)cfg->dist[c][4];
            const float h0 = div_rn(pc[0], pc[2]), h1 = div_rn(pc[1], pc[2]);
            const float n = sqrt_rn(h0 * h0 + h1 * h1);
            const float r = n * n;
            const float fr = ((1.0f + kd0 * r) + (kd1 * r) * r) + ((kd2 * r) * r) * r;
            const float d0 = h0 * fr, d1 = h1 * fr;
            const float *K = cfg->K[c];
            float u[3];
            for (int i = 0; i < 3; ++i) u[i] = (K[3 * i] * d0 + K[3 * i + 1] * d1) + K[3 * i + 2];
            const float px = div_rn(u[0], u[2]), py = div_rn(u[1], u[2]);
            const double *o = a.xy + ((size_t)head * a.J + j) * 2;
            const double dx = (double)px - o[0], dy = (double)py - o[1];
            out = sqrt(dx * dx + dy * dy);
        }
        a.res[(size_t)g * a.J + j] = out;
    }
}

// ---- statistics -------------------------------------------------------------------------------------------------------------
constexpr int RS_BITS = 11, RS_BINS = RESIDUAL_BINS, RS_PASSES = 6;
constexpr int RS_SUM_BLOCKS = RESIDUAL_SUM_BLOCKS;
constexpr int RS_MAX_BLOCKS = 512;            // workgroups per camera of a histogram launch (grid-stride beyond)
static_assert(RS_BINS == 1 << RS_BITS && RS_BITS * (RS_PASSES - 1) < 64 && RS_BITS * RS_PASSES >= 64, "digits cover 64 bits");

__host__ __device__ inline int rs_shift(int pass) { return pass < RS_PASSES - 1 ? 64 - RS_BITS * (pass + 1) : 0; }
__host__ __device__ inline int rs_width(int pass) { return pass < RS_PASSES - 1 ? RS_BITS : 64 - RS_BITS * (RS_PASSES - 1); }

// entry i of camera c in a buffer [groups][V][J]
__device__ inline size_t rs_index(long long i, int c, int V, int J) {
    const long long g = i / J;
    return ((size_t)g * V + c) * J + (size_t)(i - g * J);
}

__global__ void __launch_bounds__(256) k_res_clear(ResidualState *st, uint32_t *hist) {
    const int c = blockIdx.x;
    for (int i = threadIdx.x; i < 2 * RS_BINS; i += blockDim.x) hist[(size_t)c * 2 * RS_BINS + i] = 0;
    if (threadIdx.x == 0) {
        ResidualState z = {};
        st[c] = z;
    }
}

// sum of the entries that are not negative (a NaN entry makes it NaN), count of the non-finite ones
__global__ void __launch_bounds__(256) k_res_sum(const double *__restrict__ res, long long n_groups, int V, int J, double *partial,
                                                 ResidualState *st) {
    __shared__ double s_sum[256];
    __shared__ unsigned long long s_bad;
    const int c = blockIdx.y;
    const long long n = n_groups * J;
    if (threadIdx.x == 0) s_bad = 0;
    __syncthreads();
    double acc = 0.0;
    unsigned bad = 0;
    for (long long i = (long long)blockIdx.x * 256 + threadIdx.x; i < n; i += (long long)gridDim.x * 256) {
        const double v = res[rs_index(i, c, V, J)];
        if (!(v < 0.0)) acc = acc + v;
        if (!(fabs(v) < __builtin_huge_val())) ++bad;
    }
    s_sum[threadIdx.x] = acc;
    if (bad) atomicAdd(&s_bad, (unsigned long long)bad);
    __syncthreads();
    for (int w = 128; w > 0; w >>= 1) {
        if ((int)threadIdx.x < w) s_sum[threadIdx.x] = s_sum[threadIdx.x] + s_sum[threadIdx.x + w];
        __syncthreads();
    }
    if (threadIdx.x == 0) {
        partial[(size_t)c * RS_SUM_BLOCKS + blockIdx.x] = s_sum[0];
        if (s_bad) atomicAdd(&st[c].nonfinite, s_bad);
    }
}

__global__ void __launch_bounds__(64) k_res_sum_fold(const double *partial, ResidualState *st) {
    __shared__ double s[RS_SUM_BLOCKS];
    const int c = blockIdx.x;
    s[threadIdx.x] = partial[(size_t)c * RS_SUM_BLOCKS + threadIdx.x];
    __syncthreads();
    for (int w = RS_SUM_BLOCKS / 2; w > 0; w >>= 1) {
        if ((int)threadIdx.x < w) s[threadIdx.x] = s[threadIdx.x] + s[threadIdx.x + w];
        __syncthreads();
    }
    if (threadIdx.x == 0) st[c].sum = st[c].sum + s[0];
}

__global__ void __launch_bounds__(256) k_res_hist(const double *__restrict__ res, long long n_groups, int V, int J, int pass,
                                                  const ResidualState *st, uint32_t *hist) {
    __shared__ uint32_t s_h[2 * RS_BINS];
    const int c = blockIdx.y;
    for (int i = threadIdx.x; i < 2 * RS_BINS; i += 256) s_h[i] = 0;
    __syncthreads();
    const unsigned long long pre0 = st[c].prefix[0], pre1 = st[c].prefix[1];
    const int shift = rs_shift(pass), width = rs_width(pass);
    const unsigned mask = (1u << width) - 1u;
    const long long n = n_groups * J;
    for (long long i = (long long)blockIdx.x * 256 + threadIdx.x; i < n; i += (long long)gridDim.x * 256) {
        const double v = res[rs_index(i, c, V, J)];
        if (!(v >= 0.0)) continue;
        // -0.0 is >= 0 and sorts with 0, but its pattern lies above +inf's: it is keyed (and returned) as +0
        const unsigned long long key = v == 0.0 ? 0ull : (unsigned long long)__double_as_longlong(v);
        const unsigned long long hi = pass ? key >> (shift + width) : 0ull;
        const unsigned d = (unsigned)(key >> shift) & mask;
        if (hi == pre0) atomicAdd(&s_h[d], 1u);
        if (hi == pre1) atomicAdd(&s_h[RS_BINS + d], 1u);
    }
    __syncthreads();
    for (int i = threadIdx.x; i < 2 * RS_BINS; i += 256)
        if (s_h[i]) atomicAdd(&hist[(size_t)c * 2 * RS_BINS + i], s_h[i]);
}

// workgroup (camera, which rank): find the bin that holds the rank, narrow, clear the bins for the next pass; the last
// pass leaves the element itself and writes the camera's results
__global__ void __launch_bounds__(256) k_res_pick(ResidualState *st, uint32_t *hist, int pass, int64_t *count, int64_t *nonfinite,
                                                  double *sum, double *mid) {
    __shared__ uint32_t s_bin[RS_BINS];
    __shared__ unsigned long long s_part[256];
    const int c = blockIdx.x, w = blockIdx.y;
    uint32_t *h = hist + ((size_t)c * 2 + w) * RS_BINS;
    constexpr int PER = RS_BINS / 256;
    unsigned long long tot = 0;
    for (int k = 0; k < PER; ++k) {
        const uint32_t v = h[threadIdx.x * PER + k];
        s_bin[threadIdx.x * PER + k] = v;
        h[threadIdx.x * PER + k] = 0;
        tot += v;
    }
    s_part[threadIdx.x] = tot;
    __syncthreads();
    if (threadIdx.x != 0) return;
    unsigned long long n = 0;
    for (int t = 0; t < 256; ++t) n += s_part[t];
    ResidualState &s = st[c];
    unsigned long long rank = s.rank[w];
    if (pass == 0) {
        rank = n ? (w ? n / 2 : (n - 1) / 2) : 0;
        if (w == 0) s.count = (long long)n;
    }
    unsigned long long digit = 0;
    if (n) {                                                     // rank < n: the bin exists
        unsigned long long before = 0;
        int t = 0;
        while (t < 255 && before + s_part[t] <= rank) before += s_part[t++];
        int b = t * PER;
        while (b < RS_BINS - 1 && before + s_bin[b] <= rank) before += s_bin[b++];
        digit = (unsigned long long)b;
        rank -= before;
    }
    s.rank[w] = rank;
    const unsigned long long prefix = pass ? (s.prefix[w] << rs_width(pass)) | digit : digit;
    s.prefix[w] = prefix;
    if (pass == RS_PASSES - 1) {
        const long long cnt = s.count;
        mid[2 * c + w] = cnt ? __longlong_as_double((long long)prefix) : __builtin_nan("");
        if (w == 0) {
            count[c] = cnt;
            nonfinite[c] = (long long)s.nonfinite;
            sum[c] = s.sum;
        }
    }
}

}  // namespace

hipError_t launch_reproject(hipStream_t s, const DevCfg *cfg, int V, const mpe_batch &b, const mpe_reproject_args &x) {
    ReprojK a{x.n_frames, x.pcap, V, x.n_joints, x.pose_f64,
              Selection{V, x.n_joints, x.joint_flags, x.joint_mask, x.threshold, b.d_frame_head_off, b.d_joint_mask, b.d_vp, x.d_persons,
                        x.d_n_persons, x.d_flags},
              b.d_xy, x.d_poses, x.d_res};
    const long long groups = (long long)x.n_frames * x.pcap * V;
    const long long blocks = (groups + RP_GROUPS - 1) / RP_GROUPS;
    hipLaunchKernelGGL(k_reproject, dim3((unsigned)(blocks < 65536 ? blocks : 65536)), dim3(32 * RP_GROUPS), 0, s, cfg, a);
    return hipGetLastError();
}

hipError_t launch_residual_stats(hipStream_t s, int V, const mpe_residual_stats_args &x, ResidualState *state, uint32_t *hist,
                                 double *partial) {
    hipError_t e;
    const int J = x.n_joints;
    hipLaunchKernelGGL(k_res_clear, dim3(V), dim3(256), 0, s, state, hist);
    if ((e = hipGetLastError()) != hipSuccess) return e;
    for (int i = 0; i < x.n_buffers; ++i) {
        if (x.n_groups[i] == 0) continue;
        hipLaunchKernelGGL(k_res_sum, dim3(RS_SUM_BLOCKS, V), dim3(256), 0, s, x.d_res[i], (long long)x.n_groups[i], V, J, partial, state);
        if ((e = hipGetLastError()) != hipSuccess) return e;
        hipLaunchKernelGGL(k_res_sum_fold, dim3(V), dim3(RS_SUM_BLOCKS), 0, s, partial, state);
        if ((e = hipGetLastError()) != hipSuccess) return e;
    }
    for (int pass = 0; pass < RS_PASSES; ++pass) {
        for (int i = 0; i < x.n_buffers; ++i) {
            if (x.n_groups[i] == 0) continue;
            const long long n = (long long)x.n_groups[i] * J;
            const long long nb = (n + 255) / 256;
            hipLaunchKernelGGL(k_res_hist, dim3((unsigned)(nb < RS_MAX_BLOCKS ? nb : RS_MAX_BLOCKS), V), dim3(256), 0, s, x.d_res[i],
                               (long long)x.n_groups[i], V, J, pass, state, hist);
            if ((e = hipGetLastError()) != hipSuccess) return e;
        }
        hipLaunchKernelGGL(k_res_pick, dim3(V, 2), dim3(256), 0, s, state, hist, pass, x.d_count, x.d_nonfinite, x.d_sum, x.d_mid);
        if ((e = hipGetLastError()) != hipSuccess) return e;
    }
    return hipSuccess;
}

}  // namespace mpe
