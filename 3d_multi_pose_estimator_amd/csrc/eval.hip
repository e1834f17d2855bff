// Evaluation: the per-frame error table and the pose-to-ground-truth assignment of the callers' scoring loop
// (test/metrics_from_model.py:303-337, test/metrics_from_triangulation.py:281-320), batched.
//
// k_eval_table: one workgroup per frame.  Detections are compacted in person order, then every (GT body, detection)
// pair gets the mean joint distance in the arithmetic numpy uses on the host:
//   f32 poses (MLP mode): float32 difference; numpy's float32 dot (OpenBLAS sdot: f32 products summed in f64 from 0,
//     rounded to f32); f32 sqrt (correctly rounded, taken in f64); f32 running sum; f32 divide (taken in f64).
//   f64 poses (triangulation): f64 difference; numpy's float64 dot (OpenBLAS ddot: dx*dx, then two fused
//     multiply-adds); f64 sqrt, sum, divide.
// Nothing else may be fused: the file turns contraction off and writes the one fused step it wants as fma().
//
// k_eval_assign: one wave per frame, lane c = column c.  Exact depth-first branch-and-bound over the permutations in
// itertools order (rows g = 0..G-1 pick columns of range(N), N = max(G, R), columns >= R contribute 0).  A node's
// children are kept when their bound -- the left fold of the partial sum followed by the row minima of the rows below --
// is < the incumbent, computed for all columns at once and re-checked every time the search comes back to the node
// (the incumbent only falls).  Rounding is monotone, so a pruned subtree holds no sum the reference's strict `<`
// would accept.  Of the columns >= R (all zero) only the lowest unused one is tried: the others give the same sums
// later in itertools order.  The search stack lives in registers, lane d holding depth d's entry.
#include "mpe_internal.h"
#include "pose_rows.h"

#pragma clang fp contract(off)

namespace mpe {

namespace {

constexpr int EVAL_NMAX = 64;                 // max(G, R) the device search takes (u64 column masks)
// loop iterations of one frame's search: more than the whole tree of a 10 x 10 frame (9.9 M nodes), which a table whose
// columns all look alike (every row prefers the same detections) comes close to needing -- the row-minimum bound cannot
// tell such rows apart; a few seconds of one wave at worst
constexpr long long EVAL_NODE_BUDGET = 1ll << 24;

struct EvalK : PoseRows {             // no track ids here: PoseRows::tid stays null
    int gcap;
    uint32_t used;
    const float *gt_xyz;
    const uint8_t *gt_joint;
    const int32_t *n_gt_in;
    const uint8_t *skip;
    double *table;
    int32_t *assign;
    double *err;
    uint8_t *invalid;
    int32_t *n_gt, *n_res, *status;
};

__device__ double pair_error(const EvalK &a, size_t fp, size_t fg) {
    const uint8_t *gj = a.gt_joint + fg * a.J;
    const float *gt = a.gt_xyz + fg * a.J * 3;
    if (a.pose_f64) {
        const double *p = static_cast<const double *>(a.poses) + fp * a.J * 3;
        double tot = 0.0;
        int n = 0;
        for (int j = 0; j < a.J; ++j) {
            if (!gj[j] || !((a.used >> j) & 1u) || !joint_flag(a, fp, j)) continue;
            const double dx = p[3 * j] - (double)gt[3 * j];
            const double dy = p[3 * j + 1] - (double)gt[3 * j + 1];
            const double dz = p[3 * j + 2] - (double)gt[3 * j + 2];
            double s = dx * dx;
            s = fma(dy, dy, s);
            s = fma(dz, dz, s);
            tot = tot + sqrt(s);
            ++n;
        }
        return n ? tot / (double)n : 0.0;
    }
    const float *p = static_cast<const float *>(a.poses) + fp * a.J * 3;
    float tot = 0.f;
    int n = 0;
    for (int j = 0; j < a.J; ++j) {
        if (!gj[j] || !((a.used >> j) & 1u) || !joint_flag(a, fp, j)) continue;
        const float dx = p[3 * j] - gt[3 * j];
        const float dy = p[3 * j + 1] - gt[3 * j + 1];
        const float dz = p[3 * j + 2] - gt[3 * j + 2];
        const float px = dx * dx, py = dy * dy, pz = dz * dz;
        const float s = (float)(((double)px + (double)py) + (double)pz);
        tot = tot + (float)sqrt((double)s);
        ++n;
    }
    return n ? (double)(float)((double)tot / (double)n) : 0.0;
}

__global__ void __launch_bounds__(256) k_eval_table(EvalK a) {
    __shared__ int32_t s_det[1024];
    __shared__ int32_t s_R;
    const int f = blockIdx.x;
    const bool skip = a.skip && a.skip[f];
    const int G = skip ? 0 : min(max(a.n_gt_in[f], 0), a.gcap);
    if (threadIdx.x == 0) {
        int R = 0;
        if (!skip) {
            const int np = rows_in_frame(a, f);
            for (int p = 0; p < np; ++p)
                if (a.joint_flags || a.flags[(size_t)f * a.pcap + p]) s_det[R++] = p;
        }
        s_R = R;
        a.n_gt[f] = G;
        a.n_res[f] = R;
        a.status[f] = skip ? MPE_EVAL_SKIPPED : 0;
    }
    __syncthreads();
    const int R = s_R;
    for (int r = threadIdx.x; r < a.pcap; r += blockDim.x) {
        const size_t o = (size_t)f * a.pcap + r;
        a.assign[o] = -1;
        a.err[o] = 0.0;
        uint8_t bad = 0;
        if (r < R && a.joint_flags) {
            const size_t fp = (size_t)f * a.pcap + s_det[r];
            for (int g = 0; g < G && !bad; ++g) {
                const uint8_t *gj = a.gt_joint + ((size_t)f * a.gcap + g) * a.J;
                for (int j = 0; j < a.J; ++j)
                    if (gj[j] && ((a.used >> j) & 1u) && !joint_flag(a, fp, j)) { bad = 1; break; }
            }
        }
        a.invalid[o] = bad;
    }
    for (int i = threadIdx.x; i < a.gcap * a.pcap; i += blockDim.x) {
        const int g = i / a.pcap, r = i - g * a.pcap;
        a.table[(size_t)f * a.gcap * a.pcap + i] =
            (g < G && r < R) ? pair_error(a, (size_t)f * a.pcap + s_det[r], (size_t)f * a.gcap + g) : 0.0;
    }
}

__device__ inline double row_fold(double b, const double *s_rm, int from, int G) {
    for (int k = from; k < G; ++k) b = b + s_rm[k];
    return b;
}

__global__ void __launch_bounds__(64) k_eval_assign(EvalK a) {
    __shared__ double s_t[EVAL_NMAX * EVAL_NMAX];
    __shared__ double s_rm[EVAL_NMAX];
    const int f = blockIdx.x, lane = threadIdx.x;
    if (a.status[f] & MPE_EVAL_SKIPPED) return;
    const int G = a.n_gt[f], R = a.n_res[f];
    const int N = max(G, R);
    if (G == 0) return;                                     // one empty permutation: nothing assigned
    if (N > EVAL_NMAX) {
        if (lane == 0) a.status[f] |= MPE_EVAL_OVER_CAP;
        return;
    }
    const double *tab = a.table + (size_t)f * a.gcap * a.pcap;
    for (int i = lane; i < G * EVAL_NMAX; i += 64) {
        const int g = i / EVAL_NMAX, c = i - g * EVAL_NMAX;
        s_t[i] = c < R ? tab[(size_t)g * a.pcap + c] : 0.0;
    }
    __syncthreads();
    if (lane < G) {
        double m = s_t[lane * EVAL_NMAX];
        for (int c = 1; c < N; ++c) m = fmin(m, s_t[lane * EVAL_NMAX + c]);
        s_rm[lane] = m;
    }
    __syncthreads();

    const unsigned long long below_n = N >= 64 ? ~0ull : (1ull << N) - 1, below_r = R >= 64 ? ~0ull : (1ull << R) - 1;
    const unsigned long long zero_cols = below_n & ~below_r;    // the columns >= R
    unsigned long long used = 0;
    unsigned long long cand_reg = lane == 0 ? ~0ull : 0ull;      // lane d: children of depth d's node still to try
    double acc_reg = 0.0;                                        // lane d: left fold of rows 0..d-1
    int path_reg = -1, best_reg = -1;                            // lane d: column of row d (current / incumbent)
    double best = 10000.;
    bool have = false;
    int d = 0;
    long long iters = 0;
    while (true) {
        if (++iters > EVAL_NODE_BUDGET) {
            if (lane == 0) a.status[f] |= MPE_EVAL_OVER_BUDGET;
            return;
        }
        const unsigned long long cd = __shfl(cand_reg, d);
        const double acc = __shfl(acc_reg, d);
        bool ok = lane < N && !((used >> lane) & 1ull) && ((cd >> lane) & 1ull);
        if (lane >= R) {
            const unsigned long long z = zero_cols & ~used;
            ok = ok && z && lane == __ffsll((long long)z) - 1;
        }
        if (ok) ok = row_fold(acc + s_t[d * EVAL_NMAX + lane], s_rm, d + 1, G) < best;
        const unsigned long long m = __ballot(ok);
        if (m == 0) {
            if (d == 0) break;
            --d;
            used &= ~(1ull << __shfl(path_reg, d));
            continue;
        }
        const int c = __ffsll((long long)m) - 1;
        if (lane == d) {
            cand_reg = m & ~(1ull << c);
            path_reg = c;
        }
        const double na = acc + s_t[d * EVAL_NMAX + c];
        if (d + 1 == G) {                                        // leaf: its bound was the sum itself, < best
            best = na;
            have = true;
            best_reg = path_reg;
            continue;
        }
        used |= 1ull << c;
        ++d;
        if (lane == d) {
            cand_reg = ~0ull;
            acc_reg = na;
        }
    }
    if (!have) {
        if (lane == 0) a.status[f] |= MPE_EVAL_NO_ASSIGNMENT;
        return;
    }
    if (lane < G && best_reg < R) {
        const size_t o = (size_t)f * a.pcap + best_reg;
        a.assign[o] = lane;
        a.err[o] = s_t[lane * EVAL_NMAX + best_reg];
    }
}

}  // namespace

hipError_t launch_eval(hipStream_t s, const mpe_eval_args &x) {
    EvalK a{{x.n_frames, x.pcap, x.n_joints, x.pose_f64, x.joint_flags, x.d_poses, x.d_flags, x.d_n_persons, nullptr},
            x.gcap, x.used_joint_mask, x.d_gt_xyz, x.d_gt_joint, x.d_n_gt_in, x.d_skip, x.d_table, x.d_assign, x.d_err,
            x.d_invalid, x.d_n_gt, x.d_n_res, x.d_status};
    hipLaunchKernelGGL(k_eval_table, dim3(x.n_frames), dim3(256), 0, s, a);
    hipError_t e = hipGetLastError();
    if (e != hipSuccess) return e;
    hipLaunchKernelGGL(k_eval_assign, dim3(x.n_frames), dim3(64), 0, s, a);
    return hipGetLastError();
}

}  // namespace mpe
