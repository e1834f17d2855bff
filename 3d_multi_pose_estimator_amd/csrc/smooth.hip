// Smoothing: a causal, windowed, weighted line fit per (track, joint, axis) over the raw poses of the last W frames
// (include/mpe.h: mpe_smooth_batch; the numpy statement is harness/smoothing.py).  As in track.hip the history kept in
// the state stands in front of the batch as the virtual frames 0 .. W-1 and batch frame f is virtual frame W + f; a
// history slot that no frame has filled yet holds the id -1 in every row, which is a frame nobody is seen in.
//
// k_smooth_filter  one workgroup per frame.  It stages the ids and presence masks of the frame and its W predecessors
//                  in LDS, resolves for every row and age the source row (the lowest row of that frame with the row's
//                  id), and then runs over (row, joint): the samples of up to 16 ages are gathered and the three axes
//                  fitted in registers.  No output depends on another one, and nothing is carried from frame to frame.
// k_smooth_carry   writes the last W virtual frames (ids, masks, coordinates widened to f64) into the other half of the
//                  state.  It reads what the filter reads and writes nothing the filter reads.
#include "mpe_internal.h"
#include "pose_rows.h"

#pragma clang fp contract(off)

namespace mpe {

namespace {

constexpr int SMO_PCAP = MPE_TRACK_MAX_PERSONS;
constexpr int SMO_AGES = MPE_SMOOTH_MAX_WINDOW + 1;

struct SmoothK : PoseRows {
    int W, fill;
    uint32_t jmask;                  // joint_mask, cut to the J joints
    double lambda;
    void *poses_out;
    uint8_t *flags_out;
    double *vel;
    uint8_t *n_samples;
    // the state: the history read (o_) and the one written (n_), [W][pcap] each
    const double *o_pose;
    const uint32_t *o_mask;
    const int32_t *o_id;
    double *n_pose;
    uint32_t *n_mask;
    int32_t *n_id;
};

// id and present joints of row p of virtual frame vf; a row that is no detection has id -1 and no joint
__device__ inline void row_of(const SmoothK &a, int vf, int p, int32_t *id, uint32_t *mask) {
    *id = -1;
    *mask = 0u;
    if (vf < a.W) {
        const size_t o = (size_t)vf * a.pcap + p;
        *id = a.o_id[o];
        *mask = a.o_mask[o];
        return;
    }
    const int f = vf - a.W;
    if (p >= rows_in_frame(a, f)) return;
    const size_t fp = (size_t)f * a.pcap + p;
    const int32_t t = a.tid[fp];
    if (t < 0) return;
    const uint32_t m = flag_mask(a, fp);
    if (!a.joint_flags && !m) return;                    // per-joint flags: a row with an id and no joint is still a row
    *id = t;
    *mask = m;
}

template <typename T>
__device__ inline double coord_of(const SmoothK &a, int vf, int row, int c) {
    if (vf < a.W) return a.o_pose[((size_t)vf * a.pcap + row) * a.J * 3 + c];
    return (double)static_cast<const T *>(a.poses)[((size_t)(vf - a.W) * a.pcap + row) * a.J * 3 + c];
}

template <typename T>
__global__ void __launch_bounds__(256) k_smooth_filter(SmoothK a) {
    __shared__ int32_t s_id[SMO_AGES * SMO_PCAP];
    __shared__ uint32_t s_mask[SMO_AGES * SMO_PCAP];
    __shared__ int16_t s_src[SMO_AGES * SMO_PCAP];       // [age][row]: the row of frame v - age that has the row's id, -1: none
    typedef typename Bits<T>::type B;
    const int f = blockIdx.x, tx = threadIdx.x, pcap = a.pcap, J = a.J;
    const int v = a.W + f, ages = a.W + 1;               // v - age >= 0 for every age
    for (int i = tx; i < ages * pcap; i += 256) {
        const int age = i / pcap, p = i - age * pcap;
        row_of(a, v - age, p, &s_id[i], &s_mask[i]);
    }
    __syncthreads();
    for (int i = tx; i < ages * pcap; i += 256) {
        const int age = i / pcap, p = i - age * pcap;
        const int32_t t = s_id[p];
        int src = -1;
        if (t >= 0) {
            if (age == 0) src = p;
            else
                for (int q = 0; q < pcap; ++q)
                    if (s_id[age * pcap + q] == t) { src = q; break; }
        }
        s_src[i] = (int16_t)src;
    }
    __syncthreads();

    const B *in = static_cast<const B *>(a.poses) + (size_t)f * pcap * J * 3;
    B *out = static_cast<B *>(a.poses_out) + (size_t)f * pcap * J * 3;
    for (int i = tx; i < pcap * J; i += 256) {
        const int p = i / J, j = i - p * J;
        const size_t fp = (size_t)f * pcap + p, o = fp * J + j;
        const uint8_t flag_in = a.joint_flags ? a.flags[o] : a.flags[fp];
        B px[3] = {in[3 * i], in[3 * i + 1], in[3 * i + 2]};
        double vel[3] = {0.0, 0.0, 0.0};
        uint8_t flag_out = flag_in;
        int n = 0;
        if (s_id[p] >= 0 && ((a.jmask >> j) & 1u)) {
            const bool present = (s_mask[p] >> j) & 1u;
            double S0 = 0.0, S1 = 0.0, S2 = 0.0, T0[3] = {0.0, 0.0, 0.0}, T1[3] = {0.0, 0.0, 0.0}, xr[3] = {0.0, 0.0, 0.0};
            bool now = false;
            double w = 1.0;
            for (int age = 0; age < ages; ++age) {
                if (age > 0) w = w * a.lambda;
                const int q = s_src[age * pcap + p];
                if (q < 0 || !((s_mask[age * pcap + q] >> j) & 1u)) continue;
                double x[3];
                for (int c = 0; c < 3; ++c) x[c] = coord_of<T>(a, v - age, q, 3 * j + c);
                if (!finite3(x[0], x[1], x[2])) continue;
                if (n == 0) {
                    for (int c = 0; c < 3; ++c) xr[c] = x[c];
                    now = age == 0;
                }
                ++n;
                const double u = (double)age, cw = w * u;
                S0 = S0 + w;
                S1 = S1 + cw;
                S2 = S2 + cw * u;
                for (int c = 0; c < 3; ++c) {
                    const double y = x[c] - xr[c];
                    T0[c] = T0[c] + w * y;
                    T1[c] = T1[c] + cw * y;
                }
            }
            const double D = S0 * S2 - S1 * S1;
            double alpha[3], beta[3];
            bool fit = n >= 2 && D > 0.0;
            for (int c = 0; c < 3; ++c) {
                alpha[c] = xr[c] + (S2 * T0[c] - S1 * T1[c]) / D;
                beta[c] = (S0 * T1[c] - S1 * T0[c]) / D;
                fit = fit && __builtin_isfinite(alpha[c]) && __builtin_isfinite(beta[c]);
            }
            const bool take = fit && (now || (!present && a.fill));
            if (take)
                for (int c = 0; c < 3; ++c) {
                    const T r = (T)alpha[c];
                    __builtin_memcpy(&px[c], &r, sizeof(T));
                    vel[c] = -beta[c];
                }
            if (a.joint_flags) flag_out = present ? 1 : (take ? MPE_SMOOTH_FILLED : 0);
        }
        for (int c = 0; c < 3; ++c) {
            out[3 * i + c] = px[c];
            a.vel[o * 3 + c] = vel[c];
        }
        a.n_samples[o] = (uint8_t)n;
        if (a.joint_flags) a.flags_out[o] = flag_out;
        else if (j == 0) a.flags_out[fp] = flag_in;
    }
}

// next history slot k = virtual frame n_frames + k of this call
template <typename T>
__global__ void __launch_bounds__(256) k_smooth_carry(SmoothK a) {
    const int k = blockIdx.x, vf = a.n_frames + k, JJ = a.J * 3;
    for (int p = threadIdx.x; p < a.pcap; p += blockDim.x) {
        const size_t n = (size_t)k * a.pcap + p;
        row_of(a, vf, p, &a.n_id[n], &a.n_mask[n]);
    }
    for (int i = threadIdx.x; i < a.pcap * JJ; i += blockDim.x)
        a.n_pose[(size_t)k * a.pcap * JJ + i] = coord_of<T>(a, vf, i / JJ, i % JJ);
}

__global__ void __launch_bounds__(256) k_smooth_reset(int32_t *id, int n) {
    const int i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i < n) id[i] = -1;
}

}  // namespace

hipError_t launch_smooth_reset(hipStream_t s, mpe_smooth_state *st) {
    const int n = st->W * st->pcap;
    if (n == 0) return hipSuccess;
    hipLaunchKernelGGL(k_smooth_reset, dim3((n + 255) / 256), dim3(256), 0, s, st->id[st->cur], n);
    const hipError_t e = hipGetLastError();
    if (e == hipSuccess) ++st->launches;
    return e;
}

hipError_t launch_smooth(hipStream_t s, mpe_smooth_state *st, const mpe_smooth_args &x) {
    const int o = st->cur, n = o ^ 1, J = st->J;
    SmoothK a{};
    a.n_frames = x.n_frames; a.pcap = st->pcap; a.J = J; a.pose_f64 = st->pose_f64; a.joint_flags = x.joint_flags;
    a.W = st->W; a.fill = x.fill != 0;
    a.jmask = x.joint_mask & joint_bits(J);
    a.lambda = x.lambda;
    a.poses = x.d_poses; a.flags = x.d_flags; a.n_persons = x.d_n_persons; a.tid = x.d_track_id;
    a.poses_out = x.d_poses_out; a.flags_out = x.d_flags_out; a.vel = x.d_vel; a.n_samples = x.d_n_samples;
    a.o_pose = st->pose[o]; a.o_mask = st->mask[o]; a.o_id = st->id[o];
    a.n_pose = st->pose[n]; a.n_mask = st->mask[n]; a.n_id = st->id[n];
    hipError_t e;
#define SMO_LAUNCH(...)                                  \
    hipLaunchKernelGGL(__VA_ARGS__);                     \
    if ((e = hipGetLastError()) != hipSuccess) return e; \
    ++st->launches
    if (st->pose_f64) { SMO_LAUNCH(k_smooth_filter<double>, dim3(x.n_frames), dim3(256), 0, s, a); }
    else { SMO_LAUNCH(k_smooth_filter<float>, dim3(x.n_frames), dim3(256), 0, s, a); }
    if (st->W > 0) {
        if (st->pose_f64) { SMO_LAUNCH(k_smooth_carry<double>, dim3(st->W), dim3(256), 0, s, a); }
        else { SMO_LAUNCH(k_smooth_carry<float>, dim3(st->W), dim3(256), 0, s, a); }
        st->cur = n;
    }
#undef SMO_LAUNCH
    return hipSuccess;
}

}  // namespace mpe
