// mpe_camfit_batch: one pass of the camera fit -- every observation of every camera reduced into the camera's 105 sums (the
// 13 x 13 normal equations of a rigid perturbation, fx, fy, cx, cy and the three radial lens terms, their right-hand side
// and the cost), binary64, in the order include/mpe.h gives, so that the sums are the same bits however a recording is cut
// into batches.  k_calib_frame's contract (calib.hip) at other sizes:
//
// k_camfit_frame: one workgroup per frame.  A lane per (person, joint, camera) writes the observation's record to LDS --
// Jx[13], rx, w, Jy[13], ry, rho(e): 30 doubles at a stride of 31 -- and a byte that says whether it is summed, skipped or
// absent; then thread (c, q) folds the records of camera c in (p, j) order into S_f[c][q], every term
// rec[14] * (rec[k]*rec[l] + rec[15+k]*rec[15+l]) with l = 13 for the right-hand side.  V * 105 chains over CF_THREADS
// threads: SLOTS chains per thread, held in registers, SLOTS a template argument picked by V so that five cameras do not
// carry the registers of thirty-two.  The chains of a thread advance together record by record (they are independent, so
// their latencies overlap); each chain is still a left fold.  CF_RECORDS records fit LDS; a frame with more is taken in
// tiles of whole (p, j) pairs and the folds are carried in registers from tile to tile, in the same order.  The partials
// go to a workspace sized at create; the (c, 104) thread counts the camera's summed and skipped records on the way and
// adds them to the state with two integer atomics (the only atomics: no f64 atomic anywhere).
// k_camfit_add: one thread per (c, q) adds the partials of the frames in increasing f onto the state, as k_calib_add does.
// Two launches whatever the frame count.  The file turns contraction off; f64 quotients and roots are the language's
// correctly rounded ones.  DESIGN.md 7.17 has the sizing; profiles/camfit_resources.txt the compiler's figures.
#include "mpe_internal.h"
#include "project64.h"
#include "reproject_select.h"

#pragma clang fp contract(off)

namespace mpe {

namespace {

constexpr int CF_THREADS = 512;
constexpr int CF_N = MPE_CAMFIT_UNKNOWNS;
constexpr int CF_REC = 2 * CF_N + 4;          // doubles per record
constexpr int CF_STRIDE = CF_REC + 1;         // an odd record stride, for the reason calib.hip gives for 17
constexpr int CF_W = CF_N + 1, CF_Y = CF_N + 2;   // the weight; the first entry of the y half
constexpr int CF_RECORDS = 180;               // records per tile: 44,820 bytes of LDS, three workgroups per CU
constexpr int CF_ADD_THREADS = 128;
static_assert(CF_RECORDS >= MPE_MAX_CAMERAS, "a tile holds at least one (person, joint) pair of every camera");
static_assert(CF_REC == 30 && MPE_CAMFIT_SUMS == CF_N * (CF_N + 1) / 2 + CF_N + 1, "the record and the sums of include/mpe.h");

constexpr int cf_slots(int V) { return (V * MPE_CAMFIT_SUMS + CF_THREADS - 1) / CF_THREADS; }

enum : uint8_t { REC_ABSENT = 0, REC_SUMMED = 1, REC_SKIPPED = 2 };

struct CamfitK {
    int n_frames, pcap, V, J, pose_f64;
    double huber;
    Selection sel;
    const double *xy;
    const void *poses;
    const double *cams;                       // [V][CAMFIT_CAM] the trial set
    double *S;                                // [n_frames][V][105] partials of the call
    double *acc;                              // [V][105]
    unsigned long long *n_obs, *n_skipped;    // [V]
};

// the record of (frame f, row p, joint j, camera c) -> REC_*
__device__ inline uint8_t observe(const CamfitK &a, int f, int p, int j, int c, double *rec) {
    const long long fp = (long long)f * a.pcap + p;
    if (!sel_person(a.sel, f, p, fp)) return REC_ABSENT;
    uint32_t present = 0;
    const int head = sel_head(a.sel, f, fp, c, &present);
    if (!sel_joint(a.sel, fp, j, head, present)) return REC_ABSENT;
    double X[3], pc[3];
    load3(a.poses, a.pose_f64, (size_t)fp * a.J + j, X);
    if (!finite3(X[0], X[1], X[2])) return REC_SKIPPED;
    const double *cam = a.cams + CAMFIT_CAM * c, *dist = cam + 12;
    to_camera(cam, X[0], X[1], X[2], pc);
    if (!(pc[2] > 0.0)) return REC_SKIPPED;   // before the quotients: a skipped record computes nothing
    const float K[9] = {(float)cam[17], 0.0f, (float)cam[19], 0.0f, (float)cam[18], (float)cam[20], 0.0f, 0.0f, 1.0f};
    const Proj pr = project_pc(pc, dist, K);
    if (!finite3(pr.px, pr.py, 0.0)) return REC_SKIPPED;
    const double *o = a.xy + ((size_t)head * a.J + j) * 2;
    const double rx = pr.px - o[0], ry = pr.py - o[1];
    const double e = sqrt(rx * rx + ry * ry);
    // the six rigid unknowns: calib.hip's lines
    const double fd = radial_slope(dist, pr);
    const double da[3] = {1.0 / pc[2], 0.0, (-pr.h0) / pc[2]}, db[3] = {0.0, 1.0 / pc[2], (-pr.h1) / pc[2]};
    double cx[3], cy[3];
    for (int k = 0; k < 3; ++k) jacobian_tail(pr, K, fd, da[k], db[k], cx + k, cy + k);
    double *jx = rec, *jy = rec + CF_Y;
    jx[0] = cx[2] * pc[1] - cx[1] * pc[2];
    jx[1] = cx[0] * pc[2] - cx[2] * pc[0];
    jx[2] = cx[1] * pc[0] - cx[0] * pc[1];
    jx[3] = cx[0], jx[4] = cx[1], jx[5] = cx[2];
    jy[0] = cy[2] * pc[1] - cy[1] * pc[2];
    jy[1] = cy[0] * pc[2] - cy[2] * pc[0];
    jy[2] = cy[1] * pc[0] - cy[0] * pc[1];
    jy[3] = cy[0], jy[4] = cy[1], jy[5] = cy[2];
    // fx, fy, cx, cy and the lens terms
    jx[6] = pr.h0 * pr.f, jy[6] = 0.0;
    jx[7] = 0.0, jy[7] = pr.h1 * pr.f;
    jx[8] = 1.0, jy[8] = 0.0;
    jx[9] = 0.0, jy[9] = 1.0;
    const double gx = (double)K[0] * pr.h0, gy = (double)K[4] * pr.h1;
    const double r2 = pr.r * pr.r, r3 = r2 * pr.r;
    jx[10] = gx * pr.r, jy[10] = gy * pr.r;
    jx[11] = gx * r2, jy[11] = gy * r2;
    jx[12] = gx * r3, jy[12] = gy * r3;
    rec[CF_N] = rx;
    rec[CF_W] = huber_weight(e, a.huber);
    rec[CF_Y + CF_N] = ry;
    rec[CF_Y + CF_N + 1] = rho(e, a.huber);
    return REC_SUMMED;
}

template <int SLOTS>
__global__ void __launch_bounds__(CF_THREADS) k_camfit_frame(CamfitK a) {
    __shared__ double s_rec[CF_RECORDS * CF_STRIDE];
    __shared__ uint8_t s_kind[CF_RECORDS];
    const int f = blockIdx.x, tid = threadIdx.x;
    // this thread's (c, q) and the two record entries q multiplies: A_kl = Jx_k*Jx_l + Jy_k*Jy_l, g_k = Jx_k*rx + Jy_k*ry
    // (rx and ry sit behind the Jacobian rows, at entry 13), C = rho
    int cam[SLOTS], ek[SLOTS], el[SLOTS];
    double acc[SLOTS];
#pragma unroll
    for (int s = 0; s < SLOTS; ++s) {
        const int id = tid + s * CF_THREADS;
        const int q = id % MPE_CAMFIT_SUMS;
        cam[s] = id < a.V * MPE_CAMFIT_SUMS ? id / MPE_CAMFIT_SUMS : -1;
        int k = 0, l = q;
        if (q < CF_N * (CF_N + 1) / 2) {
            while (l >= CF_N - k) l -= CF_N - k, ++k;
            l += k;
        } else {
            k = q - CF_N * (CF_N + 1) / 2, l = CF_N;
        }
        ek[s] = q == MPE_CAMFIT_SUMS - 1 ? -1 : k;
        el[s] = l;
        acc[s] = 0.0;
    }
    unsigned long long n_sum = 0, n_skip = 0;
    int np = a.sel.n_persons[f];
    np = np < 0 ? 0 : np > a.pcap ? a.pcap : np;
    const int total = np * a.J;               // (p, j) pairs of the frame, in fold order
    const int tile = CF_RECORDS / a.V;
    for (int pj0 = 0; pj0 < total; pj0 += tile) {
        const int n = total - pj0 < tile ? total - pj0 : tile;
        for (int r = tid; r < n * a.V; r += CF_THREADS) {
            const int pj = pj0 + r / a.V;
            s_kind[r] = observe(a, f, pj / a.J, pj % a.J, r % a.V, s_rec + r * CF_STRIDE);
        }
        __syncthreads();
        for (int i = 0; i < n; ++i) {
#pragma unroll
            for (int s = 0; s < SLOTS; ++s) {
                if (cam[s] < 0) continue;
                const int r = i * a.V + cam[s];
                const uint8_t kind = s_kind[r];
                const double *rec = s_rec + r * CF_STRIDE;
                if (ek[s] < 0) {
                    n_sum += kind == REC_SUMMED;
                    n_skip += kind == REC_SKIPPED;
                    if (kind == REC_SUMMED) acc[s] = acc[s] + rec[CF_REC - 1];
                } else if (kind == REC_SUMMED) {
                    acc[s] = acc[s] + rec[CF_W] * (rec[ek[s]] * rec[el[s]] + rec[CF_Y + ek[s]] * rec[CF_Y + el[s]]);
                }
            }
        }
        __syncthreads();
    }
#pragma unroll
    for (int s = 0; s < SLOTS; ++s) {
        if (cam[s] < 0) continue;
        a.S[(size_t)f * a.V * MPE_CAMFIT_SUMS + tid + s * CF_THREADS] = acc[s];
        if (ek[s] < 0) {
            if (n_sum) atomicAdd(a.n_obs + cam[s], n_sum);
            if (n_skip) atomicAdd(a.n_skipped + cam[s], n_skip);
        }
    }
}

__global__ void __launch_bounds__(CF_ADD_THREADS) k_camfit_add(CamfitK a) {
    const int id = blockIdx.x * CF_ADD_THREADS + threadIdx.x, n = a.V * MPE_CAMFIT_SUMS;
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

}  // namespace

size_t camfit_workspace_doubles(int max_frames, int V) { return (size_t)max_frames * V * MPE_CAMFIT_SUMS; }

hipError_t launch_camfit(hipStream_t s, int V, mpe_camfit_state *st, const mpe_batch &b, const mpe_calib_args &x) {
    CamfitK a{x.n_frames, x.pcap, V, x.n_joints, x.pose_f64, x.huber_px,
              Selection{V, x.n_joints, x.joint_flags, x.joint_mask, x.threshold, b.d_frame_head_off, b.d_joint_mask, b.d_vp, x.d_persons,
                        x.d_n_persons, x.d_flags},
              b.d_xy, x.d_poses, st->cams, st->S, st->acc, st->n_obs, st->n_skipped};
    const dim3 grid((unsigned)x.n_frames), block(CF_THREADS);
    // the chains of a thread: 2 up to nine cameras, 5 up to twenty-four, 7 up to the cap
    if (cf_slots(V) <= 2)
        hipLaunchKernelGGL(k_camfit_frame<2>, grid, block, 0, s, a);
    else if (cf_slots(V) <= 5)
        hipLaunchKernelGGL(k_camfit_frame<5>, grid, block, 0, s, a);
    else
        hipLaunchKernelGGL(k_camfit_frame<cf_slots(MPE_MAX_CAMERAS)>, grid, block, 0, s, a);
    hipError_t e = hipGetLastError();
    if (e != hipSuccess) return e;
    ++st->launches;
    hipLaunchKernelGGL(k_camfit_add, dim3((V * MPE_CAMFIT_SUMS + CF_ADD_THREADS - 1) / CF_ADD_THREADS), dim3(CF_ADD_THREADS), 0, s, a);
    if ((e = hipGetLastError()) != hipSuccess) return e;
    ++st->launches;
    return hipSuccess;
}

// the sums and the counts back to zero; stream-ordered memsets, no kernel
hipError_t launch_camfit_clear(hipStream_t s, mpe_camfit_state *st, int V) {
    hipError_t e = hipMemsetAsync(st->acc, 0, (size_t)V * MPE_CAMFIT_SUMS * sizeof(double), s);
    if (e == hipSuccess) e = hipMemsetAsync(st->n_obs, 0, (size_t)V * sizeof(unsigned long long), s);
    if (e == hipSuccess) e = hipMemsetAsync(st->n_skipped, 0, (size_t)V * sizeof(unsigned long long), s);
    return e;
}

}  // namespace mpe
