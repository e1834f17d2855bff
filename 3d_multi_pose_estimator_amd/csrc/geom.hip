// mpe_geom_scores_batch: a score per edge-node from the calibration alone -- the mean distance between the back-projected
// rays of the two skeletons, over the joints both have -- binary64, in the order include/mpe.h gives.
//
// k_geom: one 256-thread workgroup per frame.  A record per head -- the unit rays of its joints (three doubles each) and a
// word with the joints that may vote and the camera -- lives in LDS, or, for contexts whose max_heads_per_frame records
// exceed GEOM_LDS_BYTES, in the context's table (indexed by the batch's head number; same code, same bits).  Phase 0:
// the camera centres (thread c) and the word of every head (thread h: presence, the caller's joint mask, the confidence
// test).  Phase 1: the ray of every (head, joint) that may vote, ONCE (a head takes part in (V - 1) P edge-nodes):
// undistort_point of dlt_common.h, two Newton steps on the lens model, the rotation, the norm (rays64.h, shared with
// consolidate.hip).  Phase 2: a 32-lane half of a wave is one edge-node (the pair
// comes from the table k_topology / k_topology_explicit wrote, so implicit and explicit lists are one code path; the
// pairs of 32 iterations are fetched by one load per lane beforehand, the loop itself touches the head records only),
// lane j owns joint j: closest points of the two rays, clamped to the front of both cameras, their distance.  The votes
// of the half are a ballot; every lane then folds the distances in increasing j through shuffles (a fixed order, whatever
// the lanes did) and lane 0 stores.  No atomics.  The file turns contraction off; f64 quotients and roots are the
// language's correctly rounded ones.
#include "rays64.h"

#pragma clang fp contract(off)

namespace mpe {

namespace {

constexpr int GEOM_THREADS = 256;
static_assert(MPE_MAX_JOINTS <= 32 && MPE_MAX_CAMERAS <= GEOM_THREADS, "a half wave holds the joints of an edge-node");

struct GeomK {
    int V, J, hmax, m_cap;                    // m_cap: edge-nodes a frame of an explicit list may hold (0: implicit list)
    double sigma, clip;
    int min_joints;
    uint32_t joint_mask;                      // already restricted to the J joints
    float min_conf;
    const int32_t *head_off, *en_off, *head_cam, *en_pair;
    const uint32_t *present;
    const double *xy;
    const float *vp;
    double *table;                            // the table route: [n_heads][3 J + 1]
    float *scores;
    uint8_t *n_votes;
    double *mean;
};

// per head: J unit rays (three doubles each), then one 8-byte word: the joints that may vote | the camera
__device__ inline size_t rec_doubles(int J) { return (size_t)J * 3 + 1; }

template <bool TABLE>
__global__ void __launch_bounds__(GEOM_THREADS) k_geom(const DevCfg *__restrict__ cfg, GeomK a) {
    extern __shared__ double s_dyn[];
    __shared__ double s_o[MPE_MAX_CAMERAS][3];
    const int f = blockIdx.x, t = threadIdx.x;
    const int h0 = a.head_off[f], H = a.head_off[f + 1] - h0;
    const int e0 = a.en_off[f], M = a.en_off[f + 1] - e0;
    if (M <= 0) return;
    if (H > a.hmax || H < 0 || (a.m_cap > 0 && M > a.m_cap)) {
        // beyond the per-frame capacity (the topology launch raised the status bit): defined output, nothing computed
        for (int m = t; m < M; m += GEOM_THREADS) {
            a.scores[(size_t)e0 + m] = 0.0f;
            if (a.n_votes) a.n_votes[(size_t)e0 + m] = 0;
            if (a.mean) a.mean[(size_t)e0 + m] = -1.0;
        }
        return;
    }
    const size_t rec = rec_doubles(a.J);
    double *heads = TABLE ? a.table + (size_t)h0 * rec : s_dyn;

    // phase 0: the camera centres; per head the joints that may vote (present, asked for, confident) and the camera
    if (t < a.V) {
        camera_centre(cfg, t, s_o[t]);
    }
    for (int h = t; h < H; h += GEOM_THREADS) {
        const int c = a.head_cam[h0 + h];
        uint32_t ok = (unsigned)c < (unsigned)a.V ? a.present[h0 + h] & a.joint_mask : 0u;
        const float *conf = a.vp + (size_t)(h0 + h) * a.J * 2;
        for (int j = 0; j < a.J; ++j)
            if (!(conf[2 * j] >= a.min_conf)) ok &= ~(1u << j);
        int2 *word = reinterpret_cast<int2 *>(heads + (size_t)h * rec + (size_t)a.J * 3);
        *word = make_int2((int)ok, c);
    }
    __syncthreads();
    // phase 1: the unit ray of every joint that may vote
    for (int i = t; i < H * a.J; i += GEOM_THREADS) {
        const int h = i / a.J, j = i - h * a.J;
        const int2 word = *reinterpret_cast<const int2 *>(heads + (size_t)h * rec + (size_t)a.J * 3);
        if (!(((uint32_t)word.x >> j) & 1u)) continue;
        const int c = word.y;
        const double *px = a.xy + ((size_t)(h0 + h) * a.J + j) * 2;
        unit_ray(cfg, c, px[0], px[1], heads + (size_t)h * rec + (size_t)j * 3);
    }
    __syncthreads();                          // (also orders the table's global stores for this workgroup's reads)

    // phase 2: half wave g takes the edge-nodes mc + 8 it + g of a chunk of 256; lane `it` fetched that pair beforehand,
    // so the loop body reads LDS (or the table) only
    const int j = t & 31, g = t >> 5, half = g & 1;
    const bool mine = j < a.J;
    for (int mc = 0; mc < M; mc += GEOM_THREADS) {
        int2 pr = make_int2(-1, -1);
        if (mc + 8 * j + g < M) pr = *reinterpret_cast<const int2 *>(a.en_pair + 2 * ((size_t)e0 + mc + 8 * j + g));
        const int its = min(32, (M - mc + 7) / 8);               // uniform: every lane reaches the shuffles
        for (int it = 0; it < its; ++it) {
            const int m = mc + 8 * it + g;
            const bool live = m < M;
            const int h1 = __shfl(pr.x, it, 32), h2 = __shfl(pr.y, it, 32);
            const bool inside = live && (unsigned)h1 < (unsigned)H && (unsigned)h2 < (unsigned)H;
            int2 w1 = make_int2(0, 0), w2 = make_int2(0, 0);
            if (inside) {
                w1 = *reinterpret_cast<const int2 *>(heads + (size_t)h1 * rec + (size_t)a.J * 3);
                w2 = *reinterpret_cast<const int2 *>(heads + (size_t)h2 * rec + (size_t)a.J * 3);
            }
            const int c1 = w1.y, c2 = w2.y;
            const bool vote = inside && mine && c1 != c2 && ((((uint32_t)w1.x & (uint32_t)w2.x) >> j) & 1u);
            double dist = 0.0;
            if (vote) {
                dist = ray_distance(heads + (size_t)h1 * rec + (size_t)j * 3, heads + (size_t)h2 * rec + (size_t)j * 3, s_o[c1], s_o[c2], a.clip);
            }
            const uint32_t votes = (uint32_t)(__ballot(vote) >> (32 * half));
            double sum = 0.0;
            for (int q = 0; q < a.J; ++q) {
                const double dq = __shfl(dist, q, 32);
                if ((votes >> q) & 1u) sum = sum + dq;
            }
            if (live && j == 0) {
                const int n = __popc(votes);
                const double mean = n ? sum / (double)n : -1.0;
                a.scores[(size_t)e0 + m] = n >= a.min_joints ? (float)(a.sigma / (a.sigma + mean)) : 0.0f;
                if (a.n_votes) a.n_votes[(size_t)e0 + m] = (uint8_t)n;
                if (a.mean) a.mean[(size_t)e0 + m] = mean;
            }
        }
    }
}

}  // namespace

size_t geom_lds_bytes(int max_heads_per_frame, int J) { return (size_t)max_heads_per_frame * ((size_t)J * 3 + 1) * sizeof(double); }

size_t geom_table_doubles(int max_heads, int J) { return (size_t)max_heads * ((size_t)J * 3 + 1); }

bool geom_needs_table(int max_heads_per_frame, int J) { return geom_lds_bytes(max_heads_per_frame, J) > GEOM_LDS_BYTES; }

hipError_t launch_geom(hipStream_t s, const DevCfg *cfg, int V, int J, const mpe_batch &b, const int32_t *en_pair, int max_heads_per_frame,
                       int x_m_cap, const mpe_geom_args &x, float *scores, double *ray_table) {
    if (b.n_frames <= 0 || b.n_edge_nodes <= 0) return hipSuccess;
    const uint32_t all = J >= 32 ? 0xFFFFFFFFu : (1u << J) - 1u;
    GeomK a{V, J, max_heads_per_frame, b.d_en_pair ? x_m_cap : 0, x.sigma_m, x.clip_m, x.min_joints, x.joint_mask ? x.joint_mask & all : all,
            x.min_conf, b.d_frame_head_off, b.d_frame_en_off, b.d_head_cam, en_pair, b.d_joint_mask, b.d_xy, b.d_vp, ray_table, scores,
            x.d_n_votes, x.d_mean};
    if (geom_needs_table(max_heads_per_frame, J)) {
        if (!ray_table) return hipErrorInvalidValue;
        hipLaunchKernelGGL(k_geom<true>, dim3(b.n_frames), dim3(GEOM_THREADS), 0, s, cfg, a);
    } else {
        hipLaunchKernelGGL(k_geom<false>, dim3(b.n_frames), dim3(GEOM_THREADS), geom_lds_bytes(max_heads_per_frame, J), s, cfg, a);
    }
    return hipGetLastError();
}

}  // namespace mpe
