// Internal declarations shared by the HIP translation units of libmpe_hip.so.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>
#include <string>
#include <vector>

#include "../../include/mpe.h"
#include "gemm_form.h"
#include "pair_handoff.h"

namespace mpe {

constexpr int GEMM_BM = 128;   // activation rows per workgroup
constexpr int GEMM_BN = 80;    // output features per workgroup (5 MFMA tiles of 16)
constexpr int GEMM_BK = 32;    // K depth per LDS stage
constexpr int GEMM_BN_MAX = 208;   // widest feature tile of the GEMM variants (13 MFMA tiles)
// rows a weight matrix / bias vector is padded to: any feature tile that starts below out_dim
// stays inside the allocation
inline int weight_rows(int out_dim) { return (out_dim + 15) / 16 * 16 + GEMM_BN_MAX; }
constexpr int LD_ALIGN = 32;   // every activation / weight row stride is a multiple of this
// largest activation stride the public GEMM entry points take: k_linear_sb (gemm_sb16.hip) addresses the rows of a 256-row tile by
// a 32-bit byte offset per lane, (row - m0) * lda * 4 + chunk, computed in int: 255 * 2^21 * 4 + 128 < 2^31
constexpr int LINEAR_MAX_LDA = 1 << 21;

inline int round_up(int x, int m) { return (x + m - 1) / m * m; }

struct Linear {                // one nn.Linear, zero padded on the device
    float *w = nullptr;        // [weight_rows(out)][ldw]
    float *b = nullptr;        // [weight_rows(out)]
    unsigned short *w16 = nullptr;   // optional bf16 copy [rows][ldw16] (reduced-precision mode)
    int ldw16 = 0;
    unsigned short *w3 = nullptr;    // optional: the three bf16 planes of w, [3][weight_rows(out)][ldw] (split-bf16 mode, gemm_sb16.hip)
    int in_dim = 0, out_dim = 0, ldw = 0;
};
// elements of the padded weight matrix = stride between the bf16 planes of w3
inline size_t plane_elems(const Linear &L) { return (size_t)weight_rows(L.out_dim) * L.ldw; }

struct GatLayer {
    Linear fc1, fc2;
    float *attn_l = nullptr;   // [heads*out_dim]
    float *attn_r = nullptr;
    int in_dim = 0, heads = 0, out_dim = 0;
};

struct DevCfg {                // calibration + scalars, lives in device memory
    int32_t V, J, W, H, npj, min_views, median_axis;
    uint32_t used_joint_mask;
    float threshold;
    double median_window;      // f64: the reference's `dist_to_median < 0.05` is a comparison of doubles
    float Kinv[MPE_MAX_CAMERAS][9];
    float K[MPE_MAX_CAMERAS][9];
    float T_i[MPE_MAX_CAMERAS][16];
    double P[MPE_MAX_CAMERAS][12];
    double dist[MPE_MAX_CAMERAS][5];
};

// hipFuncSetAttribute (dynamic-LDS opt-in) is per DEVICE: remember which devices have it
struct PerDeviceFlag {
    bool done[64] = {};
    static int dev() {
        int d = 0;
        (void)hipGetDevice(&d);
        return d & 63;
    }
    bool test() const { return done[dev()]; }
    void set() { done[dev()] = true; }
};

struct ProfileRec {
    hipEvent_t start, stop;
    double flop;      // known on the host, or
    int dev_n, dev_k;  // 2 * (device-side row count) * dev_n * dev_k
    int kind;          // 0 = fp32 MFMA launch (gemm.hip), 1 = split-bf16 launch (gemm_sb16.hip)
};

// reproject.hip: per-camera state of the radix select of mpe_residual_stats
struct ResidualState {
    unsigned long long prefix[2];  // high bits fixed so far of the lower / upper middle element
    unsigned long long rank[2];    // rank of that element among the entries that share the prefix
    long long count;               // entries >= 0
    unsigned long long nonfinite;
    double sum;
};
constexpr int RESIDUAL_BINS = 2048;          // 11-bit digits
constexpr int RESIDUAL_SUM_BLOCKS = 64;      // partial sums per camera and buffer

}  // namespace mpe

struct mpe_ctx {
    mpe_config cfg;
    int device = 0;                // HIP device the context was created on (every entry point switches to it)
    int32_t *h_status = nullptr;   // page-locked twin of the status word (mpe_sync_status reads it back without a staging copy)
    bool status_queued = false;    // mpe_status_queue has ordered a read-back nobody has waited for yet
    hipStream_t status_stream = nullptr;   // the stream that read-back was ordered on (the one to synchronise before reading h_status)
    int32_t status_carry = 0;      // bits of read-backs that were overtaken by a later mpe_status_queue
    int32_t *d_status = nullptr;   // device-side status word: bit 0 = a frame exceeded max_heads_per_frame
    bool gat_ws_ready = false;     // set only after the LAST step of ensure_gat_workspace succeeded
    bool mlp_ws_ready = false;
    int gat_out_mode = 1;          // activation of the last GAT layer: 1 = sigmoid, 2 = identity (logits)
    mpe::DevCfg hcfg;
    mpe::DevCfg *d_cfg = nullptr;
    std::string err;
    // weights
    int gat_layers = 0;
    float gat_alpha = 0.15f, gat_hidden_slope = 0.01f;
    mpe::GatLayer gat[MPE_MAX_GAT_LAYERS];
    bool gat_ready[MPE_MAX_GAT_LAYERS] = {};
    float *en0_ft2 = nullptr;      // layer-0 transformed feature shared by all edge-nodes [ld]
    float *en0_a = nullptr;        // its a1 | a2 coefficients [2*heads]
    bool en0_ready = false;
    int mlp_layers = 0;
    float mlp_slope = 0.1f;
    mpe::MlpMode mlp_mode = mpe::MlpMode::Split;   // which form the MLP GEMMs run on (mpe_set_precision; gemm_form.h)
    bool gat_acc64 = false;
    bool gat_reduced = false;      // reduced precision: bf16 MFMA GEMMs + fp16 feature rows in the attention stage
    bool gat_attn_fp16 = false;    // configs[4] as BASELINE words it: fp16 feature rows (ft2) in the attention stage, GEMMs stay fp32
    bool gat_split = true;         // DEFAULT (GAT mode 4): fc1 / fc2 of layers >= 1 in the split-bf16 form (gemm_sb16.hip); layer 0 (head rows only,
                                   // gathered / grouped launches) stays on the fp32 MFMA
    mpe::Linear mlp[MPE_MAX_MLP_LAYERS];
    bool mlp_ready[MPE_MAX_MLP_LAYERS] = {};
    // workspace (sized at create / grown when weights define the widths)
    int max_nodes = 0;
    int feat_ld = 0;               // padded F
    int act_ld = 0;                // padded widest hidden activation of the GAT
    float *x0 = nullptr;           // [max_heads][feat_ld] dense head rows
    float *h0 = nullptr;           // [max_heads][feat_ld] fc1 output of layer 0
    float *xdense = nullptr;       // [max_nodes][feat_ld] caller-provided dense rows (API mirror only)
    float *hdense = nullptr;
    // layer 0 grouped by camera: only the own-camera block of a head row is non-zero
    float *xc = nullptr;           // [max_heads][l0_ld] compact J*10 features
    int l0_ld = 0;
    mpe::Linear l0_fc1[MPE_MAX_CAMERAS];   // fc1 restricted to the camera's column block, bias + W[:,0] (views into l0_w)
    float *l0_w = nullptr;         // [V][weight_rows(in_dim)][l0_ld] the per-camera matrices, contiguous (grouped launch)
    float *l0_b = nullptr;         // [weight_rows(in_dim)] their common bias
    int32_t *cam_count = nullptr;  // [V]
    int32_t *cam_list = nullptr;   // [V][max_heads] head indices of each camera
    bool l0_grouped = true;
    float *act[3] = {nullptr, nullptr, nullptr};   // [max_nodes][act_ld]
    float *a12 = nullptr;          // [max_nodes][2*16]
    int64_t json_write_launches = 0;     // kernels queued for mpe_json_write_poses (mpe_json_write_launches; counted on the host)
    int64_t l0_attention_launches = 0;   // launches of k_l0_attention this context queued (mpe_l0_attention_launches; counted on the host)
    // small batches: every cross-camera pair of a batch solved beside the clustering (cluster.hip: k_lat_tail) for the row kernel of the
    // SAME batch to fetch: two buffers [heads][hmax][J][3] f64 written in turn, and ONE note of the batch whose pairs the last
    // mpe_match_batch solved -- kept until the next batch call, used once (pair_handoff.h has the rule)
    double *pair_pts[2] = {nullptr, nullptr};
    mpe::PairHandoff handoff;
    unsigned short *gat_pl[2] = {nullptr, nullptr};   // small batches (lat.hip): activations between attention -> fc1 -> fc2 as three bf16 planes [3][lat_rows][act_ld]
    size_t gat_pl_plane = 0;       // plane stride in elements
    int lat_rows = 0;
    int32_t *head_frame = nullptr; // [max_heads]
    int32_t *en_frame = nullptr;   // [max_edge_nodes]
    int32_t *en_pair = nullptr;    // [max_edge_nodes][2] frame-local head ids
    uint16_t *head_src = nullptr;  // [max_frames][hmax][hmax + 1] in-edge sources of the heads (small frames only); explicit
                                   // pair lists: [n_frames][hmax][2 hmax] in the same allocation
    size_t head_src_cap = 0;       // entries allocated
    int x_m_cap = 0;               // explicit pair lists: edge-nodes a frame may hold (0 = mode unavailable on this context)
    int32_t *node_off = nullptr;   // [max_frames+1]
    mpe::ResidualState *res_state = nullptr;   // mpe_residual_stats: [V]
    uint32_t *res_hist = nullptr;              // [V][2][RESIDUAL_BINS]
    double *res_partial = nullptr;             // [V][RESIDUAL_SUM_BLOCKS]
    double *log_table = nullptr;               // mpe_partition_scores: log 1 .. log n_log, as mpe_set_log_table received them
    int n_log = 0;
    uint64_t *cl_keys = nullptr;   // clustering scratch
    int32_t *cl_scratch = nullptr;
    size_t cl_keys_per_frame = 0, cl_scratch_per_frame = 0;
    int mlp_ld_in = 0, mlp_ld_hidden = 0;
    float *mlp_rows = nullptr;     // [max_frames*Pcap][mlp_ld_in]
    float *mlp_act[2] = {nullptr, nullptr};
    int32_t *mlp_count = nullptr;
    float *scores_tmp = nullptr;    // [max_edge_nodes]
    double *geom_rays = nullptr;    // mpe_geom_scores_batch: [max_heads][3 J + 1] head records, only where a frame's records do not fit LDS (geom.hip)
    int32_t *person_off = nullptr;  // [max_frames+1]
    uint8_t *valid_tmp = nullptr;   // [max_frames*Pcap]
    std::vector<void *> owned;     // everything to hipFree at destroy
    // profiling
    bool profiling = false;
    std::vector<mpe::ProfileRec> prof;
    size_t prof_used = 0;
    hipEvent_t tot_start = nullptr, tot_stop = nullptr;
    bool tot_valid = false;
    double sb_ms = 0, sb_flop = 0;      // the split-bf16 launches of the records last read by mpe_profile_read
    int64_t sb_launches = 0;
    double bf_ms = 0, bf_flop = 0;      // likewise the plain bf16 launches (reduced-precision modes)
    int64_t bf_launches = 0;
};

// track.hip: what mpe_track_batch carries from call to call.  Two copies of the history ([H][pcap] rows each, H =
// max_gap + 1 frames, oldest first): a call reads copy `cur`, writes the other one and makes it current.
struct mpe_track_state {
    int pcap = 0, J = 0, H = 0, pose_f64 = 0;
    int cur = 0;
    int64_t launches = 0;           // kernels enqueued since mpe_track_create
    double *pose[2] = {};           // [H][pcap][J][3], widened to f64
    uint32_t *mask[2] = {};         // [H][pcap] used joints present; 0: not a detection
    int32_t *id[2] = {};            // [H][pcap]
    uint8_t *child[2] = {};         // [H][pcap] 1: a later detection already continues this one
    int32_t *count = nullptr;       // [2] ids issued so far
    int32_t *ws = nullptr;          // [1024] scratch of the birth pass
};

// smooth.hip: what mpe_smooth_batch carries from call to call, the raw input of the last W frames.  Two copies
// ([W][pcap] rows each, oldest first) used as mpe_track_state's are; a slot no frame has filled holds the id -1.
struct mpe_smooth_state {
    int pcap = 0, J = 0, W = 0, pose_f64 = 0;
    int cur = 0;
    int64_t launches = 0;           // kernels enqueued since mpe_smooth_create
    double *pose[2] = {};           // [W][pcap][J][3], widened to f64
    uint32_t *mask[2] = {};         // [W][pcap] joints present; 0 where the row is no detection
    int32_t *id[2] = {};            // [W][pcap] track id, -1: no detection
};

// track_score.hip: what mpe_track_score_batch carries from call to call (everything mpe_track_score_result reads back) and
// the per-call scratch, sized for max_frames frames at create time.
struct mpe_track_score_state {
    int pcap = 0, gcap = 0, gid_cap = 0, tid_cap = 0, max_frames = 0;
    int64_t launches = 0;           // kernels enqueued since mpe_track_score_create
    int64_t *totals = nullptr;      // [MPE_TS_TOTALS]: the ten int64 totals, err_sum's bits, the sticky status
    int32_t *ident = nullptr;       // [4][gid_cap]: last, present, matched, bits
    int32_t *pred_count = nullptr;  // [tid_cap]
    int32_t *table = nullptr;       // [gid_cap][tid_cap]
    int32_t *rec = nullptr;         // scratch [max_frames][gid_cap]: h of the frame's record of o, -1 miss, -2 none
    int32_t *fstat = nullptr;       // scratch [max_frames][8]: tp, fp, fn, ignored, n_gt, n_pred, over_ids, frame counted
    uint64_t *mmask = nullptr;      // scratch [max_frames][2]: detections that are matches
    double *merr = nullptr;         // scratch [max_frames * pcap]: their errors, packed in (frame, detection) order
};
#define MPE_TS_TOTALS 12

// skel.hip: the bone-length state of mpe_skel_*: a histogram per (track id, bone), the length table read from it (or
// uploaded), and the counters.  Nothing is double-buffered: observe adds integers, update and fit only read what
// earlier calls on the stream wrote.
struct mpe_skel_state {
    int pcap = 0, J = 0, pose_f64 = 0, tid_cap = 0, n_bones = 0;
    double bin_width = 0.0;
    int64_t launches = 0;           // kernels enqueued since mpe_skel_create
    int32_t *bones = nullptr;       // [n_bones][2] (parent, child)
    uint32_t *hist = nullptr;       // [tid_cap][n_bones][MPE_SKEL_BINS]
    double *len = nullptr;          // [tid_cap][n_bones], an entry > 0 and finite is a length
    int32_t *count = nullptr;       // [tid_cap][n_bones]
    unsigned long long *ctr = nullptr;   // out_of_range, over_ids, status
    uint32_t *sched = nullptr;      // the steps of the fit (skel_schedule)
    int steps_upto[MPE_SKEL_MAX_ITERS + 1] = {};   // [iters]: the steps that hold the first `iters` sweeps
    uint32_t *refine_tab = nullptr; // what the body fit reads of the bone list (skel_refine_tables)
    int n_colours = 0;              // colours of the joints: two joints of one colour share no bone
};

// relink.hip: what mpe_relink_batch carries from call to call (canon and one record per canonical id), the counters, and
// the per-call scratch sized for max_frames frames at create time.  Nothing is double-buffered: one workgroup walks the
// frames of a call in order.  `frame` lives on the host: every call knows how many frames the calls before it had.
struct mpe_relink_state {
    int pcap = 0, J = 0, pose_f64 = 0, tid_cap = 0, n_bones = 0, max_frames = 0;
    mpe_relink_config cfg = {};     // the options as created; cfg.bones points at bones_host
    std::vector<int32_t> bones_host;
    int64_t frame = 0;              // frames seen since create / reset
    int64_t launches = 0;           // kernels enqueued since mpe_relink_create
    int32_t *bones = nullptr;       // [n_bones][2] (parent, child)
    int32_t *canon = nullptr;       // [3][tid_cap]: canon, last_frame, seen (the last frame the record was present in)
    double *last_pose = nullptr;    // [tid_cap][J][3]
    uint32_t *last_mask = nullptr;  // [tid_cap]
    double *sum = nullptr;          // [tid_cap][n_bones]
    int32_t *cnt = nullptr;         // [tid_cap][n_bones]
    unsigned long long *ctr = nullptr;   // births, linked, over_ids, status
    double *row_len = nullptr;      // scratch [max_frames * pcap][n_bones]
    uint32_t *row_act = nullptr;    // scratch [max_frames * pcap]
    int32_t *row_id = nullptr;      // scratch [max_frames * pcap]
    double *table = nullptr;        // scratch [pcap][tid_cap]
};

// normal_sums.h: what mpe_calib_batch / mpe_camfit_batch accumulate and mpe_calib_step / mpe_camfit_step read, the same
// at two sizes.  The Levenberg-Marquardt state of the cameras lives on the host (api.hip, csrc/calib_solve.h,
// csrc/camfit_solve.h), behind each family's own opaque type.
struct normal_state {
    int V = 0, max_frames = 0;
    int n_sums = 0, cam_width = 0;  // sums per camera; doubles of a trial camera on the device
    int64_t launches = 0;           // kernels enqueued since create
    double *cams = nullptr;         // [V][cam_width] the trial set
    double *acc = nullptr;          // [V][n_sums] sums of the pass so far
    unsigned long long *n_obs = nullptr, *n_skipped = nullptr;   // [V]
    double *S = nullptr;            // scratch [max_frames][V][n_sums]: the per-frame partials of a call
};
constexpr int CALIB_CAM = 12;       // doubles of a trial camera on the device: E [12]
constexpr int CAMFIT_CAM = 21;      // E [12], dist [5], (fx, fy, cx, cy) widened (exact)
struct mpe_calib_host;
struct mpe_calib_state : normal_state {
    mpe_calib_host *host = nullptr;
};
struct mpe_camfit_host;
struct mpe_camfit_state : normal_state {
    mpe_camfit_host *host = nullptr;
};

// lag.hip: what mpe_lag_batch accumulates and mpe_lag_read / mpe_lag_estimate read.  The pick of the least entry is host
// work (api.hip, csrc/lag_pick.h).
struct mpe_lag_state {
    int V = 0, K = 0, W = 0, sub = 0, pcap = 0, J = 0, pose_f64 = 0, joint_flags = 0, max_frames = 0;
    int64_t launches = 0;           // kernels enqueued since mpe_lag_create
    double *cost = nullptr;         // [V][K] sums of the pass so far
    unsigned long long *ctr = nullptr;   // n_obs [V][K] | n_skipped [V][K] | n_support [V] | n_unsupported [V]
    double *S = nullptr;            // scratch [max_frames][V][K]: the per-frame partials of a call
};

namespace mpe {

// gemm.hip
struct AttnCoef {              // fc2 of a graph-attention layer: also emit a1|a2 (gat2.py:57-58) from the epilogue
    const float *attn_l, *attn_r;   // [heads*out_dim]
    float *a12;                     // [rows][32]: a1[0..15] | a2[0..15]
    int heads, out_dim;
};
// the decode of the MLP output (metrics_from_model.py:281-294) from the epilogue of the last layer's launch: row m of the compacted
// rows is person m - person_off[f] of the frame f with person_off[f] <= m < person_off[f + 1]
struct DecodeEpi {
    const int32_t *person_off;     // [n_frames + 1]
    int n_frames, pcap, n_out;
    float scale;
    float *poses;                  // [n_frames][pcap][n_out]
};
hipError_t launch_linear_sb16(hipStream_t s, const float *A, int lda, const unsigned short *W3, size_t w_plane, int ldw,
                              const float *bias, float *C, int ldc, int m_cap, const int32_t *d_m, int n, int k_pad, bool leaky,
                              float slope, bool f64 = true, const AttnCoef *coef = nullptr, bool *coef_done = nullptr,
                              bool out_half = false,      // out_half (fp16 ft2 rows, configs[4]): tile kernel, fp32-chain launches without LeakyReLU only; hipErrorInvalidValue otherwise
                              int flush_stages = 2,       // f64 launches: K stages per f64 flush (2 = default, 1 = the maximum-accuracy mode)
                              const DecodeEpi *dec = nullptr, bool *dec_done = nullptr);   // the K-split kernel can also store the decoded poses (*dec_done says whether it did)
bool linear_sb16_uses_tile_kernel(int m_cap, int n, bool f64);
int device_cu_count();        // gemm_sb16.hip: CUs of the current device (asked once per device)

// lat.hip: the small-batch ("latency") forms -- the arithmetic of the split-bf16 kernels (same bits), shortest serial depth
bool lat_gemm_available(int k_pad, int n, bool fc2, int out_dim);
hipError_t launch_lat_gemm(hipStream_t s, const unsigned short *Apl, int lda, size_t a_plane, const unsigned short *W3, size_t w_plane, int ldw,
                           const float *bias, float *C, int ldc, unsigned short *Cpl, int ldcp, size_t c_plane, int m, int n, int k_pad, bool fc2,
                           float slope, const float *attn_l, const float *attn_r, float *a12, int out_dim, bool *coef_done = nullptr);
bool lat_gemm_fusable(int k1_pad, int n1, int k2_pad, int n2, int out_dim2);
hipError_t launch_lat_gemm_fused(hipStream_t s, const unsigned short *Apl, int lda, size_t a_plane, const unsigned short *W3, size_t w_plane, int ldw,
                                 const float *bias, int m, int n, float slope, const unsigned short *W3b, size_t w_plane_b, int ldw_b, const float *bias_b,
                                 float *C2, int ldc2, const float *attn_l, const float *attn_r, float *a12);
// ... at batch size from the fp32 rows of the batch path (k_last_fused: persistent grid, the same bits)
hipError_t launch_last_fused(hipStream_t s, const float *A, int lda, const unsigned short *W3, size_t w_plane, int ldw, const float *bias, int m,
                             float slope, const unsigned short *W3b, size_t w_plane_b, int ldw_b, const float *bias_b, float *C2, int ldc2,
                             const float *attn_l, const float *attn_r, float *a12);
// gemm_f64.hip: exact products, f64 accumulation on the f64 matrix pipe (MLP mode 5: the f64-evaluated network, not the fast path; the slope rule is in include/mpe.h)
hipError_t launch_linear_f64(hipStream_t s, const float *A, int lda, const float *W, int ldw, const float *bias, float *C, int ldc,
                             int m_cap, const int32_t *d_m, int n, int k_pad, bool leaky, float slope);
hipError_t launch_linear(hipStream_t s, const float *A, int lda, const float *W, int ldw, const float *bias,
                         float *C, int ldc, int m_cap, const int32_t *d_m, int n, int k_pad, bool leaky,
                         float slope, bool acc64, const int32_t *a_rows = nullptr, const int32_t *c_rows = nullptr,
                         const AttnCoef *coef = nullptr, bool *coef_done = nullptr, bool out_half = false);
// one launch for `n_grp` GEMMs that share the activation / result buffers: group g takes the rows
// row_lists[g * grp_stride + 0 .. grp_count[g]) (device-side counts) and the weights W + g * w_grp_stride
hipError_t launch_linear_grouped(hipStream_t s, const float *A, int lda, const float *W, int ldw, long w_grp_stride,
                                 const float *bias, float *C, int ldc, int m_cap, const int32_t *grp_count, int n_grp,
                                 const int32_t *row_lists, int grp_stride, int n, int k_pad, bool leaky, float slope, bool acc64 = false);
bool linear_uses_tile_kernel(int m_cap, int n);
hipError_t launch_onehot_rows(hipStream_t s, float *rows, int n_rows, int ld, int col);
hipError_t launch_group_heads(hipStream_t s, int n_heads, int V, const int32_t *head_cam, int32_t *cam_count,
                              int32_t *cam_list, int list_stride, bool counts_zeroed = false);

hipError_t launch_linear_bf16(hipStream_t s, const float *A, int lda, const unsigned short *Wb, int ldw,
                              const float *bias, float *C, int ldc, int m_cap, const int32_t *d_m, int n, int k_pad,
                              bool leaky, float slope, int k_lim = 0, bool out_half = false,
                              const int32_t *a_rows = nullptr, const int32_t *c_rows = nullptr);

// gemm_sb16.hip: fp32-accurate nn.Linear on the bf16 MFMA (three bf16 planes per operand, f64 flush every second stage)
hipError_t launch_split_planes(hipStream_t s, const float *w, size_t count, unsigned short *planes);
// gat.hip
hipError_t launch_topology(hipStream_t s, const mpe_batch &b, int V, int32_t *node_off, int32_t *head_frame,
                           int32_t *en_frame, int32_t *en_pair, int max_heads_per_frame, int32_t *status,
                           uint16_t *head_src, int x_deg_cap = 0, int x_m_cap = 0);
// explicit pair lists (mpe_batch::d_en_pair): row stride of the in-edge source table = largest in-degree of a head
inline int explicit_deg_cap(int max_heads_per_frame) { return 2 * max_heads_per_frame; }
// entries of the per-frame in-edge source table of the heads, or 0 when frames of that capacity do not get one
size_t head_src_entries(int max_heads_per_frame, int V);
hipError_t launch_head_features(hipStream_t s, const DevCfg *cfg, const mpe_batch &b, int J, float *feat,
                                int ld_feat, int col0, int stride_cam, bool dense, int32_t *zero_counts = nullptr,
                                int n_zero = 0);
hipError_t launch_attn_coef(hipStream_t s, const float *ft2, int ld, int n_rows, int heads, int out_dim,
                            const float *attn_l, const float *attn_r, float *a12, int ft_half = 0);
struct AggArgs {
    const float *ft2;          // rows of transformed features (fp16 rows when ft_half, reduced precision)
    int ld;                    // row stride in elements of that type
    int ft_half;
    const float *a12;          // [rows][32]: a1[0..15] | a2[0..15]
    int a12_ready;             // a12 already holds this layer's coefficients (fc2 epilogue)
    int heads, out_dim;
    float alpha, out_slope;    // attention LeakyReLU slope; activation applied to the output
    int out_mode;              // 0 = LeakyReLU(out_slope), 1 = sigmoid, 2 = identity
    const float *en_const_ft2; // layer 0: one row shared by all edge-nodes (ft2 holds head rows only)
    const float *en_const_a;   // layer 0: its a1|a2
    float *out;                // [n_nodes][ld_out] (or scores when score_mode)
    int ld_out;
    int score_mode;            // last layer: write out[edge-node index] (and heads to out_heads)
    float *out_heads;
    const float *attn_l, *attn_r;   // [heads*out_dim]: for the kernels that compute a1 | a2 themselves when a12_ready == 0 (general path, small batches)
    unsigned short *out_pl;    // small batches (lat.hip): the output as three bf16 planes [3][rows][ld_out] INSTEAD of fp32 rows
    size_t out_pl_plane;       // plane stride in elements
    int l0_whole_rows;         // layer 0 routed to k_l0_attention (gat_layer_linear): a12 was NOT filled, the kernel computes a1 | a2 itself
};
// layer 0, implicit topology, 40-wide heads, fp32 rows: coefficients + attention in one launch that writes whole rows
bool l0_attention_available(int max_heads_per_frame, int V, int heads, int out_dim);
hipError_t launch_l0_attention(hipStream_t s, const mpe_batch &b, int V, int max_heads_per_frame, const int32_t *node_off,
                               const int32_t *en_pair, const float *attn_l, const float *attn_r, const AggArgs &a);
hipError_t launch_aggregate(hipStream_t s, const mpe_batch &b, int V, int max_heads_per_frame,
                            const int32_t *node_off, const int32_t *head_frame, const int32_t *en_frame,
                            const int32_t *en_pair, const AggArgs &a, const uint16_t *head_src, int x_deg_cap = 0);

bool lat_l0a_available(int J, int l0_ld);
hipError_t launch_lat_l0a(hipStream_t s, const DevCfg *cfg, const mpe_batch &b, int V, int J, int32_t *node_off, int32_t *head_frame,
                          int32_t *en_frame, int32_t *en_pair, uint16_t *head_src, int hmax, int32_t *status, const float *l0_w,
                          long w_cam_stride, int l0_ld, const float *l0_b, int n_out, float *h0, int ld_h0, float alpha);
hipError_t launch_lat_attention(hipStream_t s, const mpe_batch &b, int V, int max_heads_per_frame, const int32_t *node_off,
                                const int32_t *head_frame, const int32_t *en_frame, const int32_t *en_pair, const AggArgs &a,
                                const uint16_t *head_src);
hipError_t launch_gat_attention(hipStream_t s, const mpe_batch &b, int V, int max_heads_per_frame,
                                const int32_t *node_off, const int32_t *head_frame, const int32_t *en_frame,
                                const int32_t *en_pair, const float *attn_l, const float *attn_r, float *a12,
                                const AggArgs &a, int n_rows_ft2, const uint16_t *head_src, int x_deg_cap = 0,
                                int x_m_cap = 0);

// cluster.hip
size_t cluster_keys_per_frame(int max_heads_per_frame);
size_t cluster_scratch_per_frame(int max_heads_per_frame);
hipError_t launch_cluster(hipStream_t s, const DevCfg *cfg, const mpe_batch &b, const int32_t *en_pair,
                          const float *scores, int pcap, int max_heads_per_frame, uint64_t *keys,
                          size_t keys_per_frame, int32_t *scratch, size_t scratch_per_frame,
                          int32_t *persons, int32_t *n_persons);

// the small-batch tail launch (cluster.hip: k_lat_tail): last layer's scores + clustering per frame, every cross-camera pair solved beside it
bool lat_tail_available(int hmax, size_t keys_per_frame);
hipError_t launch_lat_tail(hipStream_t s, const DevCfg *cfg, const mpe_batch &b, int J, const int32_t *en_pair, const int32_t *en_frame,
                           const float *ft2, int ld, const float *a12, float alpha, float out_slope, int out_mode, const int32_t *node_off,
                           float *scores, int pcap, int hmax, size_t keys_per_frame, int32_t *persons, int32_t *n_persons, double *pair_pts);

// pose3d.hip
hipError_t launch_person_scan(hipStream_t s, int n_frames, int pcap, const int32_t *n_persons, int32_t *person_off,
                              int32_t *total);
hipError_t launch_mlp_rows(hipStream_t s, const DevCfg *cfg, int V, int J, const mpe_batch &b,
                           const int32_t *persons, const int32_t *n_persons, const int32_t *person_off, int pcap,
                           float *rows, int ld_rows, uint8_t *valid, int32_t *scan_out = nullptr, int32_t *total_out = nullptr,
                           float *zero_poses = nullptr, int n_out = 0, const double *pair_pts = nullptr, int pair_hmax = 0);

hipError_t launch_triangulate(hipStream_t s, const DevCfg *cfg, int V, int J, const mpe_batch &b,
                              const int32_t *persons, const int32_t *n_persons, int pcap, double *poses,
                              uint8_t *joint_valid, uint32_t out_mask, bool positive_ids_only = false);
hipError_t launch_dlt_pairs(hipStream_t s, const DevCfg *cfg, const double *pts, const int32_t *cams, int n,
                            double *out);
hipError_t launch_decode(hipStream_t s, int n_frames, int pcap, int n_out, float scale, const int32_t *n_persons,
                         const int32_t *person_off, const float *y, int ld_y, float *poses);
int cluster_table_cap(int hmax);

// eval.hip
hipError_t launch_eval(hipStream_t s, const mpe_eval_args &a);

// track.hip
hipError_t track_prepare(int pcap);                  // dynamic-LDS opt-in of the stage kernels for this device
hipError_t launch_track_reset(hipStream_t s, mpe_track_state *st);
hipError_t launch_track(hipStream_t s, mpe_track_state *st, const mpe_track_args &a);

// smooth.hip
hipError_t launch_smooth_reset(hipStream_t s, mpe_smooth_state *st);
hipError_t launch_smooth(hipStream_t s, mpe_smooth_state *st, const mpe_smooth_args &a);

// jsonwrite.hip: *launches counts the kernels the runtime accepted
size_t json_write_scratch_bytes(int64_t n_frames, int64_t pcap, int64_t J);
hipError_t launch_json_write(hipStream_t s, const mpe_json_write_args &a, int64_t *launches);
hipError_t launch_format_f64(hipStream_t s, const double *d_values, int64_t n, char *d_slots, uint8_t *d_len);

// skel.hip
void skel_schedule(const int32_t *bones, int n_bones, std::vector<uint32_t> *table, int *steps_upto);
hipError_t launch_skel_reset(hipStream_t s, mpe_skel_state *st);
hipError_t launch_skel_observe(hipStream_t s, mpe_skel_state *st, const mpe_skel_args &a);
hipError_t launch_skel_update(hipStream_t s, mpe_skel_state *st, int min_samples);
hipError_t launch_skel_fit(hipStream_t s, mpe_skel_state *st, const mpe_skel_args &a);
// relink.hip
hipError_t launch_relink_reset(hipStream_t s, mpe_relink_state *st);
hipError_t launch_relink(hipStream_t s, mpe_relink_state *st, const mpe_relink_args &a);
// skel_refine.hip
int skel_refine_tables(const int32_t *bones, int n_bones, int J, std::vector<uint32_t> *tab);
hipError_t launch_skel_refine(hipStream_t s, const DevCfg *cfg, int V, mpe_skel_state *st, const mpe_batch &b, const mpe_body_refine_args &a);

// track_score.hip
hipError_t launch_track_score_reset(hipStream_t s, mpe_track_score_state *st);
hipError_t launch_track_score(hipStream_t s, mpe_track_score_state *st, const mpe_track_score_args &a);

// reproject.hip
hipError_t launch_reproject(hipStream_t s, const DevCfg *cfg, int V, const mpe_batch &b, const mpe_reproject_args &a);
// refine.hip
hipError_t launch_refine(hipStream_t s, const DevCfg *cfg, int V, const mpe_batch &b, const mpe_refine_args &a);
// posecov.hip
hipError_t launch_posecov(hipStream_t s, const DevCfg *cfg, int V, const mpe_batch &b, const mpe_posecov_args &a);
// regroup.hip
hipError_t launch_regroup(hipStream_t s, const DevCfg *cfg, int V, int min_views, int hmax, int32_t *sticky, const mpe_batch &b,
                          const mpe_regroup_args &a);
// consolidate.hip
hipError_t launch_consolidate(hipStream_t s, const DevCfg *cfg, int V, int hmax, int32_t *sticky, const mpe_batch &b,
                              const mpe_consolidate_args &a);
// calib.hip, camfit.hip (normal_sums.h): one pass onto the state, two launches
hipError_t launch_calib(hipStream_t s, const DevCfg *cfg, normal_state *st, const mpe_batch &b, const mpe_calib_args &a);
hipError_t launch_camfit(hipStream_t s, const DevCfg *cfg, normal_state *st, const mpe_batch &b, const mpe_calib_args &a);
// lag.hip
size_t lag_counter_words(int V, int K);
hipError_t launch_lag(hipStream_t s, const DevCfg *cfg, mpe_lag_state *st, const mpe_batch &b, const mpe_lag_args &a);
hipError_t launch_lag_reset(hipStream_t s, mpe_lag_state *st);

// refine_timed.hip
hipError_t launch_refine_timed(hipStream_t s, const DevCfg *cfg, int V, const mpe_batch &b, const mpe_refine_timed_args &a);
// geom.hip: en_pair = the context's pair table (launch_topology); ray_table only when geom_needs_table()
constexpr size_t GEOM_LDS_BYTES = 48 * 1024;     // head records of a frame staged in LDS up to this (three 256-thread workgroups per CU's 160 KiB)
bool geom_needs_table(int max_heads_per_frame, int J);
size_t geom_table_doubles(int max_heads, int J);
hipError_t launch_geom(hipStream_t s, const DevCfg *cfg, int V, int J, const mpe_batch &b, const int32_t *en_pair, int max_heads_per_frame,
                       int x_m_cap, const mpe_geom_args &a, float *scores, double *ray_table);
// partition.hip
hipError_t launch_partition_labels(hipStream_t s, int V, const mpe_batch &b, const mpe_partition_labels_args &a);
hipError_t launch_group_bodies(hipStream_t s, const mpe_group_bodies_args &a);
hipError_t launch_partition_scores(hipStream_t s, const mpe_partition_scores_args &a, const double *log_table, int n_log);
hipError_t launch_residual_stats(hipStream_t s, int V, const mpe_residual_stats_args &a, ResidualState *state, uint32_t *hist,
                                 double *partial);

}  // namespace mpe
