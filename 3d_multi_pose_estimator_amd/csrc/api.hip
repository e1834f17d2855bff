// C-ABI entry points of libmpe_hip.so (see include/mpe.h).  Host-side orchestration only:
// argument checks, workspace, weight upload, and the stream-ordered launch sequences.
#include <cmath>
#include <cstdarg>
#include <new>
#include <cstdio>
#include <cstdlib>
#include <cstring>

#include "mpe_internal.h"
#include "assign_int.h"
#include "relink_config.h"
#include "fmt_double.h"               // MPE_FMT_MAX_LEN

using namespace mpe;

namespace {

int fail(mpe_ctx *ctx, int code, const char *fmt, ...) {
    char buf[512];
    va_list ap;
    va_start(ap, fmt);
    vsnprintf(buf, sizeof buf, fmt, ap);
    va_end(ap);
    if (ctx) ctx->err = buf;
    return code;
}

#define HIPCHK(ctx, expr)                                                                     \
    do {                                                                                      \
        hipError_t e_ = (expr);                                                               \
        if (e_ != hipSuccess)                                                                 \
            return fail(ctx, MPE_ERR_HIP, "%s failed: %s (%s:%d)", #expr, hipGetErrorString(e_), __FILE__, __LINE__); \
    } while (0)

// Every entry point runs on the device the context was created on (one process per GPU is the
// deployment, but a second context on another device in the same process must also work).
struct DeviceGuard {
    int prev = -1;
    explicit DeviceGuard(const mpe_ctx *ctx) {
        if (!ctx) return;
        int cur = -1;
        if (hipGetDevice(&cur) == hipSuccess && cur != ctx->device) {
            prev = cur;
            (void)hipSetDevice(ctx->device);
        }
    }
    ~DeviceGuard() {
        if (prev >= 0) (void)hipSetDevice(prev);
    }
};

// frees p if the context owns it; says whether it did
bool dev_free(mpe_ctx *ctx, void *p) {
    if (!p) return false;
    for (size_t i = 0; i < ctx->owned.size(); ++i)
        if (ctx->owned[i] == p) {
            (void)hipFree(p);
            ctx->owned.erase(ctx->owned.begin() + i);
            return true;
        }
    return false;
}

template <typename T>
int dev_alloc(mpe_ctx *ctx, T **p, size_t count, bool zero = true) {
    void *q = nullptr;
    size_t bytes = count * sizeof(T);
    if (bytes == 0) bytes = sizeof(T);
    hipError_t e = hipMalloc(&q, bytes);
    if (e != hipSuccess) return fail(ctx, MPE_ERR_NOMEM, "hipMalloc(%zu) failed: %s", bytes, hipGetErrorString(e));
    if (zero) {
        e = hipMemset(q, 0, bytes);
        if (e != hipSuccess) return fail(ctx, MPE_ERR_HIP, "hipMemset failed: %s", hipGetErrorString(e));
    }
    ctx->owned.push_back(q);
    *p = static_cast<T *>(q);
    return MPE_OK;
}

// ---- the state objects of the sequence stages (mpe_track_*, mpe_relink_*, mpe_smooth_*, mpe_skel_*, mpe_track_score_*, mpe_calib_*) ----

// What every *_create does around its own part.  fill(st) gets the zeroed host struct: it checks the sizes first (a
// refusal there comes before anything is allocated on the device), sets the fields and allocates.  When it fails,
// destroy frees what it got as far as it came and the message of the failure stays the last error.
template <typename S, typename Fill>
int create_state(mpe_ctx *ctx, const char *who, S **out, int (*destroy)(mpe_ctx *, S *), Fill fill) {
    if (!ctx) return MPE_ERR_INVALID;
    if (!out) return fail(ctx, MPE_ERR_INVALID, "%s: NULL argument", who);
    *out = nullptr;
    DeviceGuard dg(ctx);
    S *st = new (std::nothrow) S();
    if (!st) return fail(ctx, MPE_ERR_NOMEM, "%s: out of memory", who);
    const int rc = fill(st);
    if (rc) {
        const std::string why = ctx->err;
        destroy(ctx, st);
        ctx->err = why;
        return rc;
    }
    *out = st;
    return MPE_OK;
}

template <typename S>
int reset_state(mpe_ctx *ctx, const char *who, void *stream, S *st, hipError_t (*launch_reset)(hipStream_t, S *)) {
    if (!ctx) return MPE_ERR_INVALID;
    if (!st) return fail(ctx, MPE_ERR_INVALID, "%s: NULL state", who);
    DeviceGuard dg(ctx);
    HIPCHK(ctx, launch_reset(static_cast<hipStream_t>(stream), st));
    return MPE_OK;
}

template <typename S>
int state_launches(mpe_ctx *ctx, const char *who, const S *st, int64_t *n) {
    if (!ctx) return MPE_ERR_INVALID;
    if (!st || !n) return fail(ctx, MPE_ERR_INVALID, "%s: NULL argument", who);
    *n = st->launches;
    return MPE_OK;
}

// What the batch calls on pose rows (track, relink, smooth, skel observe and fit) check alike: the sizes and the pose type the
// state was made for, the frame count and the flag mode -> MPE_OK with *run = false for a call without frames.
template <typename S, typename A>
int check_pose_rows(mpe_ctx *ctx, const char *who, const S *st, const A *a, bool *run) {
    *run = false;
    if (a->pcap != st->pcap || a->n_joints != st->J || a->pose_f64 != st->pose_f64)
        return fail(ctx, MPE_ERR_INVALID, "%s: pcap %d / joints %d / pose_f64 %d, the state was made for %d / %d / %d", who, a->pcap, a->n_joints,
                    a->pose_f64, st->pcap, st->J, st->pose_f64);
    if (a->n_frames < 0 || (a->joint_flags & ~1))
        return fail(ctx, MPE_ERR_INVALID, "%s: n_frames %d / joint_flags %d", who, a->n_frames, a->joint_flags);
    if (a->n_frames > (1 << 23)) return fail(ctx, MPE_ERR_CAPACITY, "%s: %d frames over 2^23 per call", who, a->n_frames);
    *run = a->n_frames > 0;
    return MPE_OK;
}

void free_linear(mpe_ctx *ctx, Linear *L) {
    dev_free(ctx, L->w);
    dev_free(ctx, L->b);
    dev_free(ctx, L->w16);
    dev_free(ctx, L->w3);
    *L = Linear();
}

int upload_linear(mpe_ctx *ctx, const float *w, const float *b, int out_dim, int in_dim, Linear *L) {
    if (!w || out_dim <= 0 || in_dim <= 0) return fail(ctx, MPE_ERR_INVALID, "bad linear layer %dx%d", out_dim, in_dim);
    free_linear(ctx, L);                   // a layer set twice does not keep its first copies
    L->in_dim = in_dim;
    L->out_dim = out_dim;
    L->ldw = round_up(in_dim, LD_ALIGN);
    const int rows = weight_rows(out_dim);
    int rc = dev_alloc(ctx, &L->w, (size_t)rows * L->ldw);
    if (rc) return rc;
    rc = dev_alloc(ctx, &L->b, (size_t)rows);
    if (rc) return rc;
    HIPCHK(ctx, hipMemcpy2D(L->w, (size_t)L->ldw * sizeof(float), w, (size_t)in_dim * sizeof(float),
                            (size_t)in_dim * sizeof(float), out_dim, hipMemcpyHostToDevice));
    if (b) HIPCHK(ctx, hipMemcpy(L->b, b, (size_t)out_dim * sizeof(float), hipMemcpyHostToDevice));
    return MPE_OK;
}

int check_batch(mpe_ctx *ctx, const mpe_batch *b) {
    if (!ctx) return MPE_ERR_INVALID;
    // every batch call starts here, and every batch call forgets the pairs mpe_match_batch left for mpe_mlp3d_batch: whatever this
    // call is, the next mpe_mlp3d_batch is no longer "the call right after the matching of its batch" (pair_handoff.h)
    ctx->handoff.forget();
    if (!b) return fail(ctx, MPE_ERR_INVALID, "batch is NULL");
    if (b->n_frames < 0 || b->n_heads < 0 || b->n_edge_nodes < 0) return fail(ctx, MPE_ERR_INVALID, "negative batch size");
    if (b->n_frames > ctx->cfg.max_frames || b->n_heads > ctx->cfg.max_heads ||
        b->n_edge_nodes > ctx->cfg.max_edge_nodes)
        return fail(ctx, MPE_ERR_CAPACITY, "batch (%d frames, %d heads, %d edge-nodes) exceeds capacity (%d, %d, %d)",
                    b->n_frames, b->n_heads, b->n_edge_nodes, ctx->cfg.max_frames, ctx->cfg.max_heads,
                    ctx->cfg.max_edge_nodes);
    if (b->n_frames > 0 && (!b->d_frame_head_off || !b->d_frame_en_off || (!b->d_en_pair && (!b->d_slot_cam || !b->d_slot_n))))
        return fail(ctx, MPE_ERR_INVALID, "batch offset tables missing");
    if (b->d_en_pair && ctx->x_m_cap <= 0)
        return fail(ctx, MPE_ERR_UNSUPPORTED, "explicit edge-node lists need max_heads_per_frame <= 1024 and node ids that fit 16 bits "
                    "(max_heads_per_frame = %d)", ctx->cfg.max_heads_per_frame);
    if (b->n_heads > 0 && (!b->d_head_cam || !b->d_joint_mask || !b->d_tri_mask || !b->d_xy || !b->d_vp))
        return fail(ctx, MPE_ERR_INVALID, "batch skeleton arrays missing");
    return MPE_OK;
}

// What the geometry calls on a batch's person rows (reproject, refine, regroup, consolidate, calib, body refine) check alike,
// after check_batch: the frames of the batch, the joints of the context, pcap and the two modes -> MPE_OK with *run = false
// for a call without frames.  takes_d_frame: the entry point has a d_frame list, and with one given (d_frame) the rows
// name their frames and need not be as many as the batch has.
template <typename A>
int check_batch_rows(mpe_ctx *ctx, const char *who, const mpe_batch *b, const A *a, bool *run, bool takes_d_frame = false,
                     const int32_t *d_frame = nullptr) {
    *run = false;
    if (!d_frame && a->n_frames != b->n_frames)
        return fail(ctx, MPE_ERR_INVALID, "%s: n_frames %d%s, the batch has %d frames", who, a->n_frames, takes_d_frame ? " without d_frame" : "",
                    b->n_frames);
    if (a->n_joints != ctx->cfg.n_joints)
        return fail(ctx, MPE_ERR_INVALID, "%s: %d joints, the context has %d", who, a->n_joints, ctx->cfg.n_joints);
    if (a->pcap < 1) return fail(ctx, MPE_ERR_INVALID, "%s: pcap %d must be at least 1", who, a->pcap);
    if ((a->pose_f64 & ~1) || (a->joint_flags & ~1))
        return fail(ctx, MPE_ERR_INVALID, "%s: pose_f64 %d and joint_flags %d must be 0 or 1", who, a->pose_f64, a->joint_flags);
    *run = a->n_frames > 0;
    return MPE_OK;
}

// the four arrays every one of them reads, tested where a call with frames has passed its value checks
template <typename A>
bool row_inputs_missing(const A *a) { return !a->d_persons || !a->d_n_persons || !a->d_poses || !a->d_flags; }

struct GemmProf {
    mpe_ctx *ctx;
    hipStream_t s;
    bool on;
    size_t idx;
    GemmProf(mpe_ctx *c, hipStream_t st, double flop, int dev_m_n, int dev_m_k, int kind = 0) : ctx(c), s(st), on(false), idx(0) {
        if (!c->profiling) return;
        if (c->prof_used == c->prof.size()) {
            ProfileRec r{};
            if (hipEventCreate(&r.start) != hipSuccess || hipEventCreate(&r.stop) != hipSuccess) return;
            c->prof.push_back(r);
        }
        idx = c->prof_used++;
        c->prof[idx].flop = flop;
        c->prof[idx].dev_n = dev_m_n;
        c->prof[idx].dev_k = dev_m_k;
        c->prof[idx].kind = kind;
        on = true;
        (void)hipEventRecord(c->prof[idx].start, s);
    }
    ~GemmProf() {
        if (on) (void)hipEventRecord(ctx->prof[idx].stop, s);
    }
};

// MPE_LATENCY_PATH=0: small batches through the batch path's own small-batch kernels (read per call: tests toggle it)
bool latency_path_on() {
    const char *e = getenv("MPE_LATENCY_PATH");
    return !(e && e[0] == '0');
}

unsigned short f32_to_bf16(float f) {
    uint32_t u;
    memcpy(&u, &f, 4);
    if ((u & 0x7F800000u) == 0x7F800000u && (u & 0x007FFFFFu)) return (unsigned short)((u >> 16) | 0x40);   // NaN stays NaN
    u += 0x7FFFu + ((u >> 16) & 1u);          // round to nearest even
    return (unsigned short)(u >> 16);
}

int ensure_bf16_weights(mpe_ctx *ctx, Linear *L) {
    if (L->w16) return MPE_OK;
    const int rows = weight_rows(L->out_dim);
    L->ldw16 = round_up(L->in_dim, 128);
    std::vector<float> w((size_t)rows * L->ldw);
    HIPCHK(ctx, hipMemcpy(w.data(), L->w, w.size() * sizeof(float), hipMemcpyDeviceToHost));
    std::vector<unsigned short> wb((size_t)rows * L->ldw16, 0);
    for (int r = 0; r < rows; ++r)
        for (int k = 0; k < L->in_dim; ++k) wb[(size_t)r * L->ldw16 + k] = f32_to_bf16(w[(size_t)r * L->ldw + k]);
    int rc = dev_alloc(ctx, &L->w16, wb.size(), false);
    if (rc) return rc;
    HIPCHK(ctx, hipMemcpy(L->w16, wb.data(), wb.size() * sizeof(unsigned short), hipMemcpyHostToDevice));
    return MPE_OK;
}

// the three bf16 planes of a weight matrix (split on the device from the padded fp32 copy, stream-ordered)
int ensure_split_weights(mpe_ctx *ctx, hipStream_t s, Linear *L) {
    if (L->w3) return MPE_OK;
    const size_t count = plane_elems(*L);
    int rc = dev_alloc(ctx, &L->w3, 3 * count, false);
    if (rc) return rc;
    HIPCHK(ctx, launch_split_planes(s, L->w, count, L->w3));
    return MPE_OK;
}

// One nn.Linear launch, whatever its form: act(A W^T + b) -> C
struct GemmCall {
    const float *A;
    int lda;
    float *C;
    int ldc;
    int m;
    const int32_t *d_m;                    // optional device-side row count (<= m)
    bool leaky;
    float slope;
    const int32_t *a_rows = nullptr, *c_rows = nullptr;      // gathered rows (fp32 MFMA and plain bf16 forms)
    double flop_override = -1.0;           // >= 0: the profile record's FLOP, for a launch whose row count the host knows better
    const AttnCoef *coef = nullptr;        // fc2 of a GAT layer: a1 | a2 from the epilogue where the launch has one (*coef_done)
    bool *coef_done = nullptr;
    bool out_half = false;                 // C is the same buffer seen as fp16 rows, ldc in halves
    int flush_stages = 2;                  // SB16_F64: K stages per f64 flush
    const DecodeEpi *dec = nullptr;        // SB16_F64: the decoded poses from the epilogue where the launch has one (*dec_done)
    bool *dec_done = nullptr;
    int bf16_min_ld = 0;                   // BF16: the launch reads this many columns of a row (whole 128-deep stages); 0 = L.ldw, as every other form
};

// The one place an nn.Linear is launched from (which form: gemm_form.h).  The order matters: nothing is made for an empty launch.
int gemm(mpe_ctx *ctx, hipStream_t s, GemmForm form, Linear &L, const GemmCall &c) {
    if (c.coef_done) *c.coef_done = false;
    if (c.dec_done) *c.dec_done = false;
    if (c.m <= 0) return MPE_OK;
    const bool sb16 = form == GemmForm::SB16 || form == GemmForm::SB16_F64, bf16 = form == GemmForm::BF16;
    int rc;
    if (sb16 && (rc = ensure_split_weights(ctx, s, &L))) return rc;
    if (bf16 && (rc = ensure_bf16_weights(ctx, &L))) return rc;
    // Every form reads L.ldw columns of an activation row.  The plain bf16 kernel works in 128-deep stages and zero-fills what lies
    // beyond the columns it is told to read: the MLP's strides are multiples of 128 and its launches read whole stages (L.ldw16),
    // the GAT's act_ld is a multiple of 32, not of 128, so its launches stop at L.ldw.
    const bool whole_stages = bf16 && c.bf16_min_ld;
    if (whole_stages && c.lda < c.bf16_min_ld) return fail(ctx, MPE_ERR_INVALID, "bf16 GEMM needs an input stride >= %d", c.bf16_min_ld);
    if (!whole_stages && c.lda < L.ldw) return fail(ctx, MPE_ERR_INVALID, "activation stride %d < padded K %d", c.lda, L.ldw);
    // the profile record: FLOP known on the host, or 2 * (device-side row count) * dev_n * dev_k
    const bool host_m = !c.d_m || c.flop_override >= 0.0;
    const double flop = c.flop_override >= 0.0 ? c.flop_override : c.d_m ? 0.0 : 2.0 * c.m * (double)L.out_dim * L.in_dim;
    const int kind = sb16 ? 1 : bf16 ? 2 : form == GemmForm::F64MM ? 3 : 0;
    GemmProf gp(ctx, s, flop, host_m ? 0 : L.out_dim, host_m ? 0 : L.in_dim, kind);
    switch (form) {
    case GemmForm::F32:
    case GemmForm::F32_ACC64:
        HIPCHK(ctx, launch_linear(s, c.A, c.lda, L.w, L.ldw, L.b, c.C, c.ldc, c.m, c.d_m, L.out_dim, L.ldw, c.leaky, c.slope,
                                  form == GemmForm::F32_ACC64, c.a_rows, c.c_rows, c.coef, c.coef_done, c.out_half));
        break;
    case GemmForm::SB16:
    case GemmForm::SB16_F64: {
        const bool f64 = form == GemmForm::SB16_F64;           // (the f64-sum kernels have no coefficient epilogue)
        HIPCHK(ctx, launch_linear_sb16(s, c.A, c.lda, L.w3, plane_elems(L), L.ldw, L.b, c.C, c.ldc, c.m, c.d_m, L.out_dim, L.ldw, c.leaky, c.slope,
                                       f64, f64 ? nullptr : c.coef, c.coef_done, c.out_half, c.flush_stages, c.dec, c.dec_done));
        break;
    }
    case GemmForm::BF16:
        HIPCHK(ctx, launch_linear_bf16(s, c.A, c.lda, L.w16, L.ldw16, L.b, c.C, c.ldc, c.m, c.d_m, L.out_dim, L.ldw16, c.leaky, c.slope,
                                       whole_stages ? c.bf16_min_ld : L.ldw, c.out_half, c.a_rows, c.c_rows));
        break;
    case GemmForm::F64MM:
        HIPCHK(ctx, launch_linear_f64(s, c.A, c.lda, L.w, L.ldw, L.b, c.C, c.ldc, c.m, c.d_m, L.out_dim, L.ldw, c.leaky, c.slope));
        break;
    }
    return MPE_OK;
}

// GEMM of a GAT layer, in the form the precision mode and the launch's shape select (gemm_form.h: gat_gemm_form)
int gat_linear(mpe_ctx *ctx, hipStream_t s, const float *A, int lda, Linear &L, float *C, int ldc, int m,
               const int32_t *d_m, bool leaky, float slope, bool out_half, const int32_t *a_rows = nullptr,
               const int32_t *c_rows = nullptr, double flop_override = -1.0, const AttnCoef *coef = nullptr,
               bool *coef_done = nullptr) {
    static const int mink = getenv("MPE_GAT_ACC64_MINK") ? atoi(getenv("MPE_GAT_ACC64_MINK")) : 512;
    GatGemmQuery q;
    q.gat_split = ctx->gat_split;
    q.gat_reduced = ctx->gat_reduced;
    q.gat_acc64 = ctx->gat_acc64;
    q.acc64_mink = mink;
    q.in_dim = L.in_dim;
    q.out_half = out_half;
    q.leaky = leaky;
    q.gathered = a_rows || c_rows;
    q.l0_view = L.w == ctx->l0_w;
    q.is_l0_fc2 = &L == &ctx->gat[0].fc2;
    q.sb16_tile = out_half && linear_sb16_uses_tile_kernel(m, L.out_dim, false);       // (asked only where it decides)
    return gemm(ctx, s, gat_gemm_form(q), L, {A, lda, C, ldc, m, d_m, leaky, slope, a_rows, c_rows, flop_override, coef, coef_done, out_half});
}

void drop_gat_workspace(mpe_ctx *ctx) {
    float **bufs[] = {&ctx->x0, &ctx->h0, &ctx->xdense, &ctx->hdense, &ctx->act[0], &ctx->act[1], &ctx->act[2],
                      &ctx->a12, &ctx->en0_ft2, &ctx->en0_a, &ctx->xc};
    for (float **p : bufs) {
        dev_free(ctx, *p);
        *p = nullptr;
    }
    dev_free(ctx, ctx->cam_count);
    dev_free(ctx, ctx->cam_list);
    ctx->cam_count = ctx->cam_list = nullptr;
    for (int i = 0; i < 2; ++i) {
        dev_free(ctx, ctx->gat_pl[i]);
        ctx->gat_pl[i] = nullptr;
    }
    for (int c = 0; c < MPE_MAX_CAMERAS; ++c) {
        dev_free(ctx, ctx->l0_fc1[c].w16);          // w / b are views into l0_w / l0_b
        ctx->l0_fc1[c] = Linear();
    }
    dev_free(ctx, ctx->l0_w);
    dev_free(ctx, ctx->l0_b);
    ctx->l0_w = ctx->l0_b = nullptr;
    ctx->en0_ready = false;
    ctx->gat_ws_ready = false;
}

int ensure_gat_workspace(mpe_ctx *ctx) {
    if (ctx->gat_ws_ready) return MPE_OK;
    drop_gat_workspace(ctx);               // leftovers of an attempt that failed half way
    for (int l = 0; l < ctx->gat_layers; ++l)
        if (!ctx->gat_ready[l]) return fail(ctx, MPE_ERR_STATE, "GAT layer %d has no weights", l);
    if (ctx->gat_layers <= 0) return fail(ctx, MPE_ERR_STATE, "GAT parameters not set");
    const int V = ctx->cfg.n_cameras, J = ctx->cfg.n_joints;
    const int F = 2 + V * J * 10;
    if (ctx->gat[0].in_dim != F)
        return fail(ctx, MPE_ERR_INVALID, "GAT input width %d != 2 + V*J*10 = %d", ctx->gat[0].in_dim, F);
    ctx->feat_ld = round_up(F, LD_ALIGN);
    int widest = 0;
    for (int l = 0; l < ctx->gat_layers; ++l) {
        const GatLayer &g = ctx->gat[l];
        if (l > 0 && g.in_dim != ctx->gat[l - 1].heads * ctx->gat[l - 1].out_dim)
            return fail(ctx, MPE_ERR_INVALID, "GAT layer %d input width mismatch", l);
        if (g.heads > 16) return fail(ctx, MPE_ERR_INVALID, "at most 16 attention heads supported");
        // the last layer's attention stage writes one score per node (agg_scores_out: row stride 1, column 0 only)
        if (l == ctx->gat_layers - 1 && (g.heads != 1 || g.out_dim != 1))
            return fail(ctx, MPE_ERR_INVALID, "the last GAT layer must have 1 head x 1 output (it has %d x %d)", g.heads, g.out_dim);
        if (l > 0) widest = widest > g.in_dim ? widest : g.in_dim;
        widest = widest > g.heads * g.out_dim ? widest : g.heads * g.out_dim;
    }
    ctx->act_ld = round_up(widest, LD_ALIGN);
    int rc;
    if ((rc = dev_alloc(ctx, &ctx->x0, (size_t)ctx->cfg.max_heads * ctx->feat_ld))) return rc;
    if ((rc = dev_alloc(ctx, &ctx->h0, (size_t)ctx->cfg.max_heads * ctx->feat_ld))) return rc;
    for (int i = 0; i < 3; ++i)
        if ((rc = dev_alloc(ctx, &ctx->act[i], (size_t)ctx->max_nodes * ctx->act_ld))) return rc;
    if ((rc = dev_alloc(ctx, &ctx->a12, (size_t)ctx->max_nodes * 32))) return rc;
    // layer-0 constants of the edge-nodes: every edge-node row is the one-hot e_1, so
    // fc1(e_1) = W1[:,1] + b1 and everything downstream of it is a model constant.
    const GatLayer &g0 = ctx->gat[0];
    std::vector<float> w1((size_t)g0.in_dim * g0.fc1.ldw), b1(g0.in_dim), c1(ctx->feat_ld, 0.f);
    HIPCHK(ctx, hipMemcpy(w1.data(), g0.fc1.w, w1.size() * sizeof(float), hipMemcpyDeviceToHost));
    HIPCHK(ctx, hipMemcpy(b1.data(), g0.fc1.b, b1.size() * sizeof(float), hipMemcpyDeviceToHost));
    for (int n = 0; n < g0.in_dim; ++n) {
        const float v = w1[(size_t)n * g0.fc1.ldw + 1] + b1[n];
        c1[n] = v > 0.f ? v : v * ctx->gat_alpha;
    }
    float *d_c1 = nullptr;
    if ((rc = dev_alloc(ctx, &d_c1, (size_t)ctx->feat_ld))) return rc;
    struct Tmp {                           // the staging row is only needed inside this function
        mpe_ctx *c;
        float *p;
        ~Tmp() { dev_free(c, p); }
    } tmp{ctx, d_c1};
    if ((rc = dev_alloc(ctx, &ctx->en0_ft2, (size_t)ctx->act_ld))) return rc;
    if ((rc = dev_alloc(ctx, &ctx->en0_a, 32))) return rc;
    HIPCHK(ctx, hipMemcpy(d_c1, c1.data(), c1.size() * sizeof(float), hipMemcpyHostToDevice));
    const bool was = ctx->profiling;
    ctx->profiling = false;
    rc = gemm(ctx, nullptr, GemmForm::F32, ctx->gat[0].fc2, {d_c1, ctx->feat_ld, ctx->en0_ft2, ctx->act_ld, 1, nullptr, false, 0.f});
    ctx->profiling = was;
    if (rc) return rc;
    HIPCHK(ctx, launch_attn_coef(nullptr, ctx->en0_ft2, ctx->act_ld, 1, g0.heads, g0.out_dim, g0.attn_l, g0.attn_r,
                                 ctx->en0_a));
    HIPCHK(ctx, hipDeviceSynchronize());
    ctx->en0_ready = true;
    // layer-0 fc1 grouped by camera: a head row is e_0 plus the J*10 block of its own camera,
    // so fc1(row) = W1[:, block_c] . feat + (b1 + W1[:,0]); K shrinks from F to J*10.
    {
        const int blk = J * 10;
        ctx->l0_ld = round_up(blk, LD_ALIGN);
        if ((rc = dev_alloc(ctx, &ctx->xc, (size_t)ctx->cfg.max_heads * ctx->l0_ld))) return rc;
        if ((rc = dev_alloc(ctx, &ctx->cam_count, (size_t)V))) return rc;
        if ((rc = dev_alloc(ctx, &ctx->cam_list, (size_t)V * ctx->cfg.max_heads))) return rc;
        // the V per-camera matrices live in ONE allocation at a constant stride so that a single
        // grouped launch can address them (launch_linear_grouped); l0_fc1[c] are views into it
        const int rows = weight_rows(g0.in_dim);
        const size_t per = (size_t)rows * ctx->l0_ld;
        if ((rc = dev_alloc(ctx, &ctx->l0_w, per * V))) return rc;
        if ((rc = dev_alloc(ctx, &ctx->l0_b, (size_t)rows))) return rc;
        std::vector<float> wc((size_t)g0.in_dim * blk), bc(g0.in_dim);
        for (int n = 0; n < g0.in_dim; ++n) bc[n] = b1[n] + w1[(size_t)n * g0.fc1.ldw + 0];
        HIPCHK(ctx, hipMemcpy(ctx->l0_b, bc.data(), bc.size() * sizeof(float), hipMemcpyHostToDevice));
        for (int c = 0; c < V; ++c) {
            for (int n = 0; n < g0.in_dim; ++n)
                memcpy(&wc[(size_t)n * blk], &w1[(size_t)n * g0.fc1.ldw + 2 + c * blk], blk * sizeof(float));
            Linear &L = ctx->l0_fc1[c];
            L = Linear();
            L.w = ctx->l0_w + per * c;
            L.b = ctx->l0_b;
            L.in_dim = blk;
            L.out_dim = g0.in_dim;
            L.ldw = ctx->l0_ld;
            HIPCHK(ctx, hipMemcpy2D(L.w, (size_t)L.ldw * sizeof(float), wc.data(), (size_t)blk * sizeof(float),
                                    (size_t)blk * sizeof(float), g0.in_dim, hipMemcpyHostToDevice));
        }
        // K shrinks from F to J*10 (exact: the skipped products are zeros), one launch for all cameras
        ctx->l0_grouped = true;
        if (const char *e = getenv("MPE_L0_GROUPED")) ctx->l0_grouped = atoi(e) != 0;
    }
    ctx->gat_ws_ready = true;              // last step: a failure above leaves the flag false and is retried
    return MPE_OK;
}

// caller-provided dense rows of layer 0 and their fc1 output (the API mirrors only: allocated at first use)
int ensure_dense_workspace(mpe_ctx *ctx) {
    if (ctx->xdense) return MPE_OK;
    int rc = dev_alloc(ctx, &ctx->xdense, (size_t)ctx->max_nodes * ctx->feat_ld);
    if (rc) return rc;
    return dev_alloc(ctx, &ctx->hdense, (size_t)ctx->max_nodes * ctx->feat_ld);
}

int ensure_mlp_workspace(mpe_ctx *ctx) {
    if (ctx->mlp_ws_ready) return MPE_OK;
    float **bufs[] = {&ctx->mlp_rows, &ctx->mlp_act[0], &ctx->mlp_act[1]};
    for (float **p : bufs) {
        dev_free(ctx, *p);
        *p = nullptr;
    }
    if (ctx->mlp_layers <= 0) return fail(ctx, MPE_ERR_STATE, "MLP parameters not set");
    for (int l = 0; l < ctx->mlp_layers; ++l)
        if (!ctx->mlp_ready[l]) return fail(ctx, MPE_ERR_STATE, "MLP layer %d has no weights", l);
    const int V = ctx->cfg.n_cameras, J = ctx->cfg.n_joints, npj = ctx->cfg.numbers_per_joint;
    if (ctx->mlp[0].in_dim != V * J * npj)
        return fail(ctx, MPE_ERR_INVALID, "MLP input width %d != V*J*numbers_per_joint = %d", ctx->mlp[0].in_dim,
                    V * J * npj);
    int widest = 0;
    for (int l = 0; l < ctx->mlp_layers; ++l) {
        if (l > 0 && ctx->mlp[l].in_dim != ctx->mlp[l - 1].out_dim)
            return fail(ctx, MPE_ERR_INVALID, "MLP layer %d input width mismatch", l);
        widest = widest > ctx->mlp[l].out_dim ? widest : ctx->mlp[l].out_dim;
    }
    ctx->mlp_ld_in = round_up(ctx->mlp[0].in_dim, 128);       // 128: K stage of the bf16 variant
    ctx->mlp_ld_hidden = round_up(widest, 128);
    const size_t rows = (size_t)ctx->cfg.max_frames * ctx->cfg.max_persons_per_frame;
    int rc;
    if ((rc = dev_alloc(ctx, &ctx->mlp_rows, rows * ctx->mlp_ld_in))) return rc;
    for (int i = 0; i < 2; ++i)
        if ((rc = dev_alloc(ctx, &ctx->mlp_act[i], rows * ctx->mlp_ld_hidden))) return rc;
    ctx->mlp_ws_ready = true;
    return MPE_OK;
}

// Where the input rows of a GAT layer come from
enum GatInput {
    GAT_IN_IMPLICIT,   // layer 0, production: head rows featurised on the device, edge-node rows constant
    GAT_IN_DENSE0,     // layer 0, caller-provided dense rows already copied into ctx->xdense
    GAT_IN_ACT         // layer > 0: rows in ctx->act[0]
};

// Does the last layer take the fused launch (lat.hip: k_last_fused)?  The deployed shapes in the default precision, and none of the
// cross-check switches that ask for the batch path's own kernels (the list of lat_gat_ok).
static bool last_layer_fusable(const mpe_ctx *ctx, const GatLayer &g) {
    if (!ctx->gat_split || ctx->gat_acc64 || ctx->gat_reduced || ctx->gat_attn_fp16) return false;
    if (getenv("MPE_NO_COEF_EPILOGUE") || getenv("MPE_GAT_ACC64_MINK") || getenv("MPE_SKINNY_WAVES") || getenv("MPE_GEMM_NARROW")) return false;
    return lat_gemm_fusable(g.fc1.ldw, g.in_dim, g.fc2.ldw, g.heads * g.out_dim, g.out_dim) && ctx->act_ld >= g.fc1.ldw;
}

// fc1 -> LeakyReLU(alpha) -> fc2 of layer l (gat2.py:53-55): leaves ft2 in a->ft2 / n_rows_ft2
// fuse_last: the caller is the production route (device-featurised rows) and lets the last layer take the fused launch
// clear_fc1_pad: the caller is a stage entry point (one layer on caller rows), see the GAT_IN_ACT branch
int gat_layer_linear(mpe_ctx *ctx, hipStream_t s, const mpe_batch *b, int l, GatInput in, AggArgs *a, int *n_rows_ft2, bool fuse_last = false,
                     bool clear_fc1_pad = false) {
    GatLayer &g = ctx->gat[l];
    const int V = ctx->cfg.n_cameras, J = ctx->cfg.n_joints;
    const int n_nodes = b->n_heads + b->n_edge_nodes;
    const bool red = ctx->gat_reduced;
    const bool half_rows = red || ctx->gat_attn_fp16;        // ft2 as fp16 rows for the attention stage
    const int ld_ft = half_rows ? 2 * ctx->act_ld : ctx->act_ld;   // fp16 rows keep the byte stride of the fp32 rows
    int rc;
    // fc2 also emits the attention coefficients a1|a2 from its epilogue when the layer's shape allows
    const AttnCoef coef{g.attn_l, g.attn_r, ctx->a12, g.heads, g.out_dim};
    const bool no_epi = getenv("MPE_NO_COEF_EPILOGUE") != nullptr;           // read per call: tests toggle it
    const AttnCoef *cp = no_epi ? nullptr : &coef;
    bool done = false;
    if (in == GAT_IN_DENSE0) {
        if ((rc = gat_linear(ctx, s, ctx->xdense, ctx->feat_ld, g.fc1, ctx->hdense, ctx->feat_ld, n_nodes, nullptr,
                             true, ctx->gat_alpha, false)))
            return rc;
        if ((rc = gat_linear(ctx, s, ctx->hdense, ctx->feat_ld, g.fc2, ctx->act[2], ld_ft, n_nodes, nullptr, false,
                             0.f, half_rows, nullptr, nullptr, -1.0, cp, &done)))
            return rc;
        a->ft2 = ctx->act[2];
        *n_rows_ft2 = n_nodes;
    } else if (in == GAT_IN_IMPLICIT) {
        // heads only: edge-node rows are the layer-0 constants
        if (ctx->l0_grouped && !red && linear_uses_tile_kernel(b->n_heads, g.in_dim)) {
            // ONE grouped launch: camera c's heads (device-side count, rows gathered from the compact
            // features and scattered back to head order) x camera c's J*10-column block of fc1
            GemmProf gp(ctx, s, 2.0 * b->n_heads * (double)g.in_dim * (J * 10), 0, 0);
            HIPCHK(ctx, launch_linear_grouped(s, ctx->xc, ctx->l0_ld, ctx->l0_w, ctx->l0_ld,
                                              (long)weight_rows(g.in_dim) * ctx->l0_ld, ctx->l0_b, ctx->h0, ctx->feat_ld,
                                              b->n_heads, ctx->cam_count, V, ctx->cam_list, ctx->cfg.max_heads, g.in_dim,
                                              ctx->l0_ld, true, ctx->gat_alpha, ctx->gat_acc64));
        } else if (ctx->l0_grouped) {
            // small batches / reduced precision: one launch per camera over that camera's heads
            const double flop_each = 2.0 * b->n_heads * (double)g.in_dim * (J * 10) / V;
            for (int c = 0; c < V; ++c)
                if ((rc = gat_linear(ctx, s, ctx->xc, ctx->l0_ld, ctx->l0_fc1[c], ctx->h0, ctx->feat_ld, b->n_heads,
                                     ctx->cam_count + c, true, ctx->gat_alpha, false,
                                     ctx->cam_list + (size_t)c * ctx->cfg.max_heads,
                                     ctx->cam_list + (size_t)c * ctx->cfg.max_heads, flop_each)))
                    return rc;
        } else if ((rc = gat_linear(ctx, s, ctx->x0, ctx->feat_ld, g.fc1, ctx->h0, ctx->feat_ld, b->n_heads, nullptr,
                                    true, ctx->gat_alpha, false)))
            return rc;
        if ((rc = gat_linear(ctx, s, ctx->h0, ctx->feat_ld, g.fc2, ctx->act[1], ld_ft, b->n_heads, nullptr, false,
                             0.f, half_rows, nullptr, nullptr, -1.0, cp, &done)))
            return rc;
        a->ft2 = ctx->act[1];
        *n_rows_ft2 = b->n_heads;
        a->en_const_ft2 = ctx->en0_ft2;
        a->en_const_a = ctx->en0_a;
    } else if (fuse_last && l == ctx->gat_layers - 1 && last_layer_fusable(ctx, g)) {
        // the deployed network's last layer (150 -> 150 -> 1) in the default precision: fc1, fc2 and the coefficients in ONE launch
        // (k_last_fused: the fc1 rows never leave the CU; the bits of the two launches below)
        if ((rc = ensure_split_weights(ctx, s, &g.fc1)) || (rc = ensure_split_weights(ctx, s, &g.fc2))) return rc;
        if (n_nodes > 0) {
            // The profile keeps ONE RECORD PER nn.Linear on the batch path, as gemm() files them (the census of records per precision
            // mode, tests/golden/harness/gemm_census.json, is held to that): fc1's record spans the launch, fc2's carries its FLOP
            // and no time of its own.  The sums of FLOP and of time are those of the launch.
            {
                GemmProf gp(ctx, s, 2.0 * n_nodes * (double)g.fc1.out_dim * g.fc1.in_dim, 0, 0, 1);
                HIPCHK(ctx, launch_last_fused(s, ctx->act[0], ctx->act_ld, g.fc1.w3, plane_elems(g.fc1), g.fc1.ldw, g.fc1.b, n_nodes, ctx->gat_alpha,
                                              g.fc2.w3, plane_elems(g.fc2), g.fc2.ldw, g.fc2.b, ctx->act[2], ld_ft, g.attn_l, g.attn_r, ctx->a12));
            }
            GemmProf gp2(ctx, s, 2.0 * n_nodes * (double)g.fc2.out_dim * g.fc2.in_dim, 0, 0, 1);
        }
        done = true;
        a->ft2 = ctx->act[2];
        *n_rows_ft2 = n_nodes;
    } else {
        // fc2 reads act[1] over fc2.ldw columns and fc1 writes fc1.out_dim of them (150 of 160 in the deployed last layer).  Inside a
        // forward pass the columns between hold the same rows of this batch's wider layers: finite wherever the row is, and they meet
        // zero weights.  A stage entry point finds there what the call BEFORE it left -- rows of another batch, a NaN of a bad
        // detection included, and 0 * NaN is NaN -- so it clears them (tests/test_gpu_nonfinite.py: Test B, gat_layer first).
        if (clear_fc1_pad && n_nodes > 0 && g.fc2.ldw > g.fc1.out_dim)
            HIPCHK(ctx, hipMemset2DAsync(ctx->act[1] + g.fc1.out_dim, (size_t)ctx->act_ld * sizeof(float), 0,
                                         (size_t)(g.fc2.ldw - g.fc1.out_dim) * sizeof(float), n_nodes, s));
        if ((rc = gat_linear(ctx, s, ctx->act[0], ctx->act_ld, g.fc1, ctx->act[1], ctx->act_ld, n_nodes, nullptr,
                             true, ctx->gat_alpha, false)))
            return rc;
        if ((rc = gat_linear(ctx, s, ctx->act[1], ctx->act_ld, g.fc2, ctx->act[2], ld_ft, n_nodes, nullptr, false,
                             0.f, half_rows, nullptr, nullptr, -1.0, cp, &done)))
            return rc;
        a->ft2 = ctx->act[2];
        *n_rows_ft2 = n_nodes;
    }
    // Layer 0 on device-featurised rows (fp32, 40-wide heads, implicit topology): coefficients and attention in ONE launch that
    // writes whole rows (gat.hip: k_l0_attention), so the coefficient kernel below is not launched.  The cross-check switches that
    // name the kernels of today's two launches keep them (read per call: tests toggle them).
    a->l0_whole_rows = 0;
    if (in == GAT_IN_IMPLICIT && l == 0 && !b->d_en_pair && !half_rows && !red && !no_epi && !getenv("MPE_NO_FUSED_ATTENTION") &&
        !getenv("MPE_FUSED_NO_OVERLAP") && !getenv("MPE_NO_HEAD_SRC_TABLE") &&
        l0_attention_available(ctx->cfg.max_heads_per_frame, V, g.heads, g.out_dim)) {
        a->l0_whole_rows = 1;
        a->a12_ready = 0;
        return MPE_OK;
    }
    if (!done && cp && g.out_dim == 40 && !half_rows && ctx->gat_split && !red) {
        // the split-bf16 form with f64 sums (layer-0 fc2: K = 902) has no coefficient epilogue: a1 | a2 by the coefficient kernel
        // (canonical order = the epilogue's, gat.hip:coef40), so that the attention stage still finds them ready
        HIPCHK(ctx, launch_attn_coef(s, a->ft2, ld_ft, *n_rows_ft2, g.heads, g.out_dim, g.attn_l, g.attn_r, ctx->a12, 0));
        done = true;
    }
    a->a12_ready = done ? 1 : 0;
    return MPE_OK;
}

AggArgs gat_agg_args(const mpe_ctx *ctx, int l) {
    const GatLayer &g = ctx->gat[l];
    AggArgs a{};
    a.heads = g.heads;
    a.out_dim = g.out_dim;
    a.alpha = ctx->gat_alpha;
    a.out_slope = ctx->gat_hidden_slope;
    const bool half_rows = ctx->gat_reduced || ctx->gat_attn_fp16;
    a.ft_half = half_rows ? 1 : 0;
    a.ld = half_rows ? 2 * ctx->act_ld : ctx->act_ld;
    a.a12 = ctx->a12;
    return a;
}

// the last layer's attention stage writes the scores: edge-nodes to d_scores_en, heads (optional) to d_scores_heads
void agg_scores_out(const mpe_ctx *ctx, AggArgs *a, float *d_scores_en, float *d_scores_heads) {
    a->out_mode = ctx->gat_out_mode;
    a->score_mode = 1;
    a->out = d_scores_en;
    a->out_heads = d_scores_heads;
    a->ld_out = 1;
}

int gat_attention(mpe_ctx *ctx, hipStream_t s, const mpe_batch *b, int l, const AggArgs &a, int n_rows_ft2) {
    const GatLayer &g = ctx->gat[l];
    if (a.l0_whole_rows && !a.score_mode && !a.out_pl && a.ld % 4 == 0 && a.ld_out % 4 == 0) {
        HIPCHK(ctx, launch_l0_attention(s, *b, ctx->cfg.n_cameras, ctx->cfg.max_heads_per_frame, ctx->node_off, ctx->en_pair, g.attn_l,
                                        g.attn_r, a));
        ++ctx->l0_attention_launches;
        return MPE_OK;
    }
    // (a one-layer network writes scores from layer 0: the kernels below compute the coefficients themselves when a12_ready == 0)
    HIPCHK(ctx, launch_gat_attention(s, *b, ctx->cfg.n_cameras, ctx->cfg.max_heads_per_frame, ctx->node_off,
                                     ctx->head_frame, ctx->en_frame, ctx->en_pair, g.attn_l, g.attn_r, ctx->a12, a,
                                     n_rows_ft2, ctx->head_src, explicit_deg_cap(ctx->cfg.max_heads_per_frame), ctx->x_m_cap));
    return MPE_OK;
}

int gat_topology(mpe_ctx *ctx, hipStream_t s, const mpe_batch *b) {
    if (b->d_en_pair && (size_t)b->n_frames * ctx->cfg.max_heads_per_frame * explicit_deg_cap(ctx->cfg.max_heads_per_frame) > ctx->head_src_cap)
        return fail(ctx, MPE_ERR_CAPACITY, "in-edge table too small for %d frames with explicit edge-node lists", b->n_frames);
    HIPCHK(ctx, launch_topology(s, *b, ctx->cfg.n_cameras, ctx->node_off, ctx->head_frame, ctx->en_frame, ctx->en_pair,
                                ctx->cfg.max_heads_per_frame, ctx->d_status, ctx->head_src,
                                explicit_deg_cap(ctx->cfg.max_heads_per_frame), ctx->x_m_cap));
    return MPE_OK;
}

// ---- small batches (a few frames; the reference's call pattern is one frame per call, test/metrics_from_model.py:120-300) ----
// (sixteen: measured against the batch path with one context on one stream -- 9 frames 336 against 429 us per call, 12: 389 / 456,
// 16: 427 / 449; 24: 577 / 531, 32: 657 / 558: the plane-fed GEMMs run one workgroup per CU and take a round per 256 of them)
constexpr int LAT_MAX_FRAMES = 16;
constexpr int LAT_MAX_NODES = 16384;

// Can this batch take the latency launches?  Default precision modes, implicit topology, rows featurised on the device, a network
// whose layers have instantiations (the deployed one: train_skeleton_matching.py:40-57) -- anything else keeps the batch path.
bool lat_gat_ok(mpe_ctx *ctx, const mpe_batch *b, bool dense_in) {
    if (!latency_path_on() || dense_in || b->d_en_pair || b->n_frames > LAT_MAX_FRAMES) return false;
    if (b->n_heads + b->n_edge_nodes > LAT_MAX_NODES || b->n_heads <= 0) return false;
    if (!ctx->gat_split || ctx->gat_acc64 || ctx->gat_reduced || ctx->gat_attn_fp16 || !ctx->l0_grouped) return false;
    // (cross-check switches of the batch path: a run that asks for the tile kernels at every batch size, for the coefficient kernel or
    // for another f64 threshold means the batch path's kernels)
    if (getenv("MPE_NO_COEF_EPILOGUE") || getenv("MPE_GAT_ACC64_MINK") || getenv("MPE_SKINNY_WAVES") || getenv("MPE_GEMM_NARROW")) return false;
    if (!lat_l0a_available(ctx->cfg.n_joints, ctx->l0_ld)) return false;
    const GatLayer &g0 = ctx->gat[0];
    if (g0.out_dim != 40 || g0.in_dim <= 512) return false;      // layer 0: fc2 with f64 sums + the coefficient kernel, as the batch path
    for (int l = 1; l < ctx->gat_layers; ++l) {
        const GatLayer &g = ctx->gat[l];
        if (!lat_gemm_available(g.fc1.ldw, g.in_dim, false, 0) || !lat_gemm_available(g.fc2.ldw, g.heads * g.out_dim, true, g.out_dim)) return false;
        if (g.in_dim > 512) return false;                        // (such a layer would run with f64 sums)
    }
    const size_t shm = (size_t)2 * ((size_t)16 * (ctx->cfg.max_heads_per_frame + 1) + (ctx->cfg.max_heads_per_frame + 1) + 1 +
                                    (size_t)(ctx->cfg.n_cameras + 1) * (ctx->cfg.n_cameras + 1)) * sizeof(float);
    return shm <= 40 * 1024;
}

int ensure_lat_workspace(mpe_ctx *ctx) {
    if (ctx->gat_pl[0]) return MPE_OK;
    ctx->lat_rows = ctx->max_nodes < LAT_MAX_NODES ? ctx->max_nodes : LAT_MAX_NODES;
    ctx->gat_pl_plane = (size_t)ctx->lat_rows * ctx->act_ld;
    int rc;
    for (int i = 0; i < 2; ++i)
        if ((rc = dev_alloc(ctx, &ctx->gat_pl[i], 3 * ctx->gat_pl_plane))) return rc;       // zeroed: pad columns meet zero weights
    return MPE_OK;
}

// The matching network for a small batch in 3 + 3 (L - 1) launches instead of ~26: front + layer-0 fc1 (k_lat_l0a), layer-0 fc2 as the
// batch path has it, then per layer attention (both halves, one launch) -> fc1 -> fc2 with the activations
// travelling as bf16 planes between them (k_lat_gemm).  Same arithmetic, same summation orders, same bits as the batch kernels.
// *tail (optional): the attention stage of the LAST layer is left to the caller's tail launch (k_lat_tail: scores + clustering in one
// launch) when the layer's coefficients come from the fc2 epilogue; *tail says whether it was, and describes the stage.
struct LatTail {
    bool deferred = false;
    const float *ft2 = nullptr;
    int ld = 0;
    float alpha = 0.f, out_slope = 0.f;
    int out_mode = 0;
};

int run_gat_lat(mpe_ctx *ctx, hipStream_t s, const mpe_batch *b, float *d_scores_en, float *d_scores_heads, LatTail *tail = nullptr) {
    if (tail) tail->deferred = false;
    int rc = ensure_lat_workspace(ctx);
    if (rc) return rc;
    const int V = ctx->cfg.n_cameras, J = ctx->cfg.n_joints, hmax = ctx->cfg.max_heads_per_frame;
    const int n_nodes = b->n_heads + b->n_edge_nodes;
    if (n_nodes > ctx->lat_rows) return fail(ctx, MPE_ERR_CAPACITY, "latency path: %d nodes exceed %d", n_nodes, ctx->lat_rows);
    GatLayer &g0 = ctx->gat[0];
    uint16_t *head_src = getenv("MPE_NO_HEAD_SRC_TABLE") ? nullptr : ctx->head_src;          // read per call: tests toggle it
    {
        GemmProf gp(ctx, s, 2.0 * b->n_heads * (double)g0.in_dim * (J * 10), 0, 0);
        HIPCHK(ctx, launch_lat_l0a(s, ctx->d_cfg, *b, V, J, ctx->node_off, ctx->head_frame, ctx->en_frame, ctx->en_pair, ctx->head_src, hmax,
                                   ctx->d_status, ctx->l0_w, (long)weight_rows(g0.in_dim) * ctx->l0_ld, ctx->l0_ld, ctx->l0_b, g0.in_dim, ctx->h0,
                                   ctx->feat_ld, ctx->gat_alpha));
    }
    bool done = false;
    if ((rc = gat_linear(ctx, s, ctx->h0, ctx->feat_ld, g0.fc2, ctx->act[1], ctx->act_ld, b->n_heads, nullptr, false, 0.f, false, nullptr, nullptr,
                         -1.0, nullptr, &done)))
        return rc;
    const int L = ctx->gat_layers;
    for (int l = 0; l < L; ++l) {
        GatLayer &g = ctx->gat[l];
        AggArgs a = gat_agg_args(ctx, l);
        a.attn_l = g.attn_l;
        a.attn_r = g.attn_r;
        bool coef = false;                                   // a1 | a2 already in a12?  (otherwise the attention kernel computes them from the rows)
        if (l == 0) {
            a.ft2 = ctx->act[1];
            a.en_const_ft2 = ctx->en0_ft2;
            a.en_const_a = ctx->en0_a;
        } else {
            if ((rc = ensure_split_weights(ctx, s, &g.fc1)) || (rc = ensure_split_weights(ctx, s, &g.fc2))) return rc;
            const int hd = g.heads * g.out_dim;
            if (lat_gemm_fusable(g.fc1.ldw, g.in_dim, g.fc2.ldw, hd, g.out_dim)) {
                // the last layer: fc1 and the one-row fc2 in one launch (k_lat_gemm<.., FUSE2>)
                GemmProf gp(ctx, s, 2.0 * n_nodes * (double)g.in_dim * (g.in_dim + hd), 0, 0, 1);
                HIPCHK(ctx, launch_lat_gemm_fused(s, ctx->gat_pl[0], ctx->act_ld, ctx->gat_pl_plane, g.fc1.w3, plane_elems(g.fc1), g.fc1.ldw, g.fc1.b,
                                                  n_nodes, g.in_dim, ctx->gat_alpha, g.fc2.w3, plane_elems(g.fc2), g.fc2.ldw, g.fc2.b, ctx->act[2],
                                                  ctx->act_ld, g.attn_l, g.attn_r, ctx->a12));
                coef = true;
            } else {
                {
                    GemmProf gp(ctx, s, 2.0 * n_nodes * (double)g.in_dim * g.in_dim, 0, 0, 1);
                    HIPCHK(ctx, launch_lat_gemm(s, ctx->gat_pl[0], ctx->act_ld, ctx->gat_pl_plane, g.fc1.w3, plane_elems(g.fc1), g.fc1.ldw, g.fc1.b,
                                                nullptr, 0, ctx->gat_pl[1], ctx->act_ld, ctx->gat_pl_plane, n_nodes, g.in_dim, g.fc1.ldw, false,
                                                ctx->gat_alpha, nullptr, nullptr, nullptr, 0));
                }
                GemmProf gp(ctx, s, 2.0 * n_nodes * (double)hd * g.in_dim, 0, 0, 1);
                HIPCHK(ctx, launch_lat_gemm(s, ctx->gat_pl[1], ctx->act_ld, ctx->gat_pl_plane, g.fc2.w3, plane_elems(g.fc2), g.fc2.ldw, g.fc2.b,
                                            ctx->act[2], ctx->act_ld, nullptr, 0, 0, n_nodes, hd, g.fc2.ldw, true, 0.f, g.attn_l, g.attn_r, ctx->a12,
                                            g.out_dim, &coef));
            }
            a.ft2 = ctx->act[2];
        }
        a.a12_ready = coef ? 1 : 0;
        if (l == L - 1) {
            agg_scores_out(ctx, &a, d_scores_en, d_scores_heads);
            if (tail && coef && !d_scores_heads && g.heads == 1 && g.out_dim == 1) {
                tail->deferred = true;
                tail->ft2 = a.ft2;
                tail->ld = a.ld;
                tail->alpha = a.alpha;
                tail->out_slope = a.out_slope;
                tail->out_mode = a.out_mode;
                return MPE_OK;
            }
        } else {
            a.out_mode = 0;
            a.out = nullptr;
            a.out_pl = ctx->gat_pl[0];
            a.out_pl_plane = ctx->gat_pl_plane;
            a.ld_out = ctx->act_ld;
        }
        HIPCHK(ctx, launch_lat_attention(s, *b, V, hmax, ctx->node_off, ctx->head_frame, ctx->en_frame, ctx->en_pair, a, head_src));
    }
    return MPE_OK;
}

int run_gat(mpe_ctx *ctx, hipStream_t s, const mpe_batch *b, float *d_scores_en, float *d_scores_heads,
            const float *d_feats = nullptr, int ld_feats = 0) {
    int rc = ensure_gat_workspace(ctx);
    if (rc) return rc;
    if (lat_gat_ok(ctx, b, d_feats != nullptr)) return run_gat_lat(ctx, s, b, d_scores_en, d_scores_heads);
    const int V = ctx->cfg.n_cameras, J = ctx->cfg.n_joints;
    const int n_nodes = b->n_heads + b->n_edge_nodes;
    if ((rc = gat_topology(ctx, s, b))) return rc;
    const bool dense_in = d_feats != nullptr;   // caller-provided N x F rows (GAT2.forward(inputs, g))
    if (dense_in) {
        if (ld_feats < ctx->gat[0].in_dim) return fail(ctx, MPE_ERR_INVALID, "feature stride too small");
        if ((rc = ensure_dense_workspace(ctx))) return rc;
        HIPCHK(ctx, hipMemcpy2DAsync(ctx->xdense, (size_t)ctx->feat_ld * sizeof(float), d_feats,
                                     (size_t)ld_feats * sizeof(float), (size_t)ctx->gat[0].in_dim * sizeof(float),
                                     n_nodes, hipMemcpyDeviceToDevice, s));
    } else if (ctx->l0_grouped) {
        HIPCHK(ctx, launch_head_features(s, ctx->d_cfg, *b, J, ctx->xc, ctx->l0_ld, 0, 0, false, ctx->cam_count, V));
        HIPCHK(ctx, launch_group_heads(s, b->n_heads, V, b->d_head_cam, ctx->cam_count, ctx->cam_list,
                                       ctx->cfg.max_heads, true));
    } else {
        HIPCHK(ctx, launch_head_features(s, ctx->d_cfg, *b, J, ctx->x0, ctx->feat_ld, 0, 0, true));
    }
    const int L = ctx->gat_layers;
    for (int l = 0; l < L; ++l) {
        const bool last = l == L - 1;
        AggArgs a = gat_agg_args(ctx, l);
        int n_rows_ft2 = 0;
        if ((rc = gat_layer_linear(ctx, s, b, l, l > 0 ? GAT_IN_ACT : dense_in ? GAT_IN_DENSE0 : GAT_IN_IMPLICIT, &a,
                                   &n_rows_ft2, !dense_in)))
            return rc;
        if (last) {
            agg_scores_out(ctx, &a, d_scores_en, d_scores_heads);
        } else {
            a.out_mode = 0;
            a.out = ctx->act[0];
            a.ld_out = ctx->act_ld;
        }
        if ((rc = gat_attention(ctx, s, b, l, a, n_rows_ft2))) return rc;
    }
    return MPE_OK;
}

// stage-level entry points: caller rows [n_nodes][ld] <-> workspace rows
int copy_rows_in(mpe_ctx *ctx, hipStream_t s, float *dst, int ld_dst, const float *src, int ld_src, int cols, int rows) {
    if (rows <= 0) return MPE_OK;
    // the GEMMs read whole padded rows: columns beyond `cols` must be finite (they meet zero weights)
    HIPCHK(ctx, hipMemsetAsync(dst, 0, (size_t)rows * ld_dst * sizeof(float), s));
    HIPCHK(ctx, hipMemcpy2DAsync(dst, (size_t)ld_dst * sizeof(float), src, (size_t)ld_src * sizeof(float),
                                 (size_t)cols * sizeof(float), rows, hipMemcpyDeviceToDevice, s));
    return MPE_OK;
}

}  // namespace

extern "C" {

const char *mpe_version(void) { return "mpe-hip 0.3 (gfx950)"; }

const char *mpe_last_error(const mpe_ctx *ctx) { return ctx ? ctx->err.c_str() : "null context"; }

int mpe_create(const mpe_config *cfg, mpe_ctx **out) {
    if (!cfg || !out) return MPE_ERR_INVALID;
    *out = nullptr;
    if (cfg->n_cameras < 1 || cfg->n_cameras > MPE_MAX_CAMERAS || cfg->n_joints < 1 ||
        cfg->n_joints > MPE_MAX_JOINTS || cfg->max_frames < 1 || cfg->max_heads < 1 || cfg->max_edge_nodes < 1 ||
        cfg->max_heads_per_frame < 2 || cfg->max_heads_per_frame > 32767 || cfg->max_persons_per_frame < 1 ||
        !cfg->Kinv || !cfg->K || !cfg->T_i || !cfg->P || !cfg->dist)
        return MPE_ERR_INVALID;
    int ndev = 0;
    if (hipGetDeviceCount(&ndev) != hipSuccess || ndev < 1) return MPE_ERR_HIP;
    mpe_ctx *ctx = new (std::nothrow) mpe_ctx();
    if (!ctx) return MPE_ERR_NOMEM;
    ctx->cfg = *cfg;
    if (hipGetDevice(&ctx->device) != hipSuccess) {
        delete ctx;
        return MPE_ERR_HIP;
    }
    DevCfg &h = ctx->hcfg;
    memset(&h, 0, sizeof h);
    h.V = cfg->n_cameras;
    h.J = cfg->n_joints;
    h.W = cfg->image_width;
    h.H = cfg->image_height;
    h.npj = cfg->numbers_per_joint;
    h.min_views = cfg->min_views;
    h.median_axis = cfg->median_axis;
    h.used_joint_mask = cfg->used_joint_mask;
    h.threshold = cfg->threshold;
    h.median_window = cfg->median_window;
    for (int c = 0; c < h.V; ++c) {
        memcpy(h.Kinv[c], cfg->Kinv + 9 * c, 9 * sizeof(float));
        memcpy(h.K[c], cfg->K + 9 * c, 9 * sizeof(float));
        memcpy(h.T_i[c], cfg->T_i + 16 * c, 16 * sizeof(float));
        memcpy(h.P[c], cfg->P + 12 * c, 12 * sizeof(double));
        memcpy(h.dist[c], cfg->dist + 5 * c, 5 * sizeof(double));
    }
    ctx->cfg.Kinv = ctx->cfg.K = ctx->cfg.T_i = nullptr;
    ctx->cfg.P = ctx->cfg.dist = nullptr;
    ctx->max_nodes = cfg->max_heads + cfg->max_edge_nodes;
    int rc = MPE_OK;
    do {
        if ((rc = dev_alloc(ctx, &ctx->d_cfg, 1))) break;
        if ((rc = dev_alloc(ctx, &ctx->d_status, 1))) break;
        if (hipHostMalloc(reinterpret_cast<void **>(&ctx->h_status), sizeof(int32_t), hipHostMallocDefault) != hipSuccess) { rc = MPE_ERR_NOMEM; break; }
        if (hipMemcpy(ctx->d_cfg, &h, sizeof h, hipMemcpyHostToDevice) != hipSuccess) { rc = MPE_ERR_HIP; break; }
        if ((rc = dev_alloc(ctx, &ctx->head_frame, (size_t)cfg->max_heads))) break;
        if ((rc = dev_alloc(ctx, &ctx->en_frame, (size_t)cfg->max_edge_nodes))) break;
        if ((rc = dev_alloc(ctx, &ctx->en_pair, (size_t)cfg->max_edge_nodes * 2))) break;
        if ((rc = dev_alloc(ctx, &ctx->node_off, (size_t)cfg->max_frames + 1))) break;
        if ((rc = dev_alloc(ctx, &ctx->res_state, (size_t)cfg->n_cameras))) break;
        if ((rc = dev_alloc(ctx, &ctx->res_hist, (size_t)cfg->n_cameras * 2 * RESIDUAL_BINS))) break;
        if ((rc = dev_alloc(ctx, &ctx->res_partial, (size_t)cfg->n_cameras * RESIDUAL_SUM_BLOCKS))) break;
        ctx->cl_keys_per_frame = cluster_keys_per_frame(cfg->max_heads_per_frame);
        {
            // in-edge source table of the heads: implicit topology [hmax][hmax + 1] per frame; explicit edge-node lists
            // (mpe_batch::d_en_pair) [hmax][2 hmax], available while a frame's node ids fit the table's 16 bits.  A frame
            // of an explicit list may hold as many edge-nodes as the clustering scratch has keys.
            const size_t hm = (size_t)cfg->max_heads_per_frame;
            const bool x_ok = hm <= 1024 && hm + ctx->cl_keys_per_frame <= 65535;
            ctx->x_m_cap = x_ok ? (int)ctx->cl_keys_per_frame : 0;
            size_t per = head_src_entries(cfg->max_heads_per_frame, cfg->n_cameras);
            if (x_ok && hm * explicit_deg_cap(cfg->max_heads_per_frame) > per) per = hm * explicit_deg_cap(cfg->max_heads_per_frame);
            ctx->head_src_cap = per * cfg->max_frames;
            if (per && (rc = dev_alloc(ctx, &ctx->head_src, ctx->head_src_cap, false))) break;
        }
        ctx->cl_scratch_per_frame = cluster_scratch_per_frame(cfg->max_heads_per_frame);
        if ((rc = dev_alloc(ctx, &ctx->cl_keys, ctx->cl_keys_per_frame * cfg->max_frames, false))) break;
        if ((rc = dev_alloc(ctx, &ctx->cl_scratch, ctx->cl_scratch_per_frame * cfg->max_frames, false))) break;
        if ((rc = dev_alloc(ctx, &ctx->mlp_count, 1))) break;
        if ((rc = dev_alloc(ctx, &ctx->scores_tmp, (size_t)cfg->max_edge_nodes))) break;
        if (geom_needs_table(cfg->max_heads_per_frame, cfg->n_joints) &&
            (rc = dev_alloc(ctx, &ctx->geom_rays, geom_table_doubles(cfg->max_heads, cfg->n_joints), false))) break;
        if ((rc = dev_alloc(ctx, &ctx->person_off, (size_t)cfg->max_frames + 1))) break;
        if ((rc = dev_alloc(ctx, &ctx->valid_tmp, (size_t)cfg->max_frames * cfg->max_persons_per_frame))) break;
    } while (0);
    if (rc) {
        mpe_destroy(ctx);
        return rc;
    }
    *out = ctx;
    return MPE_OK;
}

void mpe_destroy(mpe_ctx *ctx) {
    if (!ctx) return;
    DeviceGuard dg(ctx);
    (void)hipDeviceSynchronize();
    for (void *p : ctx->owned) (void)hipFree(p);
    if (ctx->h_status) (void)hipHostFree(ctx->h_status);
    for (auto &r : ctx->prof) {
        (void)hipEventDestroy(r.start);
        (void)hipEventDestroy(r.stop);
    }
    if (ctx->tot_start) (void)hipEventDestroy(ctx->tot_start);
    if (ctx->tot_stop) (void)hipEventDestroy(ctx->tot_stop);
    delete ctx;
}

int mpe_set_gat_params(mpe_ctx *ctx, int32_t n_layers, float alpha, float hidden_slope) {
    if (!ctx) return MPE_ERR_INVALID;
    DeviceGuard dg(ctx);
    if (n_layers < 2 || n_layers > MPE_MAX_GAT_LAYERS) return fail(ctx, MPE_ERR_INVALID, "bad GAT layer count %d", n_layers);
    if (ctx->gat_ws_ready) return fail(ctx, MPE_ERR_STATE, "GAT weights are frozen after the first batch");
    ctx->gat_layers = n_layers;
    ctx->gat_alpha = alpha;
    ctx->gat_hidden_slope = hidden_slope;
    return MPE_OK;
}

int mpe_set_gat_layer(mpe_ctx *ctx, int32_t layer, int32_t in_dim, int32_t heads, int32_t out_dim, const float *fc1_w,
                      const float *fc1_b, const float *fc2_w, const float *fc2_b, const float *attn_l,
                      const float *attn_r) {
    if (!ctx) return MPE_ERR_INVALID;
    DeviceGuard dg(ctx);
    if (layer < 0 || layer >= ctx->gat_layers) return fail(ctx, MPE_ERR_INVALID, "GAT layer index %d out of range", layer);
    if (ctx->gat_ws_ready) return fail(ctx, MPE_ERR_STATE, "GAT weights are frozen after the first batch");
    if (!fc1_w || !fc1_b || !fc2_w || !fc2_b || !attn_l || !attn_r || heads < 1 || out_dim < 1)
        return fail(ctx, MPE_ERR_INVALID, "GAT layer %d: missing tensor", layer);
    GatLayer &g = ctx->gat[layer];
    dev_free(ctx, g.attn_l);               // a layer set twice does not keep its first copies
    dev_free(ctx, g.attn_r);
    g.attn_l = g.attn_r = nullptr;
    ctx->gat_ready[layer] = false;
    g.in_dim = in_dim;
    g.heads = heads;
    g.out_dim = out_dim;
    int rc;
    if ((rc = upload_linear(ctx, fc1_w, fc1_b, in_dim, in_dim, &g.fc1))) return rc;
    if ((rc = upload_linear(ctx, fc2_w, fc2_b, heads * out_dim, in_dim, &g.fc2))) return rc;
    if ((rc = dev_alloc(ctx, &g.attn_l, (size_t)heads * out_dim))) return rc;
    if ((rc = dev_alloc(ctx, &g.attn_r, (size_t)heads * out_dim))) return rc;
    HIPCHK(ctx, hipMemcpy(g.attn_l, attn_l, (size_t)heads * out_dim * sizeof(float), hipMemcpyHostToDevice));
    HIPCHK(ctx, hipMemcpy(g.attn_r, attn_r, (size_t)heads * out_dim * sizeof(float), hipMemcpyHostToDevice));
    ctx->gat_ready[layer] = true;
    return MPE_OK;
}

int mpe_set_mlp_params(mpe_ctx *ctx, int32_t n_layers, float slope) {
    if (!ctx) return MPE_ERR_INVALID;
    DeviceGuard dg(ctx);
    if (n_layers < 1 || n_layers > MPE_MAX_MLP_LAYERS) return fail(ctx, MPE_ERR_INVALID, "bad MLP layer count %d", n_layers);
    if (ctx->mlp_ws_ready) return fail(ctx, MPE_ERR_STATE, "MLP weights are frozen after the first batch");
    ctx->mlp_layers = n_layers;
    ctx->mlp_slope = slope;
    return MPE_OK;
}

int mpe_set_mlp_layer(mpe_ctx *ctx, int32_t layer, int32_t in_dim, int32_t out_dim, const float *w, const float *b) {
    if (!ctx) return MPE_ERR_INVALID;
    DeviceGuard dg(ctx);
    if (layer < 0 || layer >= ctx->mlp_layers) return fail(ctx, MPE_ERR_INVALID, "MLP layer index %d out of range", layer);
    if (ctx->mlp_ws_ready) return fail(ctx, MPE_ERR_STATE, "MLP weights are frozen after the first batch");
    if (!w || !b) return fail(ctx, MPE_ERR_INVALID, "MLP layer %d: missing tensor", layer);
    int rc = upload_linear(ctx, w, b, out_dim, in_dim, &ctx->mlp[layer]);
    if (rc) return rc;
    ctx->mlp_ready[layer] = true;
    return MPE_OK;
}

int mpe_upload_linear(mpe_ctx *ctx, const float *w, const float *b, int32_t out_dim, int32_t in_dim, float **d_w,
                      float **d_b, int32_t *ldw) {
    if (!ctx || !d_w || !d_b || !ldw) return MPE_ERR_INVALID;
    Linear L;
    int rc = upload_linear(ctx, w, b, out_dim, in_dim, &L);
    if (rc) return rc;
    *d_w = L.w;
    *d_b = L.b;
    *ldw = L.ldw;
    return MPE_OK;
}

int mpe_free_device(mpe_ctx *ctx, void *d_ptr) {
    if (!ctx) return MPE_ERR_INVALID;
    DeviceGuard dg(ctx);
    return dev_free(ctx, d_ptr) ? MPE_OK : fail(ctx, MPE_ERR_INVALID, "pointer not owned by this context");
}

int mpe_linear(mpe_ctx *ctx, void *stream, const float *d_a, int32_t lda, const float *d_w, int32_t ldw,
               const float *d_bias, float *d_c, int32_t ldc, int32_t m, const int32_t *d_m, int32_t n, int32_t k,
               int32_t slope_on, float slope) {
    if (!ctx) return MPE_ERR_INVALID;
    DeviceGuard dg(ctx);
    if (!d_a || !d_w || !d_bias || !d_c || m < 0 || n < 1 || k < 1)
        return fail(ctx, MPE_ERR_INVALID, "mpe_linear: bad argument");
    if (ldw % LD_ALIGN || ldw < k || lda < ldw || ldc % 4 || ldc < n)
        return fail(ctx, MPE_ERR_INVALID, "mpe_linear: strides must satisfy ldw%%32==0, lda>=ldw>=k, ldc%%4==0");
    // every form reads A and W in 16-byte pieces (vector loads or LDS-DMA) and all but the f64 form store C as four floats
    if (lda % 4 || (reinterpret_cast<uintptr_t>(d_a) & 15) || (reinterpret_cast<uintptr_t>(d_w) & 15) || (reinterpret_cast<uintptr_t>(d_c) & 15))
        return fail(ctx, MPE_ERR_INVALID, "mpe_linear: rows must be 16-byte aligned (d_a, d_w, d_c; lda %% 4 == 0)");
    // the split form's tile kernel addresses a row of its 256-row tile by a 32-bit byte offset per lane, (row - m0) * lda * 4 (gemm_sb16.hip)
    if (lda > LINEAR_MAX_LDA)
        return fail(ctx, MPE_ERR_INVALID, "mpe_linear: lda %d beyond %d (255 rows of it must fit a 32-bit byte offset)", lda, LINEAR_MAX_LDA);
    Linear L;
    L.w = const_cast<float *>(d_w);
    L.b = const_cast<float *>(d_bias);
    L.in_dim = k;
    L.out_dim = n;
    L.ldw = ldw;
    if (slope_on & 32) {
        HIPCHK(ctx, launch_linear_f64(static_cast<hipStream_t>(stream), d_a, lda, d_w, ldw, d_bias, d_c, ldc, m, d_m, n, ldw, (slope_on & 1) != 0, slope));
        return MPE_OK;
    }
    if (slope_on & 4) {
        // split-bf16 arithmetic (gemm_sb16.hip) on caller-provided weights: the planes are made for this call (a stage-level
        // entry point for tests; the batch entry points keep theirs with the context)
        hipStream_t s = static_cast<hipStream_t>(stream);
        // (d_w must hold weight_rows(n) = round_up(n, 16) + 208 rows of ldw floats, zero padded, as mpe_upload_linear prepares
        // them: the planes are made of all of them, and the loader's 32-bit per-lane offset covers 3 planes of that size)
        const size_t count = plane_elems(L);
        if (3 * count * sizeof(unsigned short) >= ((size_t)1 << 32))
            return fail(ctx, MPE_ERR_INVALID, "mpe_linear (split form): n x ldw too large for the 32-bit plane offsets");
        unsigned short *planes = nullptr;
        HIPCHK(ctx, hipMalloc(reinterpret_cast<void **>(&planes), 3 * count * sizeof(unsigned short)));
        hipError_t e = launch_split_planes(s, d_w, count, planes);
        if (e == hipSuccess)
            e = launch_linear_sb16(s, d_a, lda, planes, count, ldw, d_bias, d_c, ldc, m, d_m, n, ldw, (slope_on & 1) != 0, slope, (slope_on & 8) == 0,
                                   nullptr, nullptr, false, (slope_on & 16) ? 1 : 2);
        if (e == hipSuccess) e = hipStreamSynchronize(s);
        (void)hipFree(planes);
        HIPCHK(ctx, e);
        return MPE_OK;
    }
    return gemm(ctx, static_cast<hipStream_t>(stream), (slope_on & 2) ? GemmForm::F32_ACC64 : GemmForm::F32, L,
                {d_a, lda, d_c, ldc, m, d_m, (slope_on & 1) != 0, slope});
}

int mpe_head_features(mpe_ctx *ctx, void *stream, const mpe_batch *b, float *d_feat) {
    int rc = check_batch(ctx, b);
    if (rc) return rc;
    if (b->n_frames == 0) return MPE_OK;        // an empty batch has nothing to write (outputs may be NULL)
    DeviceGuard dg(ctx);
    if (!d_feat) return fail(ctx, MPE_ERR_INVALID, "d_feat is NULL");
    HIPCHK(ctx, launch_head_features(static_cast<hipStream_t>(stream), ctx->d_cfg, *b, ctx->cfg.n_joints, d_feat,
                                     ctx->cfg.n_joints * 10, 0, 0, false));
    return MPE_OK;
}

int mpe_dense_rows(mpe_ctx *ctx, void *stream, const mpe_batch *b, float *d_rows, int32_t ld) {
    int rc = check_batch(ctx, b);
    if (rc) return rc;
    if (b->n_frames == 0) return MPE_OK;
    DeviceGuard dg(ctx);
    const int F = 2 + ctx->cfg.n_cameras * ctx->cfg.n_joints * 10;
    if (!d_rows || ld < F) return fail(ctx, MPE_ERR_INVALID, "mpe_dense_rows: d_rows is NULL or ld < %d", F);
    if (b->n_frames != 1) return fail(ctx, MPE_ERR_UNSUPPORTED, "mpe_dense_rows: one graph per call (node order = heads, then edge-nodes)");
    hipStream_t s = static_cast<hipStream_t>(stream);
    HIPCHK(ctx, launch_head_features(s, ctx->d_cfg, *b, ctx->cfg.n_joints, d_rows, ld, 0, 0, true));
    HIPCHK(ctx, launch_onehot_rows(s, d_rows + (size_t)b->n_heads * ld, b->n_edge_nodes, ld, 1));
    return MPE_OK;
}

int mpe_gat_forward(mpe_ctx *ctx, void *stream, const mpe_batch *b, const float *d_feats, int32_t ld_feats,
                    float *d_scores_en, float *d_scores_heads) {
    int rc = check_batch(ctx, b);
    if (rc) return rc;
    if (b->n_frames == 0) return MPE_OK;        // an empty batch has nothing to write (outputs may be NULL)
    DeviceGuard dg(ctx);
    if (!d_scores_en) return fail(ctx, MPE_ERR_INVALID, "d_scores_en is NULL");
    return run_gat(ctx, static_cast<hipStream_t>(stream), b, d_scores_en, d_scores_heads, d_feats, ld_feats);
}

int mpe_set_gat_output(mpe_ctx *ctx, int32_t mode) {
    if (!ctx) return MPE_ERR_INVALID;
    if (mode != 1 && mode != 2) return fail(ctx, MPE_ERR_INVALID, "GAT output mode: 1 = sigmoid, 2 = identity");
    ctx->gat_out_mode = mode;
    return MPE_OK;
}

static int report_status(mpe_ctx *ctx, int32_t st) {
    if (st & 2)
        return fail(ctx, MPE_ERR_INVALID, "an explicit edge-node list held a pair outside its frame (or h1 == h2), or repeated pairs "
                    "beyond the in-degree capacity 2 * max_heads_per_frame; such pairs were replaced / dropped");
    if (st & 1)
        return fail(ctx, MPE_ERR_CAPACITY, "a frame holds more than max_heads_per_frame = %d skeletons (or, with an explicit edge-node list, more "
                    "than %d edge-nodes); its scores are zero and it produced no persons", ctx->cfg.max_heads_per_frame, ctx->x_m_cap);
    return MPE_OK;
}

// mpe_sync_status in two halves, for a caller that has more to do before it waits (the per-frame mirrors: the read-back of the status
// word joins the chain it belongs to instead of starting a chain of its own after the wait): mpe_status_queue orders the read-back and
// the reset behind everything queued so far, mpe_status_wait synchronises and reports it.
int mpe_status_queue(mpe_ctx *ctx, void *stream) {
    if (!ctx) return MPE_ERR_INVALID;
    DeviceGuard dg(ctx);
    hipStream_t s = static_cast<hipStream_t>(stream);
    if (ctx->status_queued) {                       // an earlier half nobody waited for: its word must not be lost
        HIPCHK(ctx, hipStreamSynchronize(ctx->status_stream));      // (the stream IT was ordered on, which need not be `s`)
        ctx->status_carry |= *ctx->h_status;
        ctx->status_queued = false;
    }
    HIPCHK(ctx, hipMemcpyAsync(ctx->h_status, ctx->d_status, sizeof(int32_t), hipMemcpyDeviceToHost, s));
    HIPCHK(ctx, hipMemsetAsync(ctx->d_status, 0, sizeof(int32_t), s));
    ctx->status_queued = true;
    ctx->status_stream = s;
    return MPE_OK;
}

int mpe_status_wait(mpe_ctx *ctx, void *stream) {
    if (!ctx) return MPE_ERR_INVALID;
    if (!ctx->status_queued) {
        const int rc = mpe_status_queue(ctx, stream);
        if (rc) return rc;
    }
    DeviceGuard dg(ctx);
    // the pending read-back may have been ordered on another stream than `stream`: h_status is valid once THAT stream has drained
    if (ctx->status_stream != static_cast<hipStream_t>(stream)) HIPCHK(ctx, hipStreamSynchronize(ctx->status_stream));
    HIPCHK(ctx, hipStreamSynchronize(static_cast<hipStream_t>(stream)));
    ctx->status_queued = false;
    const int32_t st = *ctx->h_status | ctx->status_carry;
    ctx->status_carry = 0;
    return report_status(ctx, st);
}

int mpe_sync_status(mpe_ctx *ctx, void *stream) {
    const int rc = mpe_status_queue(ctx, stream);
    return rc ? rc : mpe_status_wait(ctx, stream);
}

static int stage_layer_checks(mpe_ctx *ctx, const mpe_batch *b, int32_t layer, const void *in, int32_t ld_in, int cols_in,
                              const void *out, int32_t ld_out, int cols_out) {
    if (layer < 0 || layer >= ctx->gat_layers) return fail(ctx, MPE_ERR_INVALID, "GAT layer index %d out of range", layer);
    if (!in || !out || ld_in < cols_in || ld_out < cols_out)
        return fail(ctx, MPE_ERR_INVALID, "stage entry point: need ld_in >= %d and ld_out >= %d", cols_in, cols_out);
    (void)b;
    return MPE_OK;
}

int mpe_gat_layer(mpe_ctx *ctx, void *stream, const mpe_batch *b, int32_t layer, const float *d_in, int32_t ld_in,
                  float *d_out, int32_t ld_out, int32_t activation) {
    int rc = check_batch(ctx, b);
    if (rc) return rc;
    if (b->n_frames == 0) return MPE_OK;        // an empty batch has nothing to write (outputs may be NULL)
    DeviceGuard dg(ctx);
    if ((rc = ensure_gat_workspace(ctx))) return rc;
    if (activation < 0 || activation > 2) return fail(ctx, MPE_ERR_INVALID, "activation: 0 LeakyReLU, 1 sigmoid, 2 none");
    if (layer < 0 || layer >= ctx->gat_layers) return fail(ctx, MPE_ERR_INVALID, "GAT layer index %d out of range", layer);
    const GatLayer &g = ctx->gat[layer];
    const int hd = g.heads * g.out_dim;
    // layer 0 with d_in == NULL: the rows are featurised on the device, as mpe_gat_forward(d_feats == NULL) has them
    const bool implicit0 = layer == 0 && !d_in;
    if ((rc = stage_layer_checks(ctx, b, layer, implicit0 ? static_cast<const void *>(d_out) : d_in, implicit0 ? g.in_dim : ld_in, g.in_dim,
                                 d_out, ld_out, hd)))
        return rc;
    if (implicit0 && b->d_en_pair) return fail(ctx, MPE_ERR_INVALID, "mpe_gat_layer: device-featurised rows need the implicit topology");
    hipStream_t s = static_cast<hipStream_t>(stream);
    const int n_nodes = b->n_heads + b->n_edge_nodes;
    if ((rc = gat_topology(ctx, s, b))) return rc;
    if (implicit0) {
        const int V = ctx->cfg.n_cameras, J = ctx->cfg.n_joints;
        // (the attention kernels differ in what they leave for frames without a graph: such rows read 0 here)
        if (n_nodes > 0) HIPCHK(ctx, hipMemsetAsync(ctx->act[0], 0, (size_t)n_nodes * ctx->act_ld * sizeof(float), s));
        if (ctx->l0_grouped) {
            HIPCHK(ctx, launch_head_features(s, ctx->d_cfg, *b, J, ctx->xc, ctx->l0_ld, 0, 0, false, ctx->cam_count, V));
            HIPCHK(ctx, launch_group_heads(s, b->n_heads, V, b->d_head_cam, ctx->cam_count, ctx->cam_list, ctx->cfg.max_heads, true));
        } else {
            HIPCHK(ctx, launch_head_features(s, ctx->d_cfg, *b, J, ctx->x0, ctx->feat_ld, 0, 0, true));
        }
    } else if (layer == 0) {
        if ((rc = ensure_dense_workspace(ctx))) return rc;
        if ((rc = copy_rows_in(ctx, s, ctx->xdense, ctx->feat_ld, d_in, ld_in, g.in_dim, n_nodes))) return rc;
    } else if ((rc = copy_rows_in(ctx, s, ctx->act[0], ctx->act_ld, d_in, ld_in, g.in_dim, n_nodes)))
        return rc;
    AggArgs a = gat_agg_args(ctx, layer);
    int n_rows_ft2 = 0;
    if ((rc = gat_layer_linear(ctx, s, b, layer, implicit0 ? GAT_IN_IMPLICIT : layer == 0 ? GAT_IN_DENSE0 : GAT_IN_ACT, &a, &n_rows_ft2, false, true)))
        return rc;
    a.out_mode = activation;
    a.out = ctx->act[0];
    a.ld_out = ctx->act_ld;
    if ((rc = gat_attention(ctx, s, b, layer, a, n_rows_ft2))) return rc;
    if (n_nodes > 0)
        HIPCHK(ctx, hipMemcpy2DAsync(d_out, (size_t)ld_out * sizeof(float), ctx->act[0], (size_t)ctx->act_ld * sizeof(float),
                                     (size_t)hd * sizeof(float), n_nodes, hipMemcpyDeviceToDevice, s));
    return MPE_OK;
}

int mpe_edge_softmax_aggregate(mpe_ctx *ctx, void *stream, const mpe_batch *b, int32_t layer, const float *d_ft2,
                               int32_t ld_ft2, float *d_out, int32_t ld_out) {
    int rc = check_batch(ctx, b);
    if (rc) return rc;
    if (b->n_frames == 0) return MPE_OK;        // an empty batch has nothing to write (outputs may be NULL)
    DeviceGuard dg(ctx);
    if ((rc = ensure_gat_workspace(ctx))) return rc;
    if (layer < 0 || layer >= ctx->gat_layers) return fail(ctx, MPE_ERR_INVALID, "GAT layer index %d out of range", layer);
    if (ctx->gat_reduced || ctx->gat_attn_fp16)
        return fail(ctx, MPE_ERR_STATE, "mpe_edge_softmax_aggregate takes fp32 rows (a reduced-precision mode is on)");
    const GatLayer &g = ctx->gat[layer];
    const int hd = g.heads * g.out_dim;
    if ((rc = stage_layer_checks(ctx, b, layer, d_ft2, ld_ft2, hd, d_out, ld_out, hd))) return rc;
    hipStream_t s = static_cast<hipStream_t>(stream);
    const int n_nodes = b->n_heads + b->n_edge_nodes;
    if ((rc = gat_topology(ctx, s, b))) return rc;
    if ((rc = copy_rows_in(ctx, s, ctx->act[2], ctx->act_ld, d_ft2, ld_ft2, hd, n_nodes))) return rc;
    AggArgs a = gat_agg_args(ctx, layer);
    a.ft2 = ctx->act[2];
    a.out_mode = 2;
    a.out = ctx->act[0];
    a.ld_out = ctx->act_ld;
    if ((rc = gat_attention(ctx, s, b, layer, a, n_nodes))) return rc;
    if (n_nodes > 0)
        HIPCHK(ctx, hipMemcpy2DAsync(d_out, (size_t)ld_out * sizeof(float), ctx->act[0], (size_t)ctx->act_ld * sizeof(float),
                                     (size_t)hd * sizeof(float), n_nodes, hipMemcpyDeviceToDevice, s));
    return MPE_OK;
}

int mpe_set_threshold(mpe_ctx *ctx, float threshold) {
    if (!ctx) return MPE_ERR_INVALID;
    DeviceGuard dg(ctx);
    if (!(threshold >= 0.f)) return fail(ctx, MPE_ERR_INVALID, "threshold must be >= 0");
    ctx->hcfg.threshold = threshold;
    ctx->cfg.threshold = threshold;
    HIPCHK(ctx, hipMemcpy(ctx->d_cfg, &ctx->hcfg, sizeof ctx->hcfg, hipMemcpyHostToDevice));
    return MPE_OK;
}

int mpe_cluster_batch(mpe_ctx *ctx, void *stream, const mpe_batch *b, const float *d_scores, int32_t *d_persons,
                      int32_t *d_n_persons) {
    int rc = check_batch(ctx, b);
    if (rc) return rc;
    if (b->n_frames == 0) return MPE_OK;        // an empty batch has nothing to write (outputs may be NULL)
    DeviceGuard dg(ctx);
    if (!d_scores || !d_persons || !d_n_persons) return fail(ctx, MPE_ERR_INVALID, "mpe_cluster_batch: NULL output");
    hipStream_t s = static_cast<hipStream_t>(stream);
    if ((rc = gat_topology(ctx, s, b))) return rc;
    HIPCHK(ctx, launch_cluster(s, ctx->d_cfg, *b, ctx->en_pair, d_scores, ctx->cfg.max_persons_per_frame,
                               ctx->cfg.max_heads_per_frame, ctx->cl_keys, ctx->cl_keys_per_frame, ctx->cl_scratch,
                               ctx->cl_scratch_per_frame, d_persons, d_n_persons));
    return MPE_OK;
}

int mpe_match_batch(mpe_ctx *ctx, void *stream, const mpe_batch *b, float *d_scores, int32_t *d_persons,
                    int32_t *d_n_persons) {
    int rc = check_batch(ctx, b);
    if (rc) return rc;
    if (b->n_frames == 0) return MPE_OK;        // an empty batch has nothing to write (outputs may be NULL)
    DeviceGuard dg(ctx);
    if (!d_persons || !d_n_persons) return fail(ctx, MPE_ERR_INVALID, "mpe_match_batch: NULL output");
    hipStream_t s = static_cast<hipStream_t>(stream);
    float *scores = d_scores;
    if (!scores) {
        scores = ctx->scores_tmp;
    }
    const int hmax = ctx->cfg.max_heads_per_frame;
    if ((rc = ensure_gat_workspace(ctx))) return rc;
    // (whatever route this call takes: check_batch has forgotten the pairs an earlier call solved)
    if (lat_gat_ok(ctx, b, false) && lat_tail_available(hmax, ctx->cl_keys_per_frame) && b->n_edge_nodes > 0) {
        // small batch: the last layer's scores and the clustering in ONE launch, and beside them every cross-camera pair of the batch
        // solved for the row kernel of mpe_mlp3d_batch (which recognises the batch and the persons by the note left here)
        LatTail tail;
        if ((rc = run_gat_lat(ctx, s, b, scores, nullptr, &tail))) return rc;
        if (tail.deferred) {
            const int J = ctx->cfg.n_joints;
            const int slot = ctx->handoff.write_slot();
            const size_t need = (size_t)LAT_MAX_FRAMES * hmax * hmax * J * 3;
            // (the buffer is indexed by the batch's head number: a batch whose frames are within capacity has at most 16 hmax of them;
            // anything else -- flagged on the device, rejected by Engine.check_capacity -- gets no pair solves and no note)
            const bool pairs_ok = (size_t)b->n_heads <= (size_t)LAT_MAX_FRAMES * hmax;
            if (pairs_ok && !ctx->pair_pts[slot] && (rc = dev_alloc(ctx, &ctx->pair_pts[slot], need, false))) return rc;
            HIPCHK(ctx, launch_lat_tail(s, ctx->d_cfg, *b, J, ctx->en_pair, ctx->en_frame, tail.ft2, tail.ld, ctx->a12, tail.alpha, tail.out_slope,
                                        tail.out_mode, ctx->node_off, scores, ctx->cfg.max_persons_per_frame, hmax, ctx->cl_keys_per_frame, d_persons,
                                        d_n_persons, pairs_ok ? ctx->pair_pts[slot] : nullptr));
            if (pairs_ok) ctx->handoff.note(mpe::pair_key(*b, d_persons, d_n_persons));      // (the next write goes to the other buffer)
            return MPE_OK;
        }
    } else if ((rc = run_gat(ctx, s, b, scores, nullptr))) {
        return rc;
    }
    HIPCHK(ctx, launch_cluster(s, ctx->d_cfg, *b, ctx->en_pair, scores, ctx->cfg.max_persons_per_frame,
                               ctx->cfg.max_heads_per_frame, ctx->cl_keys, ctx->cl_keys_per_frame, ctx->cl_scratch,
                               ctx->cl_scratch_per_frame, d_persons, d_n_persons));
    return MPE_OK;
}

int mpe_mlp_input_rows(mpe_ctx *ctx, void *stream, const mpe_batch *b, const int32_t *d_persons,
                       const int32_t *d_n_persons, float *d_rows, int32_t ld_rows, uint8_t *d_valid) {
    int rc = check_batch(ctx, b);
    if (rc) return rc;
    if (b->n_frames == 0) return MPE_OK;        // an empty batch has nothing to write (outputs may be NULL)
    DeviceGuard dg(ctx);
    const int width = ctx->cfg.n_cameras * ctx->cfg.n_joints * ctx->cfg.numbers_per_joint;
    if (!d_persons || !d_n_persons || !d_rows || ld_rows < width)
        return fail(ctx, MPE_ERR_INVALID, "mpe_mlp_input_rows: bad argument");
    HIPCHK(ctx, launch_mlp_rows(static_cast<hipStream_t>(stream), ctx->d_cfg, ctx->cfg.n_cameras, ctx->cfg.n_joints, *b,
                                d_persons, d_n_persons, nullptr, ctx->cfg.max_persons_per_frame, d_rows, ld_rows,
                                d_valid));
    return MPE_OK;
}

static int mlp_chain(mpe_ctx *ctx, hipStream_t s, const float *x, int ld_x, int m, const int32_t *d_m, float **y_out,
                     int *ld_y, const DecodeEpi *dec = nullptr, bool *dec_done = nullptr) {
    if (dec_done) *dec_done = false;
    const float *in = x;
    int ld_in = ld_x;
    const GemmForm form = mlp_gemm_form(ctx->mlp_mode);
    for (int l = 0; l < ctx->mlp_layers; ++l) {
        Linear &L = ctx->mlp[l];
        float *out = ctx->mlp_act[l & 1];
        const bool last = l == ctx->mlp_layers - 1;
        GemmCall c{in, ld_in, out, ctx->mlp_ld_hidden, m, d_m, !last, ctx->mlp_slope};
        c.flush_stages = split_flush_stages(ctx->mlp_mode);
        c.dec = last ? dec : nullptr;
        c.dec_done = last ? dec_done : nullptr;
        c.bf16_min_ld = round_up(L.in_dim, 128);               // (= L.ldw16: the bf16 launches of the MLP read whole K stages)
        const int rc = gemm(ctx, s, form, L, c);
        if (rc) return rc;
        in = out;
        ld_in = ctx->mlp_ld_hidden;
    }
    *y_out = const_cast<float *>(in);
    *ld_y = ld_in;
    return MPE_OK;
}

int mpe_mlp_forward(mpe_ctx *ctx, void *stream, const float *d_x, int32_t ld_x, int32_t m, float *d_y, int32_t ld_y) {
    if (!ctx) return MPE_ERR_INVALID;
    DeviceGuard dg(ctx);
    int rc = ensure_mlp_workspace(ctx);
    if (rc) return rc;
    if (!d_x || !d_y || m < 0) return fail(ctx, MPE_ERR_INVALID, "mpe_mlp_forward: bad argument");
    if ((size_t)m > (size_t)ctx->cfg.max_frames * ctx->cfg.max_persons_per_frame)
        return fail(ctx, MPE_ERR_CAPACITY, "mpe_mlp_forward: %d rows exceed capacity", m);
    if (ld_x < ctx->mlp_ld_in) return fail(ctx, MPE_ERR_INVALID, "mpe_mlp_forward: ld_x must be >= %d (zero padded)", ctx->mlp_ld_in);
    // (the first layer reads d_x as mpe_linear reads A; d_y is written by a strided copy of n_out floats per row)
    if (ld_x % 4 || ld_x > LINEAR_MAX_LDA || (reinterpret_cast<uintptr_t>(d_x) & 15))
        return fail(ctx, MPE_ERR_INVALID, "mpe_mlp_forward: rows of d_x must be 16-byte aligned (ld_x %% 4 == 0) and ld_x <= %d", LINEAR_MAX_LDA);
    if (ld_y < ctx->mlp[ctx->mlp_layers - 1].out_dim)
        return fail(ctx, MPE_ERR_INVALID, "mpe_mlp_forward: ld_y %d < output width %d", ld_y, ctx->mlp[ctx->mlp_layers - 1].out_dim);
    hipStream_t s = static_cast<hipStream_t>(stream);
    float *y;
    int ldy;
    if ((rc = mlp_chain(ctx, s, d_x, ld_x, m, nullptr, &y, &ldy))) return rc;
    const int n_out = ctx->mlp[ctx->mlp_layers - 1].out_dim;
    HIPCHK(ctx, hipMemcpy2DAsync(d_y, (size_t)ld_y * sizeof(float), y, (size_t)ldy * sizeof(float),
                                 (size_t)n_out * sizeof(float), m, hipMemcpyDeviceToDevice, s));
    return MPE_OK;
}

int mpe_mlp3d_batch(mpe_ctx *ctx, void *stream, const mpe_batch *b, const int32_t *d_persons,
                    const int32_t *d_n_persons, float *d_poses, uint8_t *d_valid) {
    // the pairs mpe_match_batch left, if its note names exactly this batch and these persons: taken before check_batch forgets
    // the note, as it does for every batch call -- a hand-off is used once, whatever becomes of this call
    const int fetch = (ctx && b) ? ctx->handoff.take(mpe::pair_key(*b, d_persons, d_n_persons)) : -1;
    int rc = check_batch(ctx, b);
    if (rc) return rc;
    if (b->n_frames == 0) return MPE_OK;        // an empty batch has nothing to write (outputs may be NULL)
    DeviceGuard dg(ctx);
    if ((rc = ensure_mlp_workspace(ctx))) return rc;
    if (!d_persons || !d_n_persons || !d_poses) return fail(ctx, MPE_ERR_INVALID, "mpe_mlp3d_batch: NULL argument");
    hipStream_t s = static_cast<hipStream_t>(stream);
    const int pcap = ctx->cfg.max_persons_per_frame;
    const int n_out = ctx->mlp[ctx->mlp_layers - 1].out_dim;
    if (n_out != ctx->cfg.n_joints * 3)
        return fail(ctx, MPE_ERR_INVALID, "MLP output width %d != 3*J", n_out);
    // the decode rides in the last layer's launch wherever that launch has the epilogue (the K-split kernel: 54 features are four
    // column tiles at any batch size); small batches: the persons' prefix inside the row kernel as well
    const bool small = latency_path_on() && b->n_frames <= LAT_MAX_FRAMES;
    if (small) {
        // the batch whose pairs the call before this one, mpe_match_batch, left solved (same arrays, generation and sizes, the
        // persons it wrote)?  then the row kernel fetches them
        const double *pairs = fetch >= 0 ? ctx->pair_pts[fetch] : nullptr;
        HIPCHK(ctx, launch_mlp_rows(s, ctx->d_cfg, ctx->cfg.n_cameras, ctx->cfg.n_joints, *b, d_persons, d_n_persons, nullptr, pcap, ctx->mlp_rows,
                                    ctx->mlp_ld_in, d_valid ? d_valid : ctx->valid_tmp, ctx->person_off, ctx->mlp_count, d_poses, n_out, pairs,
                                    ctx->cfg.max_heads_per_frame));
    } else {
        HIPCHK(ctx, launch_person_scan(s, b->n_frames, pcap, d_n_persons, ctx->person_off, ctx->mlp_count));
        // (the row kernel zeroes the pose slots nobody fills, as on the small-batch route: the last layer's launch decodes the rest)
        HIPCHK(ctx, launch_mlp_rows(s, ctx->d_cfg, ctx->cfg.n_cameras, ctx->cfg.n_joints, *b, d_persons, d_n_persons,
                                    ctx->person_off, pcap, ctx->mlp_rows, ctx->mlp_ld_in, d_valid ? d_valid : ctx->valid_tmp, nullptr, nullptr,
                                    d_poses, n_out));
    }
    float *y;
    int ldy;
    const DecodeEpi dec{ctx->person_off, b->n_frames, pcap, n_out, 10.f, d_poses};
    bool decoded = false;
    if ((rc = mlp_chain(ctx, s, ctx->mlp_rows, ctx->mlp_ld_in, b->n_frames * pcap, ctx->mlp_count, &y, &ldy, &dec, &decoded))) return rc;
    if (!decoded) HIPCHK(ctx, launch_decode(s, b->n_frames, pcap, n_out, 10.f, d_n_persons, ctx->person_off, y, ldy, d_poses));
    return MPE_OK;
}

int mpe_triangulate_batch(mpe_ctx *ctx, void *stream, const mpe_batch *b, const int32_t *d_persons,
                          const int32_t *d_n_persons, double *d_poses, uint8_t *d_joint_valid, uint32_t flags) {
    int rc = check_batch(ctx, b);
    if (rc) return rc;
    if (b->n_frames == 0) return MPE_OK;        // an empty batch has nothing to write (outputs may be NULL)
    DeviceGuard dg(ctx);
    if (!d_persons || !d_n_persons || !d_poses || !d_joint_valid)
        return fail(ctx, MPE_ERR_INVALID, "mpe_triangulate_batch: NULL argument");
    HIPCHK(ctx, launch_triangulate(static_cast<hipStream_t>(stream), ctx->d_cfg, ctx->cfg.n_cameras, ctx->cfg.n_joints,
                                   *b, d_persons, d_n_persons, ctx->cfg.max_persons_per_frame, d_poses, d_joint_valid,
                                   (flags & 1u) ? 0xFFFFFFFFu : ctx->cfg.used_joint_mask, (flags & 2u) != 0));
    return MPE_OK;
}

int mpe_eval_batch(mpe_ctx *ctx, void *stream, const mpe_eval_args *a) {
    if (!ctx) return MPE_ERR_INVALID;
    if (!a) return fail(ctx, MPE_ERR_INVALID, "mpe_eval_batch: NULL argument");
    DeviceGuard dg(ctx);
    if (a->n_frames < 0 || a->pcap < 1 || a->gcap < 1 || a->n_joints < 1 || (a->pose_f64 & ~1) || (a->joint_flags & ~1))
        return fail(ctx, MPE_ERR_INVALID, "mpe_eval_batch: bad sizes or modes");
    if (a->pcap > 1024 || a->gcap > 1024 || a->n_joints > MPE_MAX_JOINTS)
        return fail(ctx, MPE_ERR_CAPACITY, "mpe_eval_batch: pcap %d / gcap %d / joints %d over 1024 / 1024 / %d", a->pcap,
                    a->gcap, a->n_joints, MPE_MAX_JOINTS);
    if (a->n_frames == 0) return MPE_OK;
    if (!a->d_poses || !a->d_flags || !a->d_n_persons || !a->d_gt_xyz || !a->d_gt_joint || !a->d_n_gt_in || !a->d_table ||
        !a->d_assign || !a->d_err || !a->d_invalid || !a->d_n_gt || !a->d_n_res || !a->d_status)
        return fail(ctx, MPE_ERR_INVALID, "mpe_eval_batch: NULL argument");
    HIPCHK(ctx, launch_eval(static_cast<hipStream_t>(stream), *a));
    return MPE_OK;
}

int mpe_track_destroy(mpe_ctx *ctx, mpe_track_state *st) {
    if (!ctx) return MPE_ERR_INVALID;
    if (!st) return fail(ctx, MPE_ERR_INVALID, "mpe_track_destroy: NULL state");
    DeviceGuard dg(ctx);
    for (int i = 0; i < 2; ++i) {
        dev_free(ctx, st->pose[i]);
        dev_free(ctx, st->mask[i]);
        dev_free(ctx, st->id[i]);
        dev_free(ctx, st->child[i]);
    }
    dev_free(ctx, st->count);
    dev_free(ctx, st->ws);
    delete st;
    return MPE_OK;
}

int mpe_track_create(mpe_ctx *ctx, int32_t pcap, int32_t n_joints, int32_t max_gap, int32_t pose_f64, mpe_track_state **out) {
    return create_state(ctx, "mpe_track_create", out, mpe_track_destroy, [&](mpe_track_state *st) {
        if (pcap < 1 || n_joints < 1 || n_joints > MPE_MAX_JOINTS || max_gap < 0 || (pose_f64 & ~1))
            return fail(ctx, MPE_ERR_INVALID, "mpe_track_create: bad sizes or pose type");
        if (pcap > MPE_TRACK_MAX_PERSONS || max_gap > MPE_TRACK_MAX_GAP)
            return fail(ctx, MPE_ERR_CAPACITY, "mpe_track_create: pcap %d / max_gap %d over %d / %d", pcap, max_gap, MPE_TRACK_MAX_PERSONS,
                        MPE_TRACK_MAX_GAP);
        st->pcap = pcap;
        st->J = n_joints;
        st->H = max_gap + 1;
        st->pose_f64 = pose_f64;
        const size_t rows = (size_t)st->H * pcap;
        int rc = MPE_OK;
        for (int i = 0; i < 2 && !rc; ++i) {
            rc = dev_alloc(ctx, &st->pose[i], rows * n_joints * 3);
            if (!rc) rc = dev_alloc(ctx, &st->mask[i], rows);
            if (!rc) rc = dev_alloc(ctx, &st->id[i], rows);
            if (!rc) rc = dev_alloc(ctx, &st->child[i], rows);
        }
        if (!rc) rc = dev_alloc(ctx, &st->count, 2);
        if (!rc) rc = dev_alloc(ctx, &st->ws, 1024);
        if (!rc && track_prepare(pcap) != hipSuccess)
            rc = fail(ctx, MPE_ERR_HIP, "mpe_track_create: the stage kernel cannot have %d KB of LDS", pcap * pcap / 128);
        return rc;
    });
}

int mpe_track_reset(mpe_ctx *ctx, void *stream, mpe_track_state *st) { return reset_state(ctx, "mpe_track_reset", stream, st, launch_track_reset); }

int mpe_track_launches(mpe_ctx *ctx, const mpe_track_state *st, int64_t *n) { return state_launches(ctx, "mpe_track_launches", st, n); }

int mpe_track_batch(mpe_ctx *ctx, void *stream, mpe_track_state *st, const mpe_track_args *a) {
    if (!ctx) return MPE_ERR_INVALID;
    if (!st || !a) return fail(ctx, MPE_ERR_INVALID, "mpe_track_batch: NULL argument");
    DeviceGuard dg(ctx);
    // in front of the shared check, not behind it: a bad gate is MPE_ERR_INVALID whatever the frame count
    if (!(a->gate > 0.0)) return fail(ctx, MPE_ERR_INVALID, "mpe_track_batch: gate %g; it is > 0", a->gate);
    bool run;
    const int rc = check_pose_rows(ctx, "mpe_track_batch", st, a, &run);
    if (rc || !run) return rc;
    if (!a->d_poses || !a->d_flags || !a->d_n_persons || !a->d_track_id || !a->d_link_cost || !a->d_link_gap || !a->d_issued)
        return fail(ctx, MPE_ERR_INVALID, "mpe_track_batch: NULL argument");
    HIPCHK(ctx, launch_track(static_cast<hipStream_t>(stream), st, *a));
    return MPE_OK;
}

int mpe_smooth_destroy(mpe_ctx *ctx, mpe_smooth_state *st) {
    if (!ctx) return MPE_ERR_INVALID;
    if (!st) return fail(ctx, MPE_ERR_INVALID, "mpe_smooth_destroy: NULL state");
    DeviceGuard dg(ctx);
    for (int i = 0; i < 2; ++i) {
        dev_free(ctx, st->pose[i]);
        dev_free(ctx, st->mask[i]);
        dev_free(ctx, st->id[i]);
    }
    delete st;
    return MPE_OK;
}

int mpe_smooth_create(mpe_ctx *ctx, int32_t pcap, int32_t n_joints, int32_t window, int32_t pose_f64, mpe_smooth_state **out) {
    return create_state(ctx, "mpe_smooth_create", out, mpe_smooth_destroy, [&](mpe_smooth_state *st) {
        if (pcap < 1 || n_joints < 1 || n_joints > MPE_MAX_JOINTS || window < 0 || window > MPE_SMOOTH_MAX_WINDOW || (pose_f64 & ~1))
            return fail(ctx, MPE_ERR_INVALID, "mpe_smooth_create: pcap %d / joints %d / window %d / pose_f64 %d; joints 1 .. %d, window 0 .. %d",
                        pcap, n_joints, window, pose_f64, MPE_MAX_JOINTS, MPE_SMOOTH_MAX_WINDOW);
        if (pcap > MPE_TRACK_MAX_PERSONS) return fail(ctx, MPE_ERR_CAPACITY, "mpe_smooth_create: pcap %d over %d", pcap, MPE_TRACK_MAX_PERSONS);
        st->pcap = pcap;
        st->J = n_joints;
        st->W = window;
        st->pose_f64 = pose_f64;
        const size_t rows = (size_t)window * pcap;
        int rc = MPE_OK;
        for (int i = 0; i < 2 && !rc; ++i) {
            rc = dev_alloc(ctx, &st->pose[i], rows * n_joints * 3);
            if (!rc) rc = dev_alloc(ctx, &st->mask[i], rows);
            if (!rc) rc = dev_alloc(ctx, &st->id[i], rows);
            if (!rc && rows && hipMemset(st->id[i], 0xFF, rows * sizeof(int32_t)) != hipSuccess)      // -1: nobody is seen yet
                rc = fail(ctx, MPE_ERR_HIP, "mpe_smooth_create: hipMemset failed");
        }
        return rc;
    });
}

int mpe_smooth_reset(mpe_ctx *ctx, void *stream, mpe_smooth_state *st) { return reset_state(ctx, "mpe_smooth_reset", stream, st, launch_smooth_reset); }

int mpe_smooth_launches(mpe_ctx *ctx, const mpe_smooth_state *st, int64_t *n) { return state_launches(ctx, "mpe_smooth_launches", st, n); }

int mpe_smooth_batch(mpe_ctx *ctx, void *stream, mpe_smooth_state *st, const mpe_smooth_args *a) {
    if (!ctx) return MPE_ERR_INVALID;
    if (!st || !a) return fail(ctx, MPE_ERR_INVALID, "mpe_smooth_batch: NULL argument");
    DeviceGuard dg(ctx);
    if (!(a->lambda >= 0.25 && a->lambda <= 1.0))            // in front of the shared check, as the tracker's gate is
        return fail(ctx, MPE_ERR_INVALID, "mpe_smooth_batch: lambda %g; it is within [0.25, 1]", a->lambda);
    bool run;
    const int rc = check_pose_rows(ctx, "mpe_smooth_batch", st, a, &run);
    if (rc || !run) return rc;
    if (!a->d_poses || !a->d_flags || !a->d_n_persons || !a->d_track_id || !a->d_poses_out || !a->d_flags_out || !a->d_vel || !a->d_n_samples)
        return fail(ctx, MPE_ERR_INVALID, "mpe_smooth_batch: NULL argument");
    if (a->d_poses_out == a->d_poses) return fail(ctx, MPE_ERR_INVALID, "mpe_smooth_batch: d_poses_out is d_poses (the window reads the raw poses)");
    HIPCHK(ctx, launch_smooth(static_cast<hipStream_t>(stream), st, *a));
    return MPE_OK;
}

int mpe_skel_destroy(mpe_ctx *ctx, mpe_skel_state *st) {
    if (!ctx) return MPE_ERR_INVALID;
    if (!st) return fail(ctx, MPE_ERR_INVALID, "mpe_skel_destroy: NULL state");
    DeviceGuard dg(ctx);
    dev_free(ctx, st->bones);
    dev_free(ctx, st->hist);
    dev_free(ctx, st->len);
    dev_free(ctx, st->count);
    dev_free(ctx, st->ctr);
    dev_free(ctx, st->sched);
    dev_free(ctx, st->refine_tab);
    delete st;
    return MPE_OK;
}

int mpe_skel_create(mpe_ctx *ctx, const mpe_skel_config *cfg, mpe_skel_state **out) {
    return create_state(ctx, "mpe_skel_create", out, mpe_skel_destroy, [&](mpe_skel_state *st) {
        if (!cfg || !cfg->bones) return fail(ctx, MPE_ERR_INVALID, "mpe_skel_create: NULL argument");
        const int32_t pcap = cfg->pcap, n_joints = cfg->n_joints, pose_f64 = cfg->pose_f64, tid_cap = cfg->tid_cap, n_bones = cfg->n_bones;
        const int32_t *bones = cfg->bones;
        const double bin_width = cfg->bin_width;
        if (pcap < 1 || n_joints < 1 || n_joints > MPE_MAX_JOINTS || (pose_f64 & ~1) || tid_cap < 1 || n_bones < 1 || n_bones > MPE_SKEL_MAX_BONES)
            return fail(ctx, MPE_ERR_INVALID, "mpe_skel_create: pcap %d / joints %d / pose_f64 %d / tid_cap %d / n_bones %d; joints 1 .. %d, bones 1 .. %d",
                        pcap, n_joints, pose_f64, tid_cap, n_bones, MPE_MAX_JOINTS, MPE_SKEL_MAX_BONES);
        if (!(bin_width > 0.0) || !std::isfinite(bin_width))
            return fail(ctx, MPE_ERR_INVALID, "mpe_skel_create: bin_width %g; it is finite and > 0", bin_width);
        for (int b = 0; b < n_bones; ++b) {
            const int32_t jp = bones[2 * b], jc = bones[2 * b + 1];
            if (jp < 0 || jp >= n_joints || jc < 0 || jc >= n_joints || jp == jc)
                return fail(ctx, MPE_ERR_INVALID, "mpe_skel_create: bone %d is (%d, %d); two different joints within 0 .. %d", b, jp, jc, n_joints - 1);
        }
        if (pcap > MPE_TRACK_MAX_PERSONS) return fail(ctx, MPE_ERR_CAPACITY, "mpe_skel_create: pcap %d over %d", pcap, MPE_TRACK_MAX_PERSONS);
        const uint64_t hist_bytes = (uint64_t)tid_cap * n_bones * MPE_SKEL_BINS * sizeof(uint32_t);
        if (hist_bytes > MPE_SKEL_MAX_HIST_BYTES)
            return fail(ctx, MPE_ERR_CAPACITY, "mpe_skel_create: tid_cap %d x %d bones need %llu bytes of histogram, over %u", tid_cap, n_bones,
                        (unsigned long long)hist_bytes, (unsigned)MPE_SKEL_MAX_HIST_BYTES);
        st->pcap = pcap;
        st->J = n_joints;
        st->pose_f64 = pose_f64;
        st->tid_cap = tid_cap;
        st->n_bones = n_bones;
        st->bin_width = bin_width;
        const size_t pairs = (size_t)tid_cap * n_bones;
        int rc = dev_alloc(ctx, &st->bones, (size_t)n_bones * 2);
        if (!rc) rc = dev_alloc(ctx, &st->hist, pairs * MPE_SKEL_BINS);
        if (!rc) rc = dev_alloc(ctx, &st->len, pairs);
        if (!rc) rc = dev_alloc(ctx, &st->count, pairs);
        if (!rc) rc = dev_alloc(ctx, &st->ctr, 3);
        std::vector<uint32_t> sched;
        skel_schedule(bones, n_bones, &sched, st->steps_upto);
        if (!rc) rc = dev_alloc(ctx, &st->sched, sched.size(), false);
        std::vector<uint32_t> tab;
        st->n_colours = skel_refine_tables(bones, n_bones, n_joints, &tab);
        if (!rc) rc = dev_alloc(ctx, &st->refine_tab, tab.size(), false);
        if (!rc && (hipMemcpy(st->bones, bones, (size_t)n_bones * 2 * sizeof(int32_t), hipMemcpyHostToDevice) != hipSuccess ||
                    hipMemcpy(st->sched, sched.data(), sched.size() * sizeof(uint32_t), hipMemcpyHostToDevice) != hipSuccess ||
                    hipMemcpy(st->refine_tab, tab.data(), tab.size() * sizeof(uint32_t), hipMemcpyHostToDevice) != hipSuccess))
            rc = fail(ctx, MPE_ERR_HIP, "mpe_skel_create: hipMemcpy failed");
        return rc;
    });
}

int mpe_skel_reset(mpe_ctx *ctx, void *stream, mpe_skel_state *st) { return reset_state(ctx, "mpe_skel_reset", stream, st, launch_skel_reset); }

int mpe_skel_launches(mpe_ctx *ctx, const mpe_skel_state *st, int64_t *n) { return state_launches(ctx, "mpe_skel_launches", st, n); }

int mpe_skel_observe_batch(mpe_ctx *ctx, void *stream, mpe_skel_state *st, const mpe_skel_args *a) {
    if (!ctx) return MPE_ERR_INVALID;
    if (!st || !a) return fail(ctx, MPE_ERR_INVALID, "mpe_skel_observe_batch: NULL argument");
    DeviceGuard dg(ctx);
    bool run;
    const int rc = check_pose_rows(ctx, "mpe_skel_observe_batch", st, a, &run);
    if (rc || !run) return rc;
    if (!a->d_poses || !a->d_flags || !a->d_n_persons || !a->d_track_id) return fail(ctx, MPE_ERR_INVALID, "mpe_skel_observe_batch: NULL argument");
    HIPCHK(ctx, launch_skel_observe(static_cast<hipStream_t>(stream), st, *a));
    return MPE_OK;
}

int mpe_skel_update(mpe_ctx *ctx, void *stream, mpe_skel_state *st, int32_t min_samples) {
    if (!ctx) return MPE_ERR_INVALID;
    if (!st) return fail(ctx, MPE_ERR_INVALID, "mpe_skel_update: NULL state");
    DeviceGuard dg(ctx);
    HIPCHK(ctx, launch_skel_update(static_cast<hipStream_t>(stream), st, min_samples));
    return MPE_OK;
}

int mpe_skel_set_lengths(mpe_ctx *ctx, void *stream, mpe_skel_state *st, const double *d_len) {
    if (!ctx) return MPE_ERR_INVALID;
    if (!st || !d_len) return fail(ctx, MPE_ERR_INVALID, "mpe_skel_set_lengths: NULL argument");
    DeviceGuard dg(ctx);
    HIPCHK(ctx, hipMemcpyAsync(st->len, d_len, (size_t)st->tid_cap * st->n_bones * sizeof(double), hipMemcpyDeviceToDevice,
                               static_cast<hipStream_t>(stream)));
    return MPE_OK;
}

int mpe_skel_get_lengths(mpe_ctx *ctx, void *stream, mpe_skel_state *st, double *h_len, int32_t *h_count, int64_t *h_counters, int32_t *h_status) {
    if (!ctx) return MPE_ERR_INVALID;
    if (!st) return fail(ctx, MPE_ERR_INVALID, "mpe_skel_get_lengths: NULL state");
    DeviceGuard dg(ctx);
    hipStream_t s = static_cast<hipStream_t>(stream);
    const size_t pairs = (size_t)st->tid_cap * st->n_bones;
    unsigned long long ctr[3] = {0, 0, 0};
    if (h_len) HIPCHK(ctx, hipMemcpyAsync(h_len, st->len, pairs * sizeof(double), hipMemcpyDeviceToHost, s));
    if (h_count) HIPCHK(ctx, hipMemcpyAsync(h_count, st->count, pairs * sizeof(int32_t), hipMemcpyDeviceToHost, s));
    HIPCHK(ctx, hipMemcpyAsync(ctr, st->ctr, sizeof(ctr), hipMemcpyDeviceToHost, s));
    HIPCHK(ctx, hipStreamSynchronize(s));
    if (h_counters) {
        h_counters[0] = (int64_t)ctr[0];
        h_counters[1] = (int64_t)ctr[1];
    }
    if (h_status) *h_status = (int32_t)ctr[2];
    return MPE_OK;
}

int mpe_skel_fit_batch(mpe_ctx *ctx, void *stream, mpe_skel_state *st, const mpe_skel_args *a) {
    if (!ctx) return MPE_ERR_INVALID;
    if (!st || !a) return fail(ctx, MPE_ERR_INVALID, "mpe_skel_fit_batch: NULL argument");
    DeviceGuard dg(ctx);
    bool run;
    const int rc = check_pose_rows(ctx, "mpe_skel_fit_batch", st, a, &run);
    if (rc) return rc;
    if (a->iters < 1 || a->iters > MPE_SKEL_MAX_ITERS)
        return fail(ctx, MPE_ERR_INVALID, "mpe_skel_fit_batch: iters %d; 1 .. %d", a->iters, MPE_SKEL_MAX_ITERS);
    if (!run) return MPE_OK;
    if (!a->d_poses || !a->d_flags || !a->d_n_persons || !a->d_track_id || !a->d_poses_out || !a->d_err || !a->d_n_bones)
        return fail(ctx, MPE_ERR_INVALID, "mpe_skel_fit_batch: NULL argument");
    if (a->d_poses_out == a->d_poses) return fail(ctx, MPE_ERR_INVALID, "mpe_skel_fit_batch: d_poses_out is d_poses (rows are copied through from the input)");
    HIPCHK(ctx, launch_skel_fit(static_cast<hipStream_t>(stream), st, *a));
    return MPE_OK;
}

int mpe_body_refine_batch(mpe_ctx *ctx, void *stream, mpe_skel_state *st, const mpe_batch *b, const mpe_body_refine_args *a) {
    int rc = check_batch(ctx, b);
    if (rc) return rc;
    if (!st || !a) return fail(ctx, MPE_ERR_INVALID, "mpe_body_refine_batch: NULL argument");
    DeviceGuard dg(ctx);
    bool run;
    rc = check_pose_rows(ctx, "mpe_body_refine_batch", st, a, &run);
    if (rc) return rc;
    bool rows_run;
    rc = check_batch_rows(ctx, "mpe_body_refine_batch", b, a, &rows_run, true, a->d_frame);
    if (rc) return rc;
    if (a->sweeps < 1 || a->sweeps > MPE_SKEL_MAX_ITERS)
        return fail(ctx, MPE_ERR_INVALID, "mpe_body_refine_batch: sweeps %d; 1 .. %d", a->sweeps, MPE_SKEL_MAX_ITERS);
    if (!(a->bone_weight >= 0.0) || !(a->huber_px >= 0.0) || !(a->threshold >= 0.0f))
        return fail(ctx, MPE_ERR_INVALID, "mpe_body_refine_batch: bone_weight %g, huber_px %g and threshold %g must not be negative", a->bone_weight,
                    a->huber_px, (double)a->threshold);
    if (!run || !rows_run) return MPE_OK;
    if (row_inputs_missing(a) || !a->d_track_id || !a->d_poses_out || !a->d_status || !a->d_n_views || !a->d_cost || !a->d_err || !a->d_n_bones)
        return fail(ctx, MPE_ERR_INVALID, "mpe_body_refine_batch: NULL argument");
    if (a->d_poses_out == a->d_poses)
        return fail(ctx, MPE_ERR_INVALID, "mpe_body_refine_batch: d_poses_out is d_poses (rows are copied through from the input)");
    HIPCHK(ctx, launch_skel_refine(static_cast<hipStream_t>(stream), ctx->d_cfg, ctx->cfg.n_cameras, st, *b, *a));
    return MPE_OK;
}

int mpe_relink_destroy(mpe_ctx *ctx, mpe_relink_state *st) {
    if (!ctx) return MPE_ERR_INVALID;
    if (!st) return fail(ctx, MPE_ERR_INVALID, "mpe_relink_destroy: NULL state");
    DeviceGuard dg(ctx);
    dev_free(ctx, st->bones);
    dev_free(ctx, st->canon);
    dev_free(ctx, st->last_pose);
    dev_free(ctx, st->last_mask);
    dev_free(ctx, st->sum);
    dev_free(ctx, st->cnt);
    dev_free(ctx, st->ctr);
    dev_free(ctx, st->row_len);
    dev_free(ctx, st->row_act);
    dev_free(ctx, st->row_id);
    dev_free(ctx, st->table);
    delete st;
    return MPE_OK;
}

int mpe_relink_create(mpe_ctx *ctx, const mpe_relink_config *cfg, mpe_relink_state **out) {
    return create_state(ctx, "mpe_relink_create", out, mpe_relink_destroy, [&](mpe_relink_state *st) {
        char why[400];
        const int bad = relink_check_config(cfg, why, sizeof why);
        if (bad) return fail(ctx, bad, "mpe_relink_create: %s", why);
        st->cfg = relink_copy_config(*cfg, &st->bones_host);
        st->pcap = cfg->pcap;
        st->J = cfg->n_joints;
        st->pose_f64 = cfg->pose_f64;
        st->tid_cap = cfg->tid_cap;
        st->n_bones = cfg->n_bones;
        st->max_frames = cfg->max_frames;
        const size_t cap = (size_t)cfg->tid_cap, nb = (size_t)cfg->n_bones, rows = (size_t)cfg->max_frames * cfg->pcap;
        int rc = dev_alloc(ctx, &st->bones, nb * 2);
        if (!rc) rc = dev_alloc(ctx, &st->canon, 3 * cap);
        if (!rc) rc = dev_alloc(ctx, &st->last_pose, cap * cfg->n_joints * 3);
        if (!rc) rc = dev_alloc(ctx, &st->last_mask, cap);
        if (!rc) rc = dev_alloc(ctx, &st->sum, cap * nb);
        if (!rc) rc = dev_alloc(ctx, &st->cnt, cap * nb);
        if (!rc) rc = dev_alloc(ctx, &st->ctr, 4);
        if (!rc) rc = dev_alloc(ctx, &st->row_len, rows * nb, false);
        if (!rc) rc = dev_alloc(ctx, &st->row_act, rows, false);
        if (!rc) rc = dev_alloc(ctx, &st->row_id, rows, false);
        if (!rc) rc = dev_alloc(ctx, &st->table, (size_t)cfg->pcap * cap, false);
        if (!rc && (hipMemcpy(st->bones, st->bones_host.data(), nb * 2 * sizeof(int32_t), hipMemcpyHostToDevice) != hipSuccess ||
                    hipMemset(st->canon, 0xFF, 3 * cap * sizeof(int32_t)) != hipSuccess))       // -1: no id seen, no record, never present
            rc = fail(ctx, MPE_ERR_HIP, "mpe_relink_create: hipMemcpy failed");
        return rc;
    });
}

int mpe_relink_reset(mpe_ctx *ctx, void *stream, mpe_relink_state *st) { return reset_state(ctx, "mpe_relink_reset", stream, st, launch_relink_reset); }

int mpe_relink_launches(mpe_ctx *ctx, const mpe_relink_state *st, int64_t *n) { return state_launches(ctx, "mpe_relink_launches", st, n); }

int mpe_relink_batch(mpe_ctx *ctx, void *stream, mpe_relink_state *st, const mpe_relink_args *a) {
    if (!ctx) return MPE_ERR_INVALID;
    if (!st || !a) return fail(ctx, MPE_ERR_INVALID, "mpe_relink_batch: NULL argument");
    DeviceGuard dg(ctx);
    bool run;
    const int rc = check_pose_rows(ctx, "mpe_relink_batch", st, a, &run);
    if (rc || !run) return rc;
    if (a->n_frames > st->max_frames)
        return fail(ctx, MPE_ERR_CAPACITY, "mpe_relink_batch: %d frames, the state was made for %d per call", a->n_frames, st->max_frames);
    if (st->frame + a->n_frames > 0x7FFFFFFFll) return fail(ctx, MPE_ERR_CAPACITY, "mpe_relink_batch: the sequence is over 2^31 - 1 frames");
    if (!a->d_poses || !a->d_flags || !a->d_n_persons || !a->d_track_id || !a->d_ids || !a->d_link_cost || !a->d_link_gap)
        return fail(ctx, MPE_ERR_INVALID, "mpe_relink_batch: NULL argument");
    HIPCHK(ctx, launch_relink(static_cast<hipStream_t>(stream), st, *a));
    return MPE_OK;
}

int mpe_relink_read(mpe_ctx *ctx, void *stream, mpe_relink_state *st, int64_t *h_counters, int32_t *h_status) {
    if (!ctx) return MPE_ERR_INVALID;
    if (!st) return fail(ctx, MPE_ERR_INVALID, "mpe_relink_read: NULL state");
    DeviceGuard dg(ctx);
    hipStream_t s = static_cast<hipStream_t>(stream);
    unsigned long long ctr[4] = {0, 0, 0, 0};
    HIPCHK(ctx, hipMemcpyAsync(ctr, st->ctr, sizeof(ctr), hipMemcpyDeviceToHost, s));
    HIPCHK(ctx, hipStreamSynchronize(s));
    if (h_counters)
        for (int i = 0; i < 3; ++i) h_counters[i] = (int64_t)ctr[i];
    if (h_status) *h_status = (int32_t)ctr[3];
    return MPE_OK;
}

int mpe_track_score_destroy(mpe_ctx *ctx, mpe_track_score_state *st) {
    if (!ctx) return MPE_ERR_INVALID;
    if (!st) return fail(ctx, MPE_ERR_INVALID, "mpe_track_score_destroy: NULL state");
    DeviceGuard dg(ctx);
    dev_free(ctx, st->totals);
    dev_free(ctx, st->ident);
    dev_free(ctx, st->pred_count);
    dev_free(ctx, st->table);
    dev_free(ctx, st->rec);
    dev_free(ctx, st->fstat);
    dev_free(ctx, st->mmask);
    dev_free(ctx, st->merr);
    delete st;
    return MPE_OK;
}

int mpe_track_score_create(mpe_ctx *ctx, int32_t pcap, int32_t gcap, int32_t gid_cap, int32_t tid_cap, int32_t max_frames,
                           mpe_track_score_state **out) {
    return create_state(ctx, "mpe_track_score_create", out, mpe_track_score_destroy, [&](mpe_track_score_state *st) {
        if (pcap < 1 || gcap < 1 || gid_cap < 1 || tid_cap < 1 || max_frames < 1)
            return fail(ctx, MPE_ERR_INVALID, "mpe_track_score_create: pcap %d / gcap %d / gid_cap %d / tid_cap %d / max_frames %d, all >= 1", pcap, gcap,
                        gid_cap, tid_cap, max_frames);
        if (pcap > MPE_TRACK_MAX_PERSONS || gcap > MPE_TRACK_MAX_PERSONS)
            return fail(ctx, MPE_ERR_CAPACITY, "mpe_track_score_create: pcap %d / gcap %d over %d", pcap, gcap, MPE_TRACK_MAX_PERSONS);
        if ((int64_t)gid_cap * tid_cap > MPE_TRACK_SCORE_MAX_TABLE)
            return fail(ctx, MPE_ERR_CAPACITY, "mpe_track_score_create: gid_cap %d * tid_cap %d over %d", gid_cap, tid_cap, MPE_TRACK_SCORE_MAX_TABLE);
        st->pcap = pcap;
        st->gcap = gcap;
        st->gid_cap = gid_cap;
        st->tid_cap = tid_cap;
        st->max_frames = max_frames;
        int rc = dev_alloc(ctx, &st->totals, MPE_TS_TOTALS);
        if (!rc) rc = dev_alloc(ctx, &st->ident, (size_t)4 * gid_cap);
        if (!rc) rc = dev_alloc(ctx, &st->pred_count, tid_cap);
        if (!rc) rc = dev_alloc(ctx, &st->table, (size_t)gid_cap * tid_cap);
        if (!rc) rc = dev_alloc(ctx, &st->rec, (size_t)max_frames * gid_cap, false);
        if (!rc) rc = dev_alloc(ctx, &st->fstat, (size_t)max_frames * 8, false);
        if (!rc) rc = dev_alloc(ctx, &st->mmask, (size_t)max_frames * 2, false);
        if (!rc) rc = dev_alloc(ctx, &st->merr, (size_t)max_frames * pcap, false);
        if (!rc && hipMemset(st->ident, 0xFF, gid_cap * sizeof(int32_t)) != hipSuccess)                  // last = -1: no track yet
            rc = fail(ctx, MPE_ERR_HIP, "mpe_track_score_create: hipMemset failed");
        return rc;
    });
}

int mpe_track_score_reset(mpe_ctx *ctx, void *stream, mpe_track_score_state *st) {
    return reset_state(ctx, "mpe_track_score_reset", stream, st, launch_track_score_reset);
}

int mpe_track_score_launches(mpe_ctx *ctx, const mpe_track_score_state *st, int64_t *n) {
    return state_launches(ctx, "mpe_track_score_launches", st, n);
}

int mpe_track_score_batch(mpe_ctx *ctx, void *stream, mpe_track_score_state *st, const mpe_track_score_args *a) {
    if (!ctx) return MPE_ERR_INVALID;
    if (!st || !a) return fail(ctx, MPE_ERR_INVALID, "mpe_track_score_batch: NULL argument");
    DeviceGuard dg(ctx);
    if (a->pcap != st->pcap || a->gcap != st->gcap)
        return fail(ctx, MPE_ERR_INVALID, "mpe_track_score_batch: pcap %d / gcap %d, the state was made for %d / %d", a->pcap, a->gcap, st->pcap,
                    st->gcap);
    if (a->n_frames < 0 || (a->joint_flags & ~1) || !(a->threshold_mm > 0.0))
        return fail(ctx, MPE_ERR_INVALID, "mpe_track_score_batch: n_frames %d / joint_flags %d / threshold_mm %g; the threshold is > 0", a->n_frames,
                    a->joint_flags, a->threshold_mm);
    if (a->n_frames > st->max_frames)
        return fail(ctx, MPE_ERR_CAPACITY, "mpe_track_score_batch: %d frames, the state was made for %d per call", a->n_frames, st->max_frames);
    if (a->n_frames == 0) return MPE_OK;
    if ((!a->joint_flags && !a->d_flags) || !a->d_n_persons || !a->d_track_id || !a->d_assign || !a->d_err || !a->d_n_res || !a->d_n_gt ||
        !a->d_gt_id || !a->d_gt_valid || !a->d_frame_counts || !a->d_match_tid || !a->d_status)
        return fail(ctx, MPE_ERR_INVALID, "mpe_track_score_batch: NULL argument");
    HIPCHK(ctx, launch_track_score(static_cast<hipStream_t>(stream), st, *a));
    return MPE_OK;
}

int mpe_track_score_read(mpe_ctx *ctx, void *stream, mpe_track_score_state *st, int32_t *h_ident, int32_t *h_pred_count, int32_t *h_table) {
    if (!ctx) return MPE_ERR_INVALID;
    if (!st) return fail(ctx, MPE_ERR_INVALID, "mpe_track_score_read: NULL state");
    DeviceGuard dg(ctx);
    hipStream_t s = static_cast<hipStream_t>(stream);
    const size_t G = (size_t)st->gid_cap, T = (size_t)st->tid_cap;
    if (h_ident) HIPCHK(ctx, hipMemcpyAsync(h_ident, st->ident, 4 * G * sizeof(int32_t), hipMemcpyDeviceToHost, s));
    if (h_pred_count) HIPCHK(ctx, hipMemcpyAsync(h_pred_count, st->pred_count, T * sizeof(int32_t), hipMemcpyDeviceToHost, s));
    if (h_table) HIPCHK(ctx, hipMemcpyAsync(h_table, st->table, G * T * sizeof(int32_t), hipMemcpyDeviceToHost, s));
    HIPCHK(ctx, hipStreamSynchronize(s));
    return MPE_OK;
}

int mpe_track_score_result(mpe_ctx *ctx, void *stream, mpe_track_score_state *st, mpe_track_score_totals *out) {
    if (!ctx) return MPE_ERR_INVALID;
    if (!st || !out) return fail(ctx, MPE_ERR_INVALID, "mpe_track_score_result: NULL argument");
    const size_t G = (size_t)st->gid_cap, T = (size_t)st->tid_cap;
    std::vector<int32_t> ident, pred, table;
    try {
        ident.resize(4 * G);
        pred.resize(T);
        table.resize(G * T);
    } catch (const std::bad_alloc &) {
        return fail(ctx, MPE_ERR_NOMEM, "mpe_track_score_result: out of memory");
    }
    int64_t tot[MPE_TS_TOTALS];
    {
        DeviceGuard dg(ctx);
        HIPCHK(ctx, hipMemcpyAsync(tot, st->totals, sizeof(tot), hipMemcpyDeviceToHost, static_cast<hipStream_t>(stream)));
    }
    const int rc = mpe_track_score_read(ctx, stream, st, ident.data(), pred.data(), table.data());
    if (rc) return rc;
    mpe_track_score_totals r{};
    r.frames = tot[0]; r.n_gt = tot[1]; r.n_pred = tot[2]; r.tp = tot[3]; r.fp = tot[4]; r.fn = tot[5]; r.idsw = tot[6]; r.frag = tot[7];
    r.ignored = tot[8]; r.over_ids = tot[9];
    std::memcpy(&r.err_sum, &tot[10], sizeof(double));
    r.status = (int32_t)tot[11];
    for (size_t o = 0; o < G; ++o) {
        const int64_t present = ident[G + o], matched = ident[2 * G + o];
        if (present <= 0) continue;
        ++r.n_ids;
        if (5 * matched >= 4 * present) ++r.mt;
        else if (5 * matched < present) ++r.ml;
        else ++r.pt;
    }
    for (size_t h = 0; h < T; ++h) r.n_tracks += pred[h] > 0;
    r.idtp = assign_int_max(table.data(), G, T, T);             // host work, once per recording (assign_int.h)
    const double nan = std::nan("");
    r.mota = r.n_gt ? 1.0 - (double)(r.fn + r.fp + r.idsw) / (double)r.n_gt : nan;
    r.motp_mm = r.tp ? r.err_sum * 1000. / (double)r.tp : nan;
    r.idp = r.n_pred ? (double)r.idtp / (double)r.n_pred : nan;
    r.idr = r.n_gt ? (double)r.idtp / (double)r.n_gt : nan;
    r.idf1 = (r.n_gt + r.n_pred) ? 2.0 * (double)r.idtp / (double)(r.n_gt + r.n_pred) : nan;
    *out = r;
    return MPE_OK;
}

int mpe_reproject_batch(mpe_ctx *ctx, void *stream, const mpe_batch *b, const mpe_reproject_args *a) {
    int rc = check_batch(ctx, b);
    if (rc) return rc;
    if (!a) return fail(ctx, MPE_ERR_INVALID, "mpe_reproject_batch: NULL argument");
    DeviceGuard dg(ctx);
    bool run;
    rc = check_batch_rows(ctx, "mpe_reproject_batch", b, a, &run);
    if (rc || !run) return rc;
    if (row_inputs_missing(a) || !a->d_res) return fail(ctx, MPE_ERR_INVALID, "mpe_reproject_batch: NULL argument");
    HIPCHK(ctx, launch_reproject(static_cast<hipStream_t>(stream), ctx->d_cfg, ctx->cfg.n_cameras, *b, *a));
    return MPE_OK;
}

int mpe_refine_batch(mpe_ctx *ctx, void *stream, const mpe_batch *b, const mpe_refine_args *a) {
    int rc = check_batch(ctx, b);
    if (rc) return rc;
    if (!a) return fail(ctx, MPE_ERR_INVALID, "mpe_refine_batch: NULL argument");
    DeviceGuard dg(ctx);
    bool run;
    rc = check_batch_rows(ctx, "mpe_refine_batch", b, a, &run);
    if (rc) return rc;
    if (a->max_iters < 1 || a->max_iters > MPE_REFINE_MAX_ITERS)
        return fail(ctx, MPE_ERR_INVALID, "mpe_refine_batch: max_iters %d outside 1..%d", a->max_iters, MPE_REFINE_MAX_ITERS);
    if (!(a->step_tol >= 0.0) || !(a->huber_px >= 0.0))
        return fail(ctx, MPE_ERR_INVALID, "mpe_refine_batch: step_tol %g and huber_px %g must not be negative", a->step_tol, a->huber_px);
    if (!run) return MPE_OK;
    if (row_inputs_missing(a) || !a->d_poses_out || !a->d_status || !a->d_cost0 || !a->d_cost1 || !a->d_iters || !a->d_n_views)
        return fail(ctx, MPE_ERR_INVALID, "mpe_refine_batch: NULL argument");
    HIPCHK(ctx, launch_refine(static_cast<hipStream_t>(stream), ctx->d_cfg, ctx->cfg.n_cameras, *b, *a));
    return MPE_OK;
}

int mpe_posecov_batch(mpe_ctx *ctx, void *stream, const mpe_batch *b, const mpe_posecov_args *a) {
    int rc = check_batch(ctx, b);
    if (rc) return rc;
    if (!a) return fail(ctx, MPE_ERR_INVALID, "mpe_posecov_batch: NULL argument");
    DeviceGuard dg(ctx);
    bool run;
    rc = check_batch_rows(ctx, "mpe_posecov_batch", b, a, &run);
    if (rc) return rc;
    if (!(a->sigma_px > 0.0) || !(a->sigma_px < HUGE_VAL))
        return fail(ctx, MPE_ERR_INVALID, "mpe_posecov_batch: sigma_px %g must be positive and finite", a->sigma_px);
    if (!(a->gate_m >= 0.0) || !(a->huber_px >= 0.0))
        return fail(ctx, MPE_ERR_INVALID, "mpe_posecov_batch: gate_m %g and huber_px %g must not be negative", a->gate_m, a->huber_px);
    if (a->d_flags_out && !a->joint_flags)
        return fail(ctx, MPE_ERR_INVALID, "mpe_posecov_batch: d_flags_out needs joint_flags 1 (the gate clears joints, not persons)");
    if (!run) return MPE_OK;
    if (row_inputs_missing(a) || !a->d_cov || !a->d_sigma || !a->d_status || !a->d_n_views)
        return fail(ctx, MPE_ERR_INVALID, "mpe_posecov_batch: NULL argument");
    HIPCHK(ctx, launch_posecov(static_cast<hipStream_t>(stream), ctx->d_cfg, ctx->cfg.n_cameras, *b, *a));
    return MPE_OK;
}

int mpe_regroup_batch(mpe_ctx *ctx, void *stream, const mpe_batch *b, const mpe_regroup_args *a) {
    int rc = check_batch(ctx, b);
    if (rc) return rc;
    if (!a) return fail(ctx, MPE_ERR_INVALID, "mpe_regroup_batch: NULL argument");
    DeviceGuard dg(ctx);
    bool run;
    rc = check_batch_rows(ctx, "mpe_regroup_batch", b, a, &run);
    if (rc) return rc;
    if (a->pcap > MPE_REGROUP_MAX_PERSONS)
        return fail(ctx, MPE_ERR_CAPACITY, "mpe_regroup_batch: pcap %d over %d", a->pcap, MPE_REGROUP_MAX_PERSONS);
    if (!(a->gate_px > 0.0) || !(a->clip_px >= 0.0))
        return fail(ctx, MPE_ERR_INVALID, "mpe_regroup_batch: gate_px %g must be positive and clip_px %g must not be negative", a->gate_px,
                    a->clip_px);
    if (a->min_joints < 1 || a->min_joints > ctx->cfg.n_joints)
        return fail(ctx, MPE_ERR_INVALID, "mpe_regroup_batch: min_joints %d outside 1..%d", a->min_joints, ctx->cfg.n_joints);
    if (a->flags == 0 || (a->flags & ~(uint32_t)(MPE_REGROUP_RELEASE | MPE_REGROUP_ATTACH)))
        return fail(ctx, MPE_ERR_INVALID, "mpe_regroup_batch: flags %u must be MPE_REGROUP_RELEASE, MPE_REGROUP_ATTACH or both", a->flags);
    if (!run) return MPE_OK;
    if (row_inputs_missing(a)) return fail(ctx, MPE_ERR_INVALID, "mpe_regroup_batch: NULL argument");
    // d_cost is [n_heads][pcap]: a batch without heads has no table to point at, and no frame of it touches one
    if (!a->d_persons_out || !a->d_change || !a->d_n_views || (!a->d_cost && b->n_heads > 0) || !a->d_counts || !a->d_status)
        return fail(ctx, MPE_ERR_INVALID, "mpe_regroup_batch: NULL output");
    HIPCHK(ctx, launch_regroup(static_cast<hipStream_t>(stream), ctx->d_cfg, ctx->cfg.n_cameras, ctx->cfg.min_views,
                               ctx->cfg.max_heads_per_frame, ctx->d_status, *b, *a));
    return MPE_OK;
}

int mpe_consolidate_batch(mpe_ctx *ctx, void *stream, const mpe_batch *b, const mpe_consolidate_args *a) {
    int rc = check_batch(ctx, b);
    if (rc) return rc;
    if (!a) return fail(ctx, MPE_ERR_INVALID, "mpe_consolidate_batch: NULL argument");
    DeviceGuard dg(ctx);
    const int J = ctx->cfg.n_joints;
    bool run;
    rc = check_batch_rows(ctx, "mpe_consolidate_batch", b, a, &run);
    if (rc) return rc;
    if (a->pcap > MPE_REGROUP_MAX_PERSONS)
        return fail(ctx, MPE_ERR_CAPACITY, "mpe_consolidate_batch: pcap %d over %d", a->pcap, MPE_REGROUP_MAX_PERSONS);
    if (!(a->merge_m > 0.0) || !(a->found_m > 0.0) || !(a->clip_m >= 0.0))
        return fail(ctx, MPE_ERR_INVALID, "mpe_consolidate_batch: merge_m %g and found_m %g must be positive and clip_m %g must not be negative",
                    a->merge_m, a->found_m, a->clip_m);
    if (a->min_joints < 1 || a->min_joints > J) return fail(ctx, MPE_ERR_INVALID, "mpe_consolidate_batch: min_joints %d outside 1..%d", a->min_joints, J);
    if (a->found_min_views < 2) return fail(ctx, MPE_ERR_INVALID, "mpe_consolidate_batch: found_min_views %d must be at least 2", a->found_min_views);
    if (a->fcap < 1 || a->fcap > MPE_CONSOLIDATE_MAX_FREE)
        return fail(ctx, MPE_ERR_INVALID, "mpe_consolidate_batch: fcap %d outside 1..%d", a->fcap, MPE_CONSOLIDATE_MAX_FREE);
    if (a->fcap * (3 * J + 1) > MPE_CONSOLIDATE_RAY_DOUBLES)
        return fail(ctx, MPE_ERR_CAPACITY, "mpe_consolidate_batch: fcap %d with %d joints over %d ray doubles", a->fcap, J, MPE_CONSOLIDATE_RAY_DOUBLES);
    if (a->flags == 0 || (a->flags & ~(uint32_t)(MPE_CONSOLIDATE_MERGE | MPE_CONSOLIDATE_FOUND)))
        return fail(ctx, MPE_ERR_INVALID, "mpe_consolidate_batch: flags %u must be MPE_CONSOLIDATE_MERGE, MPE_CONSOLIDATE_FOUND or both", a->flags);
    if (!run) return MPE_OK;
    if (row_inputs_missing(a)) return fail(ctx, MPE_ERR_INVALID, "mpe_consolidate_batch: NULL argument");
    if (!a->d_persons_out || !a->d_n_persons_out || !a->d_change || !a->d_n_views || !a->d_dist || !a->d_pair || !a->d_free || !a->d_counts ||
        !a->d_status)
        return fail(ctx, MPE_ERR_INVALID, "mpe_consolidate_batch: NULL output");
    HIPCHK(ctx, launch_consolidate(static_cast<hipStream_t>(stream), ctx->d_cfg, ctx->cfg.n_cameras, ctx->cfg.max_heads_per_frame,
                                   ctx->d_status, *b, *a));
    return MPE_OK;
}

static int geom_checks(mpe_ctx *ctx, const mpe_geom_args *a, const char *who) {
    if (!a) return fail(ctx, MPE_ERR_INVALID, "%s: NULL argument", who);
    if (!(a->sigma_m > 0.0) || !(a->clip_m >= 0.0))
        return fail(ctx, MPE_ERR_INVALID, "%s: sigma_m %g must be positive and clip_m %g must not be negative", who, a->sigma_m, a->clip_m);
    if (a->min_joints < 1 || a->min_joints > ctx->cfg.n_joints)
        return fail(ctx, MPE_ERR_INVALID, "%s: min_joints %d outside 1..%d", who, a->min_joints, ctx->cfg.n_joints);
    if (!(a->min_conf >= 0.0f)) return fail(ctx, MPE_ERR_INVALID, "%s: min_conf %g must not be negative", who, (double)a->min_conf);
    return MPE_OK;
}

int mpe_geom_scores_batch(mpe_ctx *ctx, void *stream, const mpe_batch *b, const mpe_geom_args *a) {
    int rc = check_batch(ctx, b);
    if (rc) return rc;
    DeviceGuard dg(ctx);
    if ((rc = geom_checks(ctx, a, "mpe_geom_scores_batch"))) return rc;
    if (b->n_frames == 0) return MPE_OK;
    if (!a->d_scores) return fail(ctx, MPE_ERR_INVALID, "mpe_geom_scores_batch: NULL output");
    hipStream_t s = static_cast<hipStream_t>(stream);
    if ((rc = gat_topology(ctx, s, b))) return rc;
    HIPCHK(ctx, launch_geom(s, ctx->d_cfg, ctx->cfg.n_cameras, ctx->cfg.n_joints, *b, ctx->en_pair, ctx->cfg.max_heads_per_frame, ctx->x_m_cap,
                            *a, a->d_scores, ctx->geom_rays));
    return MPE_OK;
}

int mpe_geom_match_batch(mpe_ctx *ctx, void *stream, const mpe_batch *b, const mpe_geom_args *a, int32_t *d_persons,
                         int32_t *d_n_persons) {
    int rc = check_batch(ctx, b);
    if (rc) return rc;
    DeviceGuard dg(ctx);
    if ((rc = geom_checks(ctx, a, "mpe_geom_match_batch"))) return rc;
    if (b->n_frames == 0) return MPE_OK;
    if (!d_persons || !d_n_persons) return fail(ctx, MPE_ERR_INVALID, "mpe_geom_match_batch: NULL output");
    hipStream_t s = static_cast<hipStream_t>(stream);
    float *scores = a->d_scores ? a->d_scores : ctx->scores_tmp;
    if ((rc = gat_topology(ctx, s, b))) return rc;
    HIPCHK(ctx, launch_geom(s, ctx->d_cfg, ctx->cfg.n_cameras, ctx->cfg.n_joints, *b, ctx->en_pair, ctx->cfg.max_heads_per_frame, ctx->x_m_cap,
                            *a, scores, ctx->geom_rays));
    HIPCHK(ctx, launch_cluster(s, ctx->d_cfg, *b, ctx->en_pair, scores, ctx->cfg.max_persons_per_frame, ctx->cfg.max_heads_per_frame,
                               ctx->cl_keys, ctx->cl_keys_per_frame, ctx->cl_scratch, ctx->cl_scratch_per_frame, d_persons, d_n_persons));
    return MPE_OK;
}

int mpe_residual_stats(mpe_ctx *ctx, void *stream, const mpe_residual_stats_args *a) {
    if (!ctx) return MPE_ERR_INVALID;
    if (!a) return fail(ctx, MPE_ERR_INVALID, "mpe_residual_stats: NULL argument");
    DeviceGuard dg(ctx);
    if (a->n_buffers < 0 || a->n_joints < 1 || a->n_joints > MPE_MAX_JOINTS || !a->d_count || !a->d_nonfinite || !a->d_sum || !a->d_mid ||
        (a->n_buffers && (!a->d_res || !a->n_groups)))
        return fail(ctx, MPE_ERR_INVALID, "mpe_residual_stats: bad argument");
    long long total = 0;
    for (int i = 0; i < a->n_buffers; ++i) {
        if (a->n_groups[i] < 0 || (a->n_groups[i] && !a->d_res[i])) return fail(ctx, MPE_ERR_INVALID, "mpe_residual_stats: bad buffer %d", i);
        if (a->n_groups[i] > (1ll << 31) / a->n_joints) return fail(ctx, MPE_ERR_CAPACITY, "mpe_residual_stats: buffer %d too large", i);
        total += (long long)a->n_groups[i] * a->n_joints;
    }
    if (total >= (1ll << 32)) return fail(ctx, MPE_ERR_CAPACITY, "mpe_residual_stats: more than 2^32 - 1 entries per camera");
    HIPCHK(ctx, launch_residual_stats(static_cast<hipStream_t>(stream), ctx->cfg.n_cameras, *a, ctx->res_state, ctx->res_hist, ctx->res_partial));
    return MPE_OK;
}

int mpe_partition_labels(mpe_ctx *ctx, void *stream, const mpe_batch *b, const mpe_partition_labels_args *a) {
    int rc = check_batch(ctx, b);
    if (rc) return rc;
    if (!a) return fail(ctx, MPE_ERR_INVALID, "mpe_partition_labels: NULL argument");
    DeviceGuard dg(ctx);
    if (a->n_frames != b->n_frames || a->pcap < 1 || a->hcap < 1) return fail(ctx, MPE_ERR_INVALID, "mpe_partition_labels: bad sizes");
    if (b->n_frames == 0) return MPE_OK;
    if (!a->d_persons || !a->d_n_persons || !a->d_labels || !a->d_count || !a->d_status)
        return fail(ctx, MPE_ERR_INVALID, "mpe_partition_labels: NULL argument");
    HIPCHK(ctx, launch_partition_labels(static_cast<hipStream_t>(stream), ctx->cfg.n_cameras, *b, *a));
    return MPE_OK;
}

int mpe_group_bodies(mpe_ctx *ctx, void *stream, const mpe_group_bodies_args *a) {
    if (!ctx) return MPE_ERR_INVALID;
    if (!a) return fail(ctx, MPE_ERR_INVALID, "mpe_group_bodies: NULL argument");
    DeviceGuard dg(ctx);
    if (a->n_frames < 0 || a->scap < 1 || a->kcap < 1) return fail(ctx, MPE_ERR_INVALID, "mpe_group_bodies: bad sizes");
    if (a->kcap > MPE_PART_MAX_KEYS) return fail(ctx, MPE_ERR_CAPACITY, "mpe_group_bodies: %d joint keys over %d", a->kcap, MPE_PART_MAX_KEYS);
    if (a->n_frames == 0) return MPE_OK;
    if (!a->d_xyz || !a->d_mask || !a->d_nkeys || !a->d_order || !a->d_m1 || !a->d_n || !a->d_labels || !a->d_n_groups || !a->d_skip ||
        !a->d_status)
        return fail(ctx, MPE_ERR_INVALID, "mpe_group_bodies: NULL argument");
    HIPCHK(ctx, launch_group_bodies(static_cast<hipStream_t>(stream), *a));
    return MPE_OK;
}

int mpe_set_log_table(mpe_ctx *ctx, const double *table, int32_t n) {
    if (!ctx) return MPE_ERR_INVALID;
    DeviceGuard dg(ctx);
    if (!table || n < 1) return fail(ctx, MPE_ERR_INVALID, "mpe_set_log_table: bad argument");
    if (ctx->log_table) return fail(ctx, MPE_ERR_STATE, "the table of logarithms is set once per context");
    int rc = dev_alloc(ctx, &ctx->log_table, (size_t)n, false);
    if (rc) return rc;
    HIPCHK(ctx, hipMemcpy(ctx->log_table, table, (size_t)n * sizeof(double), hipMemcpyHostToDevice));
    ctx->n_log = n;
    return MPE_OK;
}

int mpe_partition_scores(mpe_ctx *ctx, void *stream, const mpe_partition_scores_args *a) {
    if (!ctx) return MPE_ERR_INVALID;
    if (!a) return fail(ctx, MPE_ERR_INVALID, "mpe_partition_scores: NULL argument");
    DeviceGuard dg(ctx);
    if (a->n_frames < 0 || a->ld_true < 1 || a->ld_pred < 1) return fail(ctx, MPE_ERR_INVALID, "mpe_partition_scores: bad sizes");
    if (ctx->n_log < 1) return fail(ctx, MPE_ERR_STATE, "mpe_partition_scores: no table of logarithms (mpe_set_log_table)");
    if (a->n_frames == 0) return MPE_OK;
    if (!a->d_labels_true || !a->d_labels_pred || !a->d_count || !a->d_scores || !a->d_status)
        return fail(ctx, MPE_ERR_INVALID, "mpe_partition_scores: NULL argument");
    HIPCHK(ctx, launch_partition_scores(static_cast<hipStream_t>(stream), *a, ctx->log_table, ctx->n_log));
    return MPE_OK;
}

int mpe_dlt_pairs(mpe_ctx *ctx, void *stream, const double *d_pts, const int32_t *d_cams, int32_t n, double *d_out) {
    if (!ctx) return MPE_ERR_INVALID;
    DeviceGuard dg(ctx);
    if (!d_pts || !d_cams || !d_out || n < 0) return fail(ctx, MPE_ERR_INVALID, "mpe_dlt_pairs: bad argument");
    HIPCHK(ctx, launch_dlt_pairs(static_cast<hipStream_t>(stream), ctx->d_cfg, d_pts, d_cams, n, d_out));
    return MPE_OK;
}

int mpe_set_precision(mpe_ctx *ctx, int32_t gat_mode, int32_t mlp_mode) {
    if (!ctx) return MPE_ERR_INVALID;
    DeviceGuard dg(ctx);
    if (gat_mode < 0 || gat_mode > 6 || mlp_mode < 0 || mlp_mode > 5)
        return fail(ctx, MPE_ERR_INVALID, "precision modes: GAT 0..6, MLP 0..5");
    // GAT modes 4 / 5: modes 0 / 1 with the GEMMs of layers >= 1 in the split-bf16 form (4 = the default); 6 = mode 3 likewise
    // (fp16 rows: from the split tile kernel's coefficient epilogue where gat_gemm_form finds it applicable, the fp32 MFMA otherwise)
    ctx->gat_split = gat_mode >= 4;
    if (gat_mode >= 4) gat_mode = gat_mode == 4 ? 0 : gat_mode == 5 ? 1 : 3;
    ctx->gat_acc64 = gat_mode == 1;
    ctx->gat_reduced = gat_mode == 2;
    ctx->gat_attn_fp16 = gat_mode == 3;
    ctx->mlp_mode = static_cast<MlpMode>(mlp_mode);      // (which form each mode runs on: gemm_form.h)
    return MPE_OK;
}

int mpe_profile_enable(mpe_ctx *ctx, int32_t on) {
    if (!ctx) return MPE_ERR_INVALID;
    DeviceGuard dg(ctx);
    ctx->profiling = on != 0;
    if (on == 1) ctx->prof_used = 0;        // 1 = start afresh, 2 = resume (keep the records), 0 = pause / off
    return MPE_OK;
}

int mpe_profile_read(mpe_ctx *ctx, double *gemm_ms, double *gemm_flop, int64_t *gemm_launches, double *total_ms) {
    if (!ctx) return MPE_ERR_INVALID;
    DeviceGuard dg(ctx);
    HIPCHK(ctx, hipDeviceSynchronize());
    int32_t dev_m = 0;
    HIPCHK(ctx, hipMemcpy(&dev_m, ctx->mlp_count, sizeof dev_m, hipMemcpyDeviceToHost));
    double ms[3] = {0, 0, 0}, flop[3] = {0, 0, 0};
    int64_t cnt[3] = {0, 0, 0};
    for (size_t i = 0; i < ctx->prof_used; ++i) {
        if (ctx->prof[i].kind == 3) continue;        // f64 matrix-pipe launches (MLP mode 5): not part of the roofline figures
        const int k = ctx->prof[i].kind == 1 ? 1 : ctx->prof[i].kind == 2 ? 2 : 0;       // fp32 MFMA | split-bf16 | plain bf16 (reduced modes)
        float t = 0;
        if (hipEventElapsedTime(&t, ctx->prof[i].start, ctx->prof[i].stop) == hipSuccess) ms[k] += t;
        flop[k] += ctx->prof[i].flop;
        if (ctx->prof[i].dev_n) flop[k] += 2.0 * dev_m * (double)ctx->prof[i].dev_n * ctx->prof[i].dev_k;
        ++cnt[k];
    }
    if (gemm_ms) *gemm_ms = ms[0];
    if (gemm_flop) *gemm_flop = flop[0];
    if (gemm_launches) *gemm_launches = cnt[0];
    ctx->sb_ms = ms[1];
    ctx->sb_flop = flop[1];
    ctx->sb_launches = cnt[1];
    ctx->bf_ms = ms[2];
    ctx->bf_flop = flop[2];
    ctx->bf_launches = cnt[2];
    if (total_ms) *total_ms = 0;
    ctx->prof_used = 0;
    return MPE_OK;
}

int mpe_profile_read_split(mpe_ctx *ctx, double *ms, double *flop, int64_t *launches) {
    if (!ctx) return MPE_ERR_INVALID;
    if (ms) *ms = ctx->sb_ms;
    if (flop) *flop = ctx->sb_flop;
    if (launches) *launches = ctx->sb_launches;
    return MPE_OK;
}

int mpe_profile_read_bf16(mpe_ctx *ctx, double *ms, double *flop, int64_t *launches) {
    if (!ctx) return MPE_ERR_INVALID;
    if (ms) *ms = ctx->bf_ms;
    if (flop) *flop = ctx->bf_flop;
    if (launches) *launches = ctx->bf_launches;
    return MPE_OK;
}

int mpe_l0_attention_launches(mpe_ctx *ctx, int64_t *n) {
    if (!ctx || !n) return MPE_ERR_INVALID;
    *n = ctx->l0_attention_launches;
    return MPE_OK;
}

}  // extern "C"

// ---- calibration and camera fit (normal_sums.h sums on the device; the step is host work, once per pass) ----
// mpe_calib_* and mpe_camfit_* are one algorithm at two sizes.  What they share is written once below, over normal_state
// and a family's host half; `who` is the entry point's name, the prefix of its messages.
#include "camfit_solve.h"
#include "normal_sums.h"

template <typename Cam, int SUMS, int WIDTH>
struct normal_host {
    Cam cam[MPE_MAX_CAMERAS];
    double cams[MPE_MAX_CAMERAS * WIDTH];            // staging of the trial set for the copy to the device
    double sums[MPE_MAX_CAMERAS * SUMS];
    int64_t n_obs[MPE_MAX_CAMERAS], n_skipped[MPE_MAX_CAMERAS];
};
struct mpe_calib_host : normal_host<calib_cam, MPE_CALIB_SUMS, CALIB_CAM> {};
struct mpe_camfit_host : normal_host<camfit_cam, MPE_CAMFIT_SUMS, CAMFIT_CAM> {};

namespace {

// a camera's trial set as the device holds it
void stage_trial(const calib_cam &cam, double *d) { std::memcpy(d, cam.Et, sizeof cam.Et); }

void stage_trial(const camfit_cam &cam, double *d) {
    const camfit_set &t = cam.t;
    std::memcpy(d, t.E, sizeof t.E);
    std::memcpy(d + 12, t.dist, sizeof t.dist);
    for (int i = 0; i < 4; ++i) d[17 + i] = (double)t.k[i];
}

// the trial sets to the staging buffer and from there to the device
template <typename S>
int normal_upload(mpe_ctx *ctx, hipStream_t s, S *st) {
    for (int c = 0; c < st->V; ++c) stage_trial(st->host->cam[c], st->host->cams + (size_t)c * st->cam_width);
    HIPCHK(ctx, hipMemcpyAsync(st->cams, st->host->cams, (size_t)st->V * st->cam_width * sizeof(double), hipMemcpyHostToDevice, s));
    return MPE_OK;
}

// after every camera's *_cam_start: the trial set on the device, the sums zeroed
template <typename S>
int normal_start(mpe_ctx *ctx, hipStream_t s, S *st) {
    int rc = normal_upload(ctx, s, st);
    if (rc) return rc;
    HIPCHK(ctx, launch_normal_clear(s, st));
    HIPCHK(ctx, hipStreamSynchronize(s));            // the staging buffer is the state's own: the next call may rewrite it
    return MPE_OK;
}

template <typename S>
int normal_fetch(mpe_ctx *ctx, hipStream_t s, S *st) {
    auto *h = st->host;
    HIPCHK(ctx, hipMemcpyAsync(h->sums, st->acc, (size_t)st->V * st->n_sums * sizeof(double), hipMemcpyDeviceToHost, s));
    HIPCHK(ctx, hipMemcpyAsync(h->n_obs, st->n_obs, (size_t)st->V * sizeof(int64_t), hipMemcpyDeviceToHost, s));
    HIPCHK(ctx, hipMemcpyAsync(h->n_skipped, st->n_skipped, (size_t)st->V * sizeof(int64_t), hipMemcpyDeviceToHost, s));
    HIPCHK(ctx, hipStreamSynchronize(s));
    return MPE_OK;
}

template <typename S>
int normal_destroy(mpe_ctx *ctx, const char *who, S *st) {
    if (!ctx) return MPE_ERR_INVALID;
    if (!st) return fail(ctx, MPE_ERR_INVALID, "%s: NULL state", who);
    DeviceGuard dg(ctx);
    dev_free(ctx, st->cams);
    dev_free(ctx, st->acc);
    dev_free(ctx, st->n_obs);
    dev_free(ctx, st->n_skipped);
    dev_free(ctx, st->S);
    delete st->host;
    delete st;
    return MPE_OK;
}

// the host half and the device arrays of a new state
template <typename S, typename Host>
int normal_alloc(mpe_ctx *ctx, const char *who, S *st, Host *host, int n_sums, int cam_width) {
    if (!(st->host = host)) return fail(ctx, MPE_ERR_NOMEM, "%s: out of memory", who);
    st->V = ctx->cfg.n_cameras;
    st->max_frames = ctx->cfg.max_frames;
    st->n_sums = n_sums;
    st->cam_width = cam_width;
    int rc = dev_alloc(ctx, &st->cams, (size_t)st->V * cam_width);
    if (!rc) rc = dev_alloc(ctx, &st->acc, (size_t)st->V * n_sums);
    if (!rc) rc = dev_alloc(ctx, &st->n_obs, st->V);
    if (!rc) rc = dev_alloc(ctx, &st->n_skipped, st->V);
    if (!rc) rc = dev_alloc(ctx, &st->S, normal_workspace_doubles(st), false);
    return rc;
}

int normal_batch(mpe_ctx *ctx, const char *who, void *stream, normal_state *st, const mpe_batch *b, const mpe_calib_args *a,
                 hipError_t (*launch)(hipStream_t, const mpe::DevCfg *, normal_state *, const mpe_batch &, const mpe_calib_args &)) {
    int rc = check_batch(ctx, b);
    if (rc) return rc;
    if (!st || !a) return fail(ctx, MPE_ERR_INVALID, "%s: NULL argument", who);
    DeviceGuard dg(ctx);
    bool run;
    rc = check_batch_rows(ctx, who, b, a, &run);
    if (rc) return rc;
    if (!(a->huber_px >= 0.0)) return fail(ctx, MPE_ERR_INVALID, "%s: huber_px %g must not be negative", who, a->huber_px);
    if (st->V != ctx->cfg.n_cameras || b->n_frames > st->max_frames) return fail(ctx, MPE_ERR_INVALID, "%s: the state belongs to another context", who);
    if (!run) return MPE_OK;
    if (row_inputs_missing(a)) return fail(ctx, MPE_ERR_INVALID, "%s: NULL argument", who);
    HIPCHK(ctx, launch(static_cast<hipStream_t>(stream), ctx->d_cfg, st, *b, *a));
    return MPE_OK;
}

template <typename S>
int normal_read(mpe_ctx *ctx, const char *who, void *stream, S *st, double *sums, int64_t *n_obs, int64_t *n_skipped) {
    if (!ctx) return MPE_ERR_INVALID;
    if (!st) return fail(ctx, MPE_ERR_INVALID, "%s: NULL state", who);
    DeviceGuard dg(ctx);
    int rc = normal_fetch(ctx, static_cast<hipStream_t>(stream), st);
    if (rc) return rc;
    if (sums) std::memcpy(sums, st->host->sums, (size_t)st->V * st->n_sums * sizeof(double));
    if (n_obs) std::memcpy(n_obs, st->host->n_obs, (size_t)st->V * sizeof(int64_t));
    if (n_skipped) std::memcpy(n_skipped, st->host->n_skipped, (size_t)st->V * sizeof(int64_t));
    return MPE_OK;
}

// The step after the family's checks of its arguments: the sums read and zeroed, cam_step(cam, sums, n_obs, held) per
// camera, the trial sets to the device, and what the two reports share.
template <typename S, typename Report, typename Step>
int normal_step(mpe_ctx *ctx, const char *who, void *stream, S *st, uint32_t hold_mask, Report *report, Step cam_step) {
    DeviceGuard dg(ctx);
    hipStream_t s = static_cast<hipStream_t>(stream);
    auto *h = st->host;
    int rc = normal_fetch(ctx, s, st);
    if (rc) return rc;
    HIPCHK(ctx, launch_normal_clear(s, st));
    for (int c = 0; c < st->V; ++c)
        if (h->cam[c].passes > 0 && h->n_obs[c] != h->cam[c].n_obs) {
            HIPCHK(ctx, hipStreamSynchronize(s));
            return fail(ctx, MPE_ERR_INVALID, "%s: the passes did not see the same data (camera %d: %lld observations, %lld in the first pass)", who, c,
                        (long long)h->n_obs[c], (long long)h->cam[c].n_obs);
        }
    int all_done = 1;
    for (int c = 0; c < st->V; ++c) {
        cam_step(&h->cam[c], h->sums + (size_t)c * st->n_sums, h->n_obs[c], (hold_mask >> c) & 1u);
        all_done &= calib_lm_done(&h->cam[c]);
    }
    rc = normal_upload(ctx, s, st);
    if (rc) return rc;
    HIPCHK(ctx, hipStreamSynchronize(s));
    if (!report) return MPE_OK;
    std::memset(report, 0, sizeof *report);
    report->n_cameras = st->V;
    report->all_done = all_done;
    for (int c = 0; c < st->V; ++c) {
        const auto &cam = h->cam[c];
        auto &r = report->cam[c];
        r.status = cam.status;
        r.passes = cam.passes;
        r.n_obs = h->n_obs[c];
        r.n_skipped = h->n_skipped[c];
        r.cost_start = cam.cost_start;
        r.cost = cam.Aa[st->n_sums - 1];
        r.lambda = cam.lambda;
        r.last_rot = cam.last_rot;
        r.last_trans = cam.last_trans;
        std::memcpy(r.delta, cam.delta, sizeof r.delta);
    }
    return MPE_OK;
}

// accepted = trial = E for every camera
int calib_start(mpe_ctx *ctx, hipStream_t s, mpe_calib_state *st, const double *E) {
    for (int c = 0; c < st->V; ++c) calib_cam_start(&st->host->cam[c], E + 12 * c);
    return normal_start(ctx, s, st);
}

// accepted = trial = (E, k, dist) for every camera
int camfit_start(mpe_ctx *ctx, hipStream_t s, mpe_camfit_state *st, const double *E, const float *k, const double *dist) {
    for (int c = 0; c < st->V; ++c) camfit_cam_start(&st->host->cam[c], E + 12 * c, k + 4 * c, dist + 5 * c);
    return normal_start(ctx, s, st);
}

// (fx, fy, cx, cy) of the context's own cfg.K -> k [V][4].  A K of another form than [[fx,0,cx],[0,fy,cy],[0,0,1]] is
// refused.
int camfit_own_k(mpe_ctx *ctx, const char *who, float *k) {
    for (int c = 0; c < ctx->cfg.n_cameras; ++c) {
        const float *K = ctx->hcfg.K[c];
        if (K[1] != 0.0f || K[3] != 0.0f || K[6] != 0.0f || K[7] != 0.0f || K[8] != 1.0f)
            return fail(ctx, MPE_ERR_INVALID, "%s: K of camera %d is not [[fx,0,cx],[0,fy,cy],[0,0,1]]", who, c);
        k[4 * c] = K[0], k[4 * c + 1] = K[4], k[4 * c + 2] = K[2], k[4 * c + 3] = K[5];
    }
    return MPE_OK;
}

void camfit_copy_out(const camfit_set &from, int c, double *E, float *k, double *dist) {
    if (E) std::memcpy(E + 12 * c, from.E, sizeof from.E);
    if (k) std::memcpy(k + 4 * c, from.k, sizeof from.k);
    if (dist) std::memcpy(dist + 5 * c, from.dist, sizeof from.dist);
}

}  // namespace

extern "C" {

int mpe_calib_destroy(mpe_ctx *ctx, mpe_calib_state *st) { return normal_destroy(ctx, "mpe_calib_destroy", st); }

int mpe_calib_create(mpe_ctx *ctx, mpe_calib_state **out) {
    return create_state(ctx, "mpe_calib_create", out, mpe_calib_destroy, [&](mpe_calib_state *st) {
        int rc = normal_alloc(ctx, "mpe_calib_create", st, new (std::nothrow) mpe_calib_host(), MPE_CALIB_SUMS, CALIB_CAM);
        if (!rc) rc = calib_start(ctx, nullptr, st, &ctx->hcfg.P[0][0]);
        return rc;
    });
}

int mpe_calib_reset(mpe_ctx *ctx, void *stream, mpe_calib_state *st) {
    if (!ctx) return MPE_ERR_INVALID;
    if (!st) return fail(ctx, MPE_ERR_INVALID, "mpe_calib_reset: NULL state");
    DeviceGuard dg(ctx);
    return calib_start(ctx, static_cast<hipStream_t>(stream), st, &ctx->hcfg.P[0][0]);
}

int mpe_calib_set_extrinsics(mpe_ctx *ctx, void *stream, mpe_calib_state *st, const double *E) {
    if (!ctx) return MPE_ERR_INVALID;
    if (!st || !E) return fail(ctx, MPE_ERR_INVALID, "mpe_calib_set_extrinsics: NULL argument");
    for (int i = 0; i < st->V * 12; ++i)
        if (!calib_finite(E[i])) return fail(ctx, MPE_ERR_INVALID, "mpe_calib_set_extrinsics: entry %d of camera %d is not finite", i % 12, i / 12);
    DeviceGuard dg(ctx);
    return calib_start(ctx, static_cast<hipStream_t>(stream), st, E);
}

int mpe_calib_get_extrinsics(mpe_ctx *ctx, const mpe_calib_state *st, double *accepted, double *trial) {
    if (!ctx) return MPE_ERR_INVALID;
    if (!st) return fail(ctx, MPE_ERR_INVALID, "mpe_calib_get_extrinsics: NULL state");
    for (int c = 0; c < st->V; ++c) {
        if (accepted) std::memcpy(accepted + 12 * c, st->host->cam[c].Ea, 12 * sizeof(double));
        if (trial) std::memcpy(trial + 12 * c, st->host->cam[c].Et, 12 * sizeof(double));
    }
    return MPE_OK;
}

int mpe_calib_launches(mpe_ctx *ctx, const mpe_calib_state *st, int64_t *n) { return state_launches(ctx, "mpe_calib_launches", st, n); }

int mpe_calib_batch(mpe_ctx *ctx, void *stream, mpe_calib_state *st, const mpe_batch *b, const mpe_calib_args *a) {
    return normal_batch(ctx, "mpe_calib_batch", stream, st, b, a, launch_calib);
}

int mpe_calib_read(mpe_ctx *ctx, void *stream, mpe_calib_state *st, double *sums, int64_t *n_obs, int64_t *n_skipped) {
    return normal_read(ctx, "mpe_calib_read", stream, st, sums, n_obs, n_skipped);
}

int mpe_calib_step(mpe_ctx *ctx, void *stream, mpe_calib_state *st, const mpe_calib_step_args *a, mpe_calib_report *report) {
    if (!ctx) return MPE_ERR_INVALID;
    if (!st || !a) return fail(ctx, MPE_ERR_INVALID, "mpe_calib_step: NULL argument");
    if (a->min_obs < 6) return fail(ctx, MPE_ERR_INVALID, "mpe_calib_step: min_obs %lld is below 6, the unknowns of a camera", (long long)a->min_obs);
    if (!(a->rot_tol >= 0.0) || !(a->trans_tol >= 0.0))
        return fail(ctx, MPE_ERR_INVALID, "mpe_calib_step: rot_tol %g and trans_tol %g must not be negative", a->rot_tol, a->trans_tol);
    return normal_step(ctx, "mpe_calib_step", stream, st, a->hold_mask, report, [&](calib_cam *cam, const double *sums, long long n_obs, int held) {
        calib_cam_step(cam, sums, n_obs, held, a->min_obs, a->rot_tol, a->trans_tol);
    });
}

int mpe_camfit_destroy(mpe_ctx *ctx, mpe_camfit_state *st) { return normal_destroy(ctx, "mpe_camfit_destroy", st); }

int mpe_camfit_create(mpe_ctx *ctx, mpe_camfit_state **out) {
    return create_state(ctx, "mpe_camfit_create", out, mpe_camfit_destroy, [&](mpe_camfit_state *st) {
        float k[MPE_MAX_CAMERAS * 4];
        int rc = camfit_own_k(ctx, "mpe_camfit_create", k);   // the form of K, before anything is allocated on the device
        if (!rc) rc = normal_alloc(ctx, "mpe_camfit_create", st, new (std::nothrow) mpe_camfit_host(), MPE_CAMFIT_SUMS, CAMFIT_CAM);
        if (!rc) rc = camfit_start(ctx, nullptr, st, &ctx->hcfg.P[0][0], k, &ctx->hcfg.dist[0][0]);
        return rc;
    });
}

int mpe_camfit_reset(mpe_ctx *ctx, void *stream, mpe_camfit_state *st) {
    if (!ctx) return MPE_ERR_INVALID;
    if (!st) return fail(ctx, MPE_ERR_INVALID, "mpe_camfit_reset: NULL state");
    DeviceGuard dg(ctx);
    float k[MPE_MAX_CAMERAS * 4];
    const int rc = camfit_own_k(ctx, "mpe_camfit_reset", k);
    return rc ? rc : camfit_start(ctx, static_cast<hipStream_t>(stream), st, &ctx->hcfg.P[0][0], k, &ctx->hcfg.dist[0][0]);
}

int mpe_camfit_set_cameras(mpe_ctx *ctx, void *stream, mpe_camfit_state *st, const double *E, const float *k, const double *dist) {
    if (!ctx) return MPE_ERR_INVALID;
    if (!st || !E || !k || !dist) return fail(ctx, MPE_ERR_INVALID, "mpe_camfit_set_cameras: NULL argument");
    for (int c = 0; c < st->V; ++c) {
        bool ok = true;
        for (int i = 0; i < 12; ++i) ok &= calib_finite(E[12 * c + i]) != 0;
        for (int i = 0; i < 4; ++i) ok &= calib_finite((double)k[4 * c + i]) != 0;
        for (int i = 0; i < 5; ++i) ok &= calib_finite(dist[5 * c + i]) != 0;
        if (!ok) return fail(ctx, MPE_ERR_INVALID, "mpe_camfit_set_cameras: camera %d has a value that is not finite", c);
        if (!(k[4 * c] > 0.0f) || !(k[4 * c + 1] > 0.0f))
            return fail(ctx, MPE_ERR_INVALID, "mpe_camfit_set_cameras: fx %g and fy %g of camera %d must be positive", (double)k[4 * c],
                        (double)k[4 * c + 1], c);
    }
    DeviceGuard dg(ctx);
    return camfit_start(ctx, static_cast<hipStream_t>(stream), st, E, k, dist);
}

int mpe_camfit_get_cameras(mpe_ctx *ctx, const mpe_camfit_state *st, double *E_accepted, float *k_accepted, double *dist_accepted,
                           double *E_trial, float *k_trial, double *dist_trial) {
    if (!ctx) return MPE_ERR_INVALID;
    if (!st) return fail(ctx, MPE_ERR_INVALID, "mpe_camfit_get_cameras: NULL state");
    for (int c = 0; c < st->V; ++c) {
        camfit_copy_out(st->host->cam[c].a, c, E_accepted, k_accepted, dist_accepted);
        camfit_copy_out(st->host->cam[c].t, c, E_trial, k_trial, dist_trial);
    }
    return MPE_OK;
}

int mpe_camfit_launches(mpe_ctx *ctx, const mpe_camfit_state *st, int64_t *n) { return state_launches(ctx, "mpe_camfit_launches", st, n); }

int mpe_camfit_batch(mpe_ctx *ctx, void *stream, mpe_camfit_state *st, const mpe_batch *b, const mpe_calib_args *a) {
    return normal_batch(ctx, "mpe_camfit_batch", stream, st, b, a, launch_camfit);
}

int mpe_camfit_read(mpe_ctx *ctx, void *stream, mpe_camfit_state *st, double *sums, int64_t *n_obs, int64_t *n_skipped) {
    return normal_read(ctx, "mpe_camfit_read", stream, st, sums, n_obs, n_skipped);
}

int mpe_camfit_step(mpe_ctx *ctx, void *stream, mpe_camfit_state *st, const mpe_camfit_step_args *a, mpe_camfit_report *report) {
    if (!ctx) return MPE_ERR_INVALID;
    if (!st || !a) return fail(ctx, MPE_ERR_INVALID, "mpe_camfit_step: NULL argument");
    if (a->free_mask == 0 || (a->free_mask & ~(uint32_t)CAMFIT_ALL))
        return fail(ctx, MPE_ERR_INVALID, "mpe_camfit_step: free_mask 0x%x must name at least one of the six groups and nothing else", a->free_mask);
    int idx[CAMFIT_N];
    const int n_free = camfit_free(a->free_mask, idx);
    if (a->min_obs < 6 || a->min_obs < n_free)
        return fail(ctx, MPE_ERR_INVALID, "mpe_camfit_step: min_obs %lld is below %d, the larger of 6 and the free unknowns of a camera",
                    (long long)a->min_obs, n_free > 6 ? n_free : 6);
    if (!(a->rot_tol >= 0.0) || !(a->trans_tol >= 0.0) || !(a->pix_tol >= 0.0) || !(a->lens_tol >= 0.0))
        return fail(ctx, MPE_ERR_INVALID, "mpe_camfit_step: rot_tol %g, trans_tol %g, pix_tol %g and lens_tol %g must not be negative", a->rot_tol,
                    a->trans_tol, a->pix_tol, a->lens_tol);
    const camfit_rule rule{a->rot_tol, a->trans_tol, a->pix_tol, a->lens_tol, (long long)a->min_obs, a->free_mask};
    const int rc = normal_step(ctx, "mpe_camfit_step", stream, st, a->hold_mask, report,
                               [&](camfit_cam *cam, const double *sums, long long n_obs, int held) { camfit_cam_step(cam, sums, n_obs, held, &rule); });
    if (rc || !report) return rc;
    for (int c = 0; c < st->V; ++c) {
        report->cam[c].last_pix = st->host->cam[c].last_pix;
        report->cam[c].last_lens = st->host->cam[c].last_lens;
    }
    return MPE_OK;
}

}  // extern "C"

// ---- time lags (lag.hip sums on the device; the pick below is host work, once per pass) ----
#include "lag_pick.h"

namespace {

struct LagSums {
    std::vector<double> cost;
    std::vector<int64_t> ctr;                        // n_obs [V][K] | n_skipped [V][K] | n_support [V] | n_unsupported [V]
};

int lag_fetch(mpe_ctx *ctx, hipStream_t s, mpe_lag_state *st, LagSums *h) {
    const size_t vk = (size_t)st->V * st->K;
    h->cost.resize(vk);
    h->ctr.resize(lag_counter_words(st->V, st->K));
    HIPCHK(ctx, hipMemcpyAsync(h->cost.data(), st->cost, vk * sizeof(double), hipMemcpyDeviceToHost, s));
    HIPCHK(ctx, hipMemcpyAsync(h->ctr.data(), st->ctr, h->ctr.size() * sizeof(int64_t), hipMemcpyDeviceToHost, s));
    HIPCHK(ctx, hipStreamSynchronize(s));
    return MPE_OK;
}

}  // namespace

extern "C" {

int mpe_lag_destroy(mpe_ctx *ctx, mpe_lag_state *st) {
    if (!ctx) return MPE_ERR_INVALID;
    if (!st) return fail(ctx, MPE_ERR_INVALID, "mpe_lag_destroy: NULL state");
    DeviceGuard dg(ctx);
    dev_free(ctx, st->cost);
    dev_free(ctx, st->ctr);
    dev_free(ctx, st->S);
    delete st;
    return MPE_OK;
}

int mpe_lag_create(mpe_ctx *ctx, const mpe_lag_config *cfg, mpe_lag_state **out) {
    return create_state(ctx, "mpe_lag_create", out, mpe_lag_destroy, [&](mpe_lag_state *st) {
        if (!cfg) return fail(ctx, MPE_ERR_INVALID, "mpe_lag_create: NULL argument");
        if (cfg->window < 0 || cfg->window > MPE_LAG_MAX_WINDOW || cfg->sub < 1 || cfg->sub > MPE_LAG_MAX_SUB)
            return fail(ctx, MPE_ERR_INVALID, "mpe_lag_create: window %d must be within 0 .. %d and sub %d within 1 .. %d", cfg->window,
                        MPE_LAG_MAX_WINDOW, cfg->sub, MPE_LAG_MAX_SUB);
        if (cfg->n_joints != ctx->cfg.n_joints)
            return fail(ctx, MPE_ERR_INVALID, "mpe_lag_create: %d joints, the context has %d", cfg->n_joints, ctx->cfg.n_joints);
        if (cfg->pcap < 1 || cfg->max_frames < 1 || (cfg->pose_f64 & ~1) || (cfg->joint_flags & ~1))
            return fail(ctx, MPE_ERR_INVALID, "mpe_lag_create: pcap %d and max_frames %d must be at least 1, pose_f64 %d and joint_flags %d 0 or 1",
                        cfg->pcap, cfg->max_frames, cfg->pose_f64, cfg->joint_flags);
        if (cfg->pcap > MPE_TRACK_MAX_PERSONS || cfg->max_frames > (1 << 23))
            return fail(ctx, MPE_ERR_CAPACITY, "mpe_lag_create: pcap %d over %d or max_frames %d over 2^23", cfg->pcap, MPE_TRACK_MAX_PERSONS,
                        cfg->max_frames);
        st->V = ctx->cfg.n_cameras;
        st->W = cfg->window;
        st->sub = cfg->sub;
        st->K = 2 * cfg->window * cfg->sub + 1;
        st->pcap = cfg->pcap;
        st->J = cfg->n_joints;
        st->pose_f64 = cfg->pose_f64;
        st->joint_flags = cfg->joint_flags;
        st->max_frames = cfg->max_frames;
        const size_t vk = (size_t)st->V * st->K;
        int rc = dev_alloc(ctx, &st->cost, vk);
        if (!rc) rc = dev_alloc(ctx, &st->ctr, lag_counter_words(st->V, st->K));
        if (!rc) rc = dev_alloc(ctx, &st->S, (size_t)st->max_frames * vk, false);
        return rc;
    });
}

int mpe_lag_reset(mpe_ctx *ctx, void *stream, mpe_lag_state *st) { return reset_state(ctx, "mpe_lag_reset", stream, st, launch_lag_reset); }

int mpe_lag_launches(mpe_ctx *ctx, const mpe_lag_state *st, int64_t *n) { return state_launches(ctx, "mpe_lag_launches", st, n); }

int mpe_lag_batch(mpe_ctx *ctx, void *stream, mpe_lag_state *st, const mpe_batch *b, const mpe_lag_args *a) {
    int rc = check_batch(ctx, b);
    if (rc) return rc;
    if (!st || !a) return fail(ctx, MPE_ERR_INVALID, "mpe_lag_batch: NULL argument");
    DeviceGuard dg(ctx);
    if (a->n_frames != b->n_frames)
        return fail(ctx, MPE_ERR_INVALID, "mpe_lag_batch: n_frames %d, the batch has %d frames", a->n_frames, b->n_frames);
    if (a->n_joints != ctx->cfg.n_joints)
        return fail(ctx, MPE_ERR_INVALID, "mpe_lag_batch: %d joints, the context has %d", a->n_joints, ctx->cfg.n_joints);
    bool run;
    rc = check_pose_rows(ctx, "mpe_lag_batch", st, a, &run);
    if (rc) return rc;
    if (a->joint_flags != st->joint_flags)
        return fail(ctx, MPE_ERR_INVALID, "mpe_lag_batch: joint_flags %d, the state was made for %d", a->joint_flags, st->joint_flags);
    if (st->V != ctx->cfg.n_cameras) return fail(ctx, MPE_ERR_INVALID, "mpe_lag_batch: the state belongs to another context");
    if (a->frame_start < 0 || a->n_table < 0 || (int64_t)a->frame_start + a->n_frames > a->n_table)
        return fail(ctx, MPE_ERR_INVALID, "mpe_lag_batch: frame_start %d + n_frames %d must lie within the table's %d frames", a->frame_start,
                    a->n_frames, a->n_table);
    if (a->n_frames > st->max_frames)
        return fail(ctx, MPE_ERR_INVALID, "mpe_lag_batch: %d frames, max_frames of the state is %d", a->n_frames, st->max_frames);
    if (!(a->huber_px >= 0.0)) return fail(ctx, MPE_ERR_INVALID, "mpe_lag_batch: huber_px %g must not be negative", a->huber_px);
    if (!run) return MPE_OK;
    if (!a->d_persons || !a->d_poses || !a->d_flags || !a->d_n_persons || !a->d_tid) return fail(ctx, MPE_ERR_INVALID, "mpe_lag_batch: NULL argument");
    HIPCHK(ctx, launch_lag(static_cast<hipStream_t>(stream), ctx->d_cfg, st, *b, *a));
    return MPE_OK;
}

int mpe_lag_read(mpe_ctx *ctx, void *stream, mpe_lag_state *st, double *cost, int64_t *n_obs, int64_t *n_skipped, int64_t *n_support,
                 int64_t *n_unsupported) {
    if (!ctx) return MPE_ERR_INVALID;
    if (!st) return fail(ctx, MPE_ERR_INVALID, "mpe_lag_read: NULL state");
    DeviceGuard dg(ctx);
    LagSums h;
    const int rc = lag_fetch(ctx, static_cast<hipStream_t>(stream), st, &h);
    if (rc) return rc;
    const size_t vk = (size_t)st->V * st->K, v = (size_t)st->V;
    if (cost) std::memcpy(cost, h.cost.data(), vk * sizeof(double));
    if (n_obs) std::memcpy(n_obs, h.ctr.data(), vk * sizeof(int64_t));
    if (n_skipped) std::memcpy(n_skipped, h.ctr.data() + vk, vk * sizeof(int64_t));
    if (n_support) std::memcpy(n_support, h.ctr.data() + 2 * vk, v * sizeof(int64_t));
    if (n_unsupported) std::memcpy(n_unsupported, h.ctr.data() + 2 * vk + v, v * sizeof(int64_t));
    return MPE_OK;
}

int mpe_lag_estimate(mpe_ctx *ctx, void *stream, mpe_lag_state *st, int32_t min_obs, mpe_lag_report *report) {
    if (!ctx) return MPE_ERR_INVALID;
    if (!st || !report) return fail(ctx, MPE_ERR_INVALID, "mpe_lag_estimate: NULL argument");
    if (min_obs < 1) return fail(ctx, MPE_ERR_INVALID, "mpe_lag_estimate: min_obs %lld is below 1", (long long)min_obs);
    DeviceGuard dg(ctx);
    LagSums h;
    const int rc = lag_fetch(ctx, static_cast<hipStream_t>(stream), st, &h);
    if (rc) return rc;
    const size_t vk = (size_t)st->V * st->K;
    std::memset(report, 0, sizeof *report);
    report->n_cameras = st->V;
    report->n_grid = st->K;
    for (int c = 0; c < st->V; ++c) {
        const lag_pick_result p = lag_pick(h.cost.data() + (size_t)c * st->K, h.ctr.data() + (size_t)c * st->K, st->W, st->sub, min_obs);
        mpe_lag_cam_report &r = report->cam[c];
        r.status = p.status;
        r.k_best = p.k_best;
        r.lag_grid = p.lag_grid;
        r.lag_refined = p.lag_refined;
        r.cost_best = p.cost_best;
        r.cost_zero = p.cost_zero;
        r.n_obs = p.n_obs;
        r.n_support = h.ctr[2 * vk + c];
        r.n_unsupported = h.ctr[2 * vk + st->V + c];
    }
    return MPE_OK;
}

// ---- time-aware refinement (refine_timed.hip): mpe_refine_batch's checks, mpe_lag_batch's on the table, and the lags ----
int mpe_refine_timed_batch(mpe_ctx *ctx, void *stream, const mpe_batch *b, const mpe_refine_timed_args *a) {
    int rc = check_batch(ctx, b);
    if (rc) return rc;
    if (!a) return fail(ctx, MPE_ERR_INVALID, "mpe_refine_timed_batch: NULL argument");
    DeviceGuard dg(ctx);
    bool run;
    rc = check_batch_rows(ctx, "mpe_refine_timed_batch", b, a, &run);
    if (rc) return rc;
    if (a->n_frames > (1 << 23)) return fail(ctx, MPE_ERR_CAPACITY, "mpe_refine_timed_batch: %d frames over 2^23 per call", a->n_frames);
    if (a->max_iters < 1 || a->max_iters > MPE_REFINE_MAX_ITERS)
        return fail(ctx, MPE_ERR_INVALID, "mpe_refine_timed_batch: max_iters %d outside 1..%d", a->max_iters, MPE_REFINE_MAX_ITERS);
    if (!(a->step_tol >= 0.0) || !(a->huber_px >= 0.0))
        return fail(ctx, MPE_ERR_INVALID, "mpe_refine_timed_batch: step_tol %g and huber_px %g must not be negative", a->step_tol, a->huber_px);
    if (a->frame_start < 0 || a->n_table < 0 || (int64_t)a->frame_start + a->n_frames > a->n_table)
        return fail(ctx, MPE_ERR_INVALID, "mpe_refine_timed_batch: frame_start %d + n_frames %d must lie within the table's %d frames",
                    a->frame_start, a->n_frames, a->n_table);
    for (int c = 0; c < ctx->cfg.n_cameras; ++c)
        if (!(fabs(a->lag[c]) <= (double)MPE_LAG_MAX_WINDOW))          // a NaN fails the comparison, an infinity exceeds it
            return fail(ctx, MPE_ERR_INVALID, "mpe_refine_timed_batch: lag %g of camera %d must be finite and within %d frames", a->lag[c], c,
                        MPE_LAG_MAX_WINDOW);
    if (!run) return MPE_OK;
    if (!a->d_persons || !a->d_poses || !a->d_flags || !a->d_n_persons || !a->d_tid || !a->d_poses_out || !a->d_status || !a->d_cost0 ||
        !a->d_cost1 || !a->d_iters || !a->d_n_views || !a->d_n_timed)
        return fail(ctx, MPE_ERR_INVALID, "mpe_refine_timed_batch: NULL argument");
    const size_t joint_bytes = (size_t)a->pcap * a->n_joints * 3 * (a->pose_f64 ? sizeof(double) : sizeof(float));
    const uintptr_t tab0 = reinterpret_cast<uintptr_t>(a->d_poses), tab1 = tab0 + (size_t)a->n_table * joint_bytes;
    const uintptr_t out0 = reinterpret_cast<uintptr_t>(a->d_poses_out), out1 = out0 + (size_t)a->n_frames * joint_bytes;
    if (out0 < tab1 && tab0 < out1)
        return fail(ctx, MPE_ERR_INVALID, "mpe_refine_timed_batch: d_poses_out overlaps the table (other frames read their neighbours from it)");
    if ((int64_t)a->n_frames * a->pcap > 0x7FFFFFFFLL)             // one workgroup per 1 .. 8 rows, no stride loop
        return fail(ctx, MPE_ERR_CAPACITY, "mpe_refine_timed_batch: %d frames of %d rows are more workgroups than a launch takes", a->n_frames, a->pcap);
    HIPCHK(ctx, launch_refine_timed(static_cast<hipStream_t>(stream), ctx->d_cfg, ctx->cfg.n_cameras, *b, *a));
    return MPE_OK;
}

// ---- the pose document (jsonwrite.hip) ----
size_t mpe_json_write_bound(int32_t n_frames, int32_t pcap, int32_t n_joints, int32_t with_ids) {
    if (n_frames < 0 || pcap < 0 || n_joints < 0) return 0;
    // `"jj": [x, y, z], ` with three 24-byte tokens; `{}, ` around a row; an id of 11 bytes with `, `; a frame number of 20
    const size_t joint = 4 + 8 + 3 * MPE_FMT_MAX_LEN + 2, row = 2 + 2 + (size_t)n_joints * joint;
    const size_t line = 10 + 20 + (with_ids ? 10 + (size_t)pcap * 13 + 1 : 0) + 13 + (size_t)pcap * row + 3;
    return (size_t)n_frames * line;
}

size_t mpe_json_write_scratch_bytes(int32_t n_frames, int32_t pcap, int32_t n_joints) {
    if (n_frames < 0 || pcap < 0 || n_joints < 0) return 0;
    return json_write_scratch_bytes(n_frames, pcap, n_joints);
}

int mpe_json_write_launches(mpe_ctx *ctx, int64_t *n) {
    if (!ctx) return MPE_ERR_INVALID;
    if (!n) return fail(ctx, MPE_ERR_INVALID, "mpe_json_write_launches: NULL argument");
    *n = ctx->json_write_launches;
    return MPE_OK;
}

int mpe_json_write_poses(mpe_ctx *ctx, void *stream, const mpe_json_write_args *a) {
    if (!ctx) return MPE_ERR_INVALID;
    if (!a) return fail(ctx, MPE_ERR_INVALID, "mpe_json_write_poses: NULL argument");
    DeviceGuard dg(ctx);
    if (a->n_joints != ctx->cfg.n_joints || a->pcap < 1 || (a->pose_f64 & ~1) || (a->joint_flags & ~1))
        return fail(ctx, MPE_ERR_INVALID, "mpe_json_write_poses: joints %d (the context has %d) / pcap %d / pose_f64 %d / joint_flags %d", a->n_joints,
                    ctx->cfg.n_joints, a->pcap, a->pose_f64, a->joint_flags);
    if (a->n_frames < 0 || a->frame_start < 0 || a->frame_start > ((int64_t)1 << 62))
        return fail(ctx, MPE_ERR_INVALID, "mpe_json_write_poses: n_frames %d / frame_start %lld", a->n_frames, (long long)a->frame_start);
    if (!(fabs(a->scale) < HUGE_VAL)) return fail(ctx, MPE_ERR_INVALID, "mpe_json_write_poses: scale %g is not finite", a->scale);
    if (a->text_cap >= ((uint64_t)1 << 32))
        return fail(ctx, MPE_ERR_INVALID, "mpe_json_write_poses: text_cap %llu; the extents are 32-bit offsets", (unsigned long long)a->text_cap);
    if (a->pcap > MPE_JSON_WRITE_MAX_PERSONS) return fail(ctx, MPE_ERR_CAPACITY, "mpe_json_write_poses: pcap %d over %d", a->pcap, MPE_JSON_WRITE_MAX_PERSONS);
    if (a->n_frames > (1 << 23)) return fail(ctx, MPE_ERR_CAPACITY, "mpe_json_write_poses: %d frames over 2^23 per call", a->n_frames);
    if ((int64_t)a->n_frames * a->pcap * a->n_joints * 3 >= ((int64_t)1 << 31))
        return fail(ctx, MPE_ERR_CAPACITY, "mpe_json_write_poses: %d frames of %d rows are 2^31 coordinates or more", a->n_frames, a->pcap);
    if (!a->d_frame_off || !a->d_total || (a->text_cap && !a->d_text)) return fail(ctx, MPE_ERR_INVALID, "mpe_json_write_poses: NULL argument");
    if (a->n_frames > 0) {
        if (!a->d_poses || !a->d_flags || !a->d_n_persons || !a->d_text || !a->d_bodies_extent || !a->d_rows_written || !a->d_status || !a->d_scratch)
            return fail(ctx, MPE_ERR_INVALID, "mpe_json_write_poses: NULL argument");
        const size_t need = json_write_scratch_bytes(a->n_frames, a->pcap, a->n_joints);
        if (a->scratch_bytes < need || (reinterpret_cast<uintptr_t>(a->d_scratch) & 15u))
            return fail(ctx, MPE_ERR_INVALID, "mpe_json_write_poses: scratch of %zu bytes, %zu needed, 16-byte aligned", a->scratch_bytes, need);
    }
    HIPCHK(ctx, launch_json_write(static_cast<hipStream_t>(stream), *a, &ctx->json_write_launches));
    return MPE_OK;
}

int mpe_format_f64(mpe_ctx *ctx, void *stream, const double *d_values, int64_t n, char *d_slots, uint8_t *d_len) {
    if (!ctx) return MPE_ERR_INVALID;
    if (n < 0 || n >= ((int64_t)1 << 31)) return fail(ctx, MPE_ERR_INVALID, "mpe_format_f64: n %lld outside 0 .. 2^31 - 1", (long long)n);
    if (n == 0) return MPE_OK;
    if (!d_values || !d_slots || !d_len) return fail(ctx, MPE_ERR_INVALID, "mpe_format_f64: NULL argument");
    DeviceGuard dg(ctx);
    HIPCHK(ctx, launch_format_f64(static_cast<hipStream_t>(stream), d_values, n, d_slots, d_len));
    return MPE_OK;
}

}  // extern "C"
