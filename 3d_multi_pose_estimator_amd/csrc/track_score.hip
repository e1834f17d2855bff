// Track scoring: CLEAR-MOT and identity counts of tracked poses against ground-truth identities (include/mpe.h:
// mpe_track_score_batch; the numpy statement is harness/track_score.py).  Three kernels per call whatever the frame count:
//
// k_ts_frame   one wavefront per frame.  It numbers the detections (ballot + prefix count over the person flags), sorts
//              them into ignored / match / false positive, writes the frame's counts and d_match_tid, leaves the frame's
//              records in the dense scratch rec[f][o] (h, -1 miss, -2 none) and adds to table and pred_count.
// k_ts_ident   one lane per identity walks rec over the frames of the call; neighbouring lanes read neighbouring
//              words.  last / present / matched / bits live in registers in between and go back to the state; an ID switch
//              is added to its frame's counter, the fragmentations to the total.
// k_ts_totals  one workgroup.  A scan over the frames' tp packs the errors of the matches in (frame, detection) order,
//              the integer totals are summed, and one lane continues the left fold of err_sum over the packed errors.
//
// Integer atomics only: every output is the same whatever the order the hardware takes.  The one-to-one pairing behind
// IDTP is not here: it runs once per recording on the host (assign_int.h, called by mpe_track_score_result).
#include "mpe_internal.h"
#include "pose_rows.h"

#pragma clang fp contract(off)

namespace mpe {

namespace {

constexpr int TS_CAP = MPE_TRACK_MAX_PERSONS;          // rows of either side, two per lane
constexpr int TS_WAVE = 64;
enum { T_FRAMES, T_NGT, T_NPRED, T_TP, T_FP, T_FN, T_IDSW, T_FRAG, T_IGN, T_OVER, T_ERR, T_STATUS };
static_assert(T_STATUS + 1 == MPE_TS_TOTALS, "totals layout");
static_assert(TS_CAP == 2 * TS_WAVE, "two rows per lane");

struct TsK : PoseRows {               // no coordinates here: PoseRows::poses stays null, J and pose_f64 0
    int gcap, gid_cap, tid_cap;
    double thr;
    const int32_t *assign;
    const double *err;
    const uint8_t *invalid;
    const int32_t *n_res, *n_gt, *gt_id;
    const uint8_t *gt_valid, *skip;
    int32_t *frame_counts, *match_tid, *status;
    int64_t *totals;
    int32_t *ident, *pred_count, *table, *rec, *fstat;
    uint64_t *mmask;
    double *merr;
};

__device__ inline int wave_count(bool b) { return __popcll(__ballot(b)); }

__global__ void __launch_bounds__(TS_WAVE) k_ts_frame(TsK a) {
    __shared__ int16_t s_row[TS_CAP];                    // detection r -> person row p
    __shared__ int32_t s_go[TS_CAP], s_first[TS_CAP], s_mtid[TS_CAP];
    __shared__ uint8_t s_cls[TS_CAP];                    // GT row: 0 none, 1 ignore, 2 counted
    const int f = blockIdx.x, lane = threadIdx.x, pcap = a.pcap, gcap = a.gcap;
    const size_t fp0 = (size_t)f * pcap, fg0 = (size_t)f * gcap;
    int32_t *rec = a.rec + (size_t)f * a.gid_cap;
    for (int o = lane; o < a.gid_cap; o += TS_WAVE) rec[o] = -2;
    if (a.skip && a.skip[f]) {
        for (int g = lane; g < gcap; g += TS_WAVE) a.match_tid[fg0 + g] = -2;
        if (lane < 4) a.frame_counts[(size_t)f * 4 + lane] = 0;
        if (lane < 8) a.fstat[(size_t)f * 8 + lane] = 0;
        if (lane < 2) a.mmask[(size_t)f * 2 + lane] = 0;
        return;
    }
    const int n_p = rows_in_frame(a, f), n_g = min(max(a.n_gt[f], 0), gcap);
    int n_det = n_p;
    if (!a.joint_flags) {
        n_det = 0;
        for (int base = 0; base < TS_CAP; base += TS_WAVE) {
            const int p = base + lane;
            const bool on = p < n_p && a.flags[fp0 + p] != 0;
            const uint64_t m = __ballot(on);
            if (on) s_row[n_det + __popcll(m & ((1ull << lane) - 1ull))] = (int16_t)p;
            n_det += __popcll(m);
        }
    } else {
        for (int p = lane; p < n_p; p += TS_WAVE) s_row[p] = (int16_t)p;
    }
    n_det = min(n_det, min(max(a.n_res[f], 0), pcap));
    for (int g = lane; g < gcap; g += TS_WAVE) {
        const int32_t o = g < n_g ? a.gt_id[fg0 + g] : -1;
        const int cls = g < n_g ? ((a.gt_valid[fg0 + g] != 0 && o >= 0) ? 2 : 1) : 0;
        s_go[g] = o;
        s_cls[g] = (uint8_t)cls;
        s_first[g] = INT_MAX;
        s_mtid[g] = cls == 2 ? -1 : -2;
    }
    __syncthreads();

    int32_t g_[2], h_[2];
    bool ign_[2], cand_[2], det_[2];
    for (int k = 0; k < 2; ++k) {
        const int r = k * TS_WAVE + lane;
        det_[k] = r < n_det;
        g_[k] = -1; h_[k] = -1; ign_[k] = false; cand_[k] = false;
        if (det_[k]) {
            const int32_t g = a.assign[fp0 + r];
            const double e = a.err[fp0 + r];
            const bool inv = a.invalid && a.invalid[fp0 + r] != 0;
            const int cls = (g >= 0 && g < n_g) ? s_cls[g] : 0;
            g_[k] = g;
            h_[k] = a.tid[fp0 + s_row[r]];
            ign_[k] = cls == 1;
            cand_[k] = cls == 2 && e * 1000. < a.thr && !inv && h_[k] >= 0;
            if (cand_[k]) atomicMin(&s_first[g], r);
        }
    }
    __syncthreads();
    int tp = 0, fp = 0, ign = 0, over = 0;
    for (int k = 0; k < 2; ++k) {
        const int r = k * TS_WAVE + lane;
        const bool match = cand_[k] && s_first[g_[k]] == r;
        const bool counts = det_[k] && !ign_[k];
        const uint64_t mm = __ballot(match);
        if (lane == 0) a.mmask[(size_t)f * 2 + k] = mm;
        tp += __popcll(mm);
        fp += wave_count(counts && !match);
        ign += wave_count(ign_[k]);
        if (match) s_mtid[g_[k]] = h_[k];
        const bool named = counts && h_[k] >= 0;
        if (named && h_[k] < a.tid_cap) atomicAdd(&a.pred_count[h_[k]], 1);
        over += wave_count(named && h_[k] >= a.tid_cap);
    }
    __syncthreads();
    int counted = 0;
    for (int base = 0; base < TS_CAP; base += TS_WAVE) {
        const int g = base + lane;
        const bool row = g < gcap && s_cls[g] == 2;
        bool left_out = false;
        if (g < gcap) a.match_tid[fg0 + g] = s_mtid[g];
        if (row) {
            const int32_t o = s_go[g], h = s_mtid[g];
            left_out = o >= a.gid_cap || h >= a.tid_cap;
            for (int q = 0; q < g && !left_out; ++q) left_out = s_cls[q] == 2 && s_go[q] == o;
            if (!left_out) {
                rec[o] = h;
                if (h >= 0) atomicAdd(&a.table[(size_t)o * a.tid_cap + h], 1);
            }
        }
        counted += wave_count(row);
        over += wave_count(left_out);
    }
    if (lane == 0) {
        int32_t *c = a.frame_counts + (size_t)f * 4, *s = a.fstat + (size_t)f * 8;
        c[0] = tp; c[1] = fp; c[2] = counted - tp; c[3] = 0;
        s[0] = tp; s[1] = fp; s[2] = counted - tp; s[3] = ign; s[4] = counted; s[5] = tp + fp; s[6] = over; s[7] = 1;
    }
}

__global__ void __launch_bounds__(256) k_ts_ident(TsK a) {
    const int o = blockIdx.x * blockDim.x + threadIdx.x, G = a.gid_cap;
    if (o >= G) return;
    int32_t last = a.ident[o], present = a.ident[G + o], matched = a.ident[2 * G + o], bits = a.ident[3 * G + o];
    unsigned long long frag = 0;
    for (int f0 = 0; f0 < a.n_frames; f0 += 8) {
        int32_t v[8];
        for (int k = 0; k < 8; ++k) v[k] = f0 + k < a.n_frames ? a.rec[(size_t)(f0 + k) * G + o] : -2;
        for (int k = 0; k < 8; ++k) {
            if (v[k] == -2) continue;
            ++present;
            if (v[k] >= 0) {
                ++matched;
                if (last >= 0 && last != v[k]) atomicAdd(&a.frame_counts[(size_t)(f0 + k) * 4 + 3], 1);
                last = v[k];
                if (bits == 3) ++frag;
                bits = 1;
            } else {
                bits |= 2;
            }
        }
    }
    a.ident[o] = last; a.ident[G + o] = present; a.ident[2 * G + o] = matched; a.ident[3 * G + o] = bits;
    if (frag) atomicAdd(reinterpret_cast<unsigned long long *>(a.totals + T_FRAG), frag);
}

__global__ void __launch_bounds__(256) k_ts_totals(TsK a) {
    __shared__ int s_scan[256];
    __shared__ unsigned long long s_tot[T_OVER + 1];
    const int t = threadIdx.x;
    if (t <= T_OVER) s_tot[t] = 0;
    unsigned long long sum[T_OVER + 1] = {};
    size_t running = 0;
    for (int base = 0; base < a.n_frames; base += 256) {
        const int f = base + t;
        const bool in = f < a.n_frames;
        const int32_t *s = a.fstat + (size_t)f * 8;
        const int c = in ? s[0] : 0;
        s_scan[t] = c;
        __syncthreads();
        for (int d = 1; d < 256; d <<= 1) {
            const int add = t >= d ? s_scan[t - d] : 0;
            __syncthreads();
            s_scan[t] += add;
            __syncthreads();
        }
        if (in) {
            sum[T_TP] += s[0]; sum[T_FP] += s[1]; sum[T_FN] += s[2]; sum[T_IGN] += s[3]; sum[T_NGT] += s[4];
            sum[T_NPRED] += s[5]; sum[T_OVER] += s[6]; sum[T_FRAMES] += s[7];
            sum[T_IDSW] += a.frame_counts[(size_t)f * 4 + 3];
            size_t off = running + s_scan[t] - c;
            for (int k = 0; k < 2; ++k) {
                uint64_t m = a.mmask[(size_t)f * 2 + k];
                while (m) {
                    const int r = k * TS_WAVE + __ffsll((unsigned long long)m) - 1;
                    m &= m - 1;
                    a.merr[off++] = a.err[(size_t)f * a.pcap + r];
                }
            }
        }
        running += s_scan[255];
        __syncthreads();
    }
    for (int i = 0; i <= T_OVER; ++i)
        if (i != T_FRAG && sum[i]) atomicAdd(&s_tot[i], sum[i]);
    __syncthreads();
    if (t != 0) return;
    for (int i = 0; i <= T_OVER; ++i)
        if (i != T_FRAG) a.totals[i] += (int64_t)s_tot[i];
    double e = __longlong_as_double(a.totals[T_ERR]);
    for (size_t i0 = 0; i0 < running; i0 += 8) {
        double v[8];
        for (int k = 0; k < 8; ++k) v[k] = i0 + k < running ? a.merr[i0 + k] : 0.0;
        for (int k = 0; k < 8; ++k)
            if (i0 + k < running) e = e + v[k];
    }
    a.totals[T_ERR] = __double_as_longlong(e);
    if (s_tot[T_OVER]) a.totals[T_STATUS] |= MPE_TRACK_SCORE_OVER_IDS;
    *a.status = (int32_t)a.totals[T_STATUS];
}

}  // namespace

// everything a recording accumulates, back to the start; stream-ordered memsets, no kernel
hipError_t launch_track_score_reset(hipStream_t s, mpe_track_score_state *st) {
    const size_t G = (size_t)st->gid_cap, T = (size_t)st->tid_cap;
    hipError_t e = hipMemsetAsync(st->totals, 0, MPE_TS_TOTALS * sizeof(int64_t), s);
    if (e == hipSuccess) e = hipMemsetAsync(st->ident, 0xFF, G * sizeof(int32_t), s);                 // last = -1
    if (e == hipSuccess) e = hipMemsetAsync(st->ident + G, 0, 3 * G * sizeof(int32_t), s);
    if (e == hipSuccess) e = hipMemsetAsync(st->pred_count, 0, T * sizeof(int32_t), s);
    if (e == hipSuccess) e = hipMemsetAsync(st->table, 0, G * T * sizeof(int32_t), s);
    return e;
}

hipError_t launch_track_score(hipStream_t s, mpe_track_score_state *st, const mpe_track_score_args &x) {
    TsK a{};
    a.n_frames = x.n_frames; a.pcap = st->pcap; a.gcap = st->gcap; a.gid_cap = st->gid_cap; a.tid_cap = st->tid_cap;
    a.joint_flags = x.joint_flags; a.thr = x.threshold_mm;
    a.flags = x.d_flags; a.n_persons = x.d_n_persons; a.tid = x.d_track_id; a.assign = x.d_assign; a.err = x.d_err;
    a.invalid = x.d_invalid; a.n_res = x.d_n_res; a.n_gt = x.d_n_gt; a.gt_id = x.d_gt_id; a.gt_valid = x.d_gt_valid; a.skip = x.d_skip;
    a.frame_counts = x.d_frame_counts; a.match_tid = x.d_match_tid; a.status = x.d_status;
    a.totals = st->totals; a.ident = st->ident; a.pred_count = st->pred_count; a.table = st->table;
    a.rec = st->rec; a.fstat = st->fstat; a.mmask = st->mmask; a.merr = st->merr;
    hipError_t e;
#define TS_LAUNCH(...)                                   \
    hipLaunchKernelGGL(__VA_ARGS__);                     \
    if ((e = hipGetLastError()) != hipSuccess) return e; \
    ++st->launches
    TS_LAUNCH(k_ts_frame, dim3(x.n_frames), dim3(TS_WAVE), 0, s, a);
    TS_LAUNCH(k_ts_ident, dim3((st->gid_cap + 255) / 256), dim3(256), 0, s, a);
    TS_LAUNCH(k_ts_totals, dim3(1), dim3(256), 0, s, a);
#undef TS_LAUNCH
    return hipSuccess;
}

}  // namespace mpe
