// Clustering quality of the skeleton-matching stage (test/sm_metrics.py:125-229, test/sm_metrics_without_gt.py:131-170),
// batched: one label per head from the proposals, the greedy ground-truth grouping of a frame's bodies_3D, and the four
// scores of two labelings (adjusted Rand index, homogeneity, completeness, V-measure).  harness/partition.py states the
// same arithmetic on the host and the two agree bit for bit.
//
// k_part_labels: one thread per (frame, head): the first proposal whose row holds the head, else n_persons.
//
// k_part_group: one wave per frame.  The algorithm is sequential in the skeletons, so they go one by one; the persons
// founded so far go across the lanes (person lane, lane + 64, ...), each lane summing its person's distance over that
// person's keys in the order of the founding body's dict.  The reference's scan (strict `<` from 1e9, first wins) is the
// minimum of (distance, person id) in lexicographic order: a running minimum per lane, then a butterfly over the wave.
// The distance of one key is numpy's float64 dot of three elements and a square root, as in eval.hip: dx*dx, then two
// fused multiply-adds.
//
// k_part_scores: one workgroup per frame, thread i = sample i, labels in LDS.  A pass over all pairs gives every sample
// the size of its true class a_i, of its predicted class b_i and of its cell c_i, and tells whether it is the first of
// each; sum a_i = sum of the squared row sums (likewise b, c), so the four pair counts are exact integers.  A second
// pass ranks the first-occurrence representatives by key: the classes by label, the cells by (true, predicted).  Every
// representative writes its term to LDS at its rank and three lanes add the three lists from the left, one term after
// the other: the written order of the host statement.  Nothing is fused (contraction is off in this file) and every
// logarithm is read from the table the host uploaded (mpe_set_log_table).
#include "mpe_internal.h"

#pragma clang fp contract(off)

namespace mpe {

namespace {

// ---- labels -----------------------------------------------------------------------------------------------------------
struct PartLabelsK {
    int n_frames, pcap, hcap, V;
    const int32_t *frame_head_off, *persons, *n_persons;
    int32_t *labels, *count, *status;
};

__global__ void __launch_bounds__(256) k_part_labels(PartLabelsK a) {
    const long long total = (long long)a.n_frames * a.hcap;
    for (long long i = (long long)blockIdx.x * 256 + threadIdx.x; i < total; i += (long long)gridDim.x * 256) {
        const int f = (int)(i / a.hcap), h = (int)(i - (long long)f * a.hcap);
        const int H = a.frame_head_off[f + 1] - a.frame_head_off[f];
        int lab = -1;
        if (h < H) {
            const int np = min(max(a.n_persons[f], 0), a.pcap);
            const int32_t *row = a.persons + (size_t)f * a.pcap * a.V;
            lab = np;
            for (int p = 0; p < np && lab == np; ++p)
                for (int c = 0; c < a.V; ++c)
                    if (row[p * a.V + c] == h) { lab = p; break; }
        }
        a.labels[i] = lab;
        if (h == 0) {
            a.count[f] = H;
            a.status[f] = H > a.hcap ? MPE_PART_OVER_CAP : 0;
        }
    }
}

// ---- ground-truth grouping --------------------------------------------------------------------------------------------
struct PartGroupK {
    int scap, kcap;
    const double *xyz;
    const uint32_t *mask;
    const int32_t *nkeys;
    const uint8_t *order, *m1;
    const int32_t *n;
    const uint8_t *skip_in;
    int32_t *labels, *n_groups;
    uint8_t *skip;
    int32_t *status;
};

__global__ void __launch_bounds__(64) k_part_group(PartGroupK a) {
    __shared__ int32_t s_founder[MPE_PART_MAX_SKELETONS];
    const int f = blockIdx.x, lane = threadIdx.x;
    const int S = min(max(a.n[f], 0), a.scap);
    const bool skip_in = a.skip_in && a.skip_in[f];
    const bool over = S > MPE_PART_MAX_SKELETONS;
    int32_t *lab = a.labels + (size_t)f * a.scap;
    // every label is written once: -1 beyond the frame's skeletons (all of them on a frame that is not grouped)
    for (int s = ((skip_in || over) ? 0 : S) + lane; s < a.scap; s += 64) lab[s] = -1;
    if (skip_in || over) {
        if (lane == 0) {
            a.n_groups[f] = 0;
            a.skip[f] = 1;
            a.status[f] = over ? MPE_PART_OVER_CAP : MPE_PART_SKIPPED;
        }
        return;
    }
    const double *X = a.xyz + (size_t)f * a.scap * a.kcap * 3;
    const uint32_t *M = a.mask + (size_t)f * a.scap;
    const int32_t *NK = a.nkeys + (size_t)f * a.scap;
    const uint8_t *ORD = a.order + (size_t)f * a.scap * a.kcap;
    const uint8_t *M1 = a.m1 + (size_t)f * a.scap;
    int bad = 0;
    for (int s = lane; s < S; s += 64) bad |= M1[s] == 0;
    const bool invalid = __ballot(bad) != 0;
    int G = 0;                                   // the same in every lane
    for (int s = 0; s < S; ++s) {
        const uint32_t ms = M[s];
        const double *xs = X + (size_t)s * a.kcap * 3;
        double best = 1000000000.;
        int matched = -1, nj = 0;
        for (int base = 0; base < G; base += 64) {
            const int pid = base + lane;
            if (pid >= G) continue;
            const int q = s_founder[pid];
            const double *xq = X + (size_t)q * a.kcap * 3;
            const int nk = min(max(NK[q], 0), a.kcap);
            double dist = 0.0;
            int cnt = 0;
            for (int i = 0; i < nk; ++i) {
                const int k = ORD[(size_t)q * a.kcap + i];
                if (k >= a.kcap || !((ms >> k) & 1u)) continue;
                const double dx = xs[3 * k] - xq[3 * k];
                const double dy = xs[3 * k + 1] - xq[3 * k + 1];
                const double dz = xs[3 * k + 2] - xq[3 * k + 2];
                double sq = dx * dx;
                sq = fma(dy, dy, sq);
                sq = fma(dz, dz, sq);
                dist = dist + sqrt(sq);
                ++cnt;
            }
            if (dist < best) best = dist, matched = pid, nj = cnt;
        }
        for (int off = 32; off > 0; off >>= 1) {
            const double ob = __shfl_xor(best, off);
            const int om = __shfl_xor(matched, off), on = __shfl_xor(nj, off);
            if (om >= 0 && (matched < 0 || ob < best || (ob == best && om < matched))) best = ob, matched = om, nj = on;
        }
        if (nj == 0 || best / (double)nj > 1.) matched = -1;
        if (matched < 0) {
            matched = G;
            if (lane == 0) s_founder[G] = s;
            ++G;
            __syncthreads();
        }
        if (lane == 0) lab[s] = matched;
    }
    if (lane == 0) {
        a.n_groups[f] = G;
        a.skip[f] = (G == 0 || invalid) ? 1 : 0;
        a.status[f] = 0;
    }
}

// ---- scores -----------------------------------------------------------------------------------------------------------
struct PartScoresK {
    int ld_true, ld_pred, n_log;
    const int32_t *lt, *lp, *count, *count_true;
    const uint8_t *skip;
    const double *lg;
    double *scores;
    int32_t *status;
};

__device__ inline int wave_sum(int v) {
    for (int off = 32; off > 0; off >>= 1) v += __shfl_xor(v, off);
    return v;
}

template <int NT>
__global__ void __launch_bounds__(NT) k_part_scores(PartScoresK a) {
    __shared__ int32_t s_t[NT], s_p[NT];
    __shared__ uint8_t s_flag[NT];
    __shared__ double s_term[3][NT];
    __shared__ int s_acc[6];                     // sum a_i, sum b_i, sum c_i, true classes, predicted classes, cells
    __shared__ double s_sum[3];
    const int f = blockIdx.x, i = threadIdx.x;
    const int n = a.count[f];
    const bool skip = (a.skip && a.skip[f]) || n <= 0 || (a.count_true && a.count_true[f] != n);
    const bool over = !skip && (n > NT || n > a.ld_true || n > a.ld_pred || (long long)n * n > a.n_log);
    if (skip || over) {
        if (i < 4) a.scores[(size_t)f * 4 + i] = __builtin_nan("");
        if (i == 0) a.status[f] = over ? MPE_PART_OVER_CAP : MPE_PART_SKIPPED;
        return;
    }
    const bool on = i < n;
    const int ti = on ? a.lt[(size_t)f * a.ld_true + i] : 0, pi = on ? a.lp[(size_t)f * a.ld_pred + i] : 0;
    s_t[i] = ti;
    s_p[i] = pi;
    if (i < 6) s_acc[i] = 0;
    __syncthreads();
    int ai = 0, bi = 0, ci = 0;
    bool fT = on, fP = on, fC = on;
    if (on) {
        for (int k = 0; k < n; ++k) {
            const bool et = s_t[k] == ti, ep = s_p[k] == pi;
            ai += et;
            bi += ep;
            ci += et && ep;
            if (k < i) {
                if (et) fT = false;
                if (ep) fP = false;
                if (et && ep) fC = false;
            }
        }
    }
    s_flag[i] = (uint8_t)((fT ? 1 : 0) | (fP ? 2 : 0) | (fC ? 4 : 0));
    {
        const int v[6] = {ai, bi, ci, fT ? 1 : 0, fP ? 1 : 0, fC ? 1 : 0};
        for (int k = 0; k < 6; ++k) {
            const int w = wave_sum(v[k]);
            if ((i & 63) == 0 && w) atomicAdd(&s_acc[k], w);
        }
    }
    __syncthreads();
    int rT = 0, rP = 0, rC = 0;
    if (fT || fP || fC) {
        for (int k = 0; k < n; ++k) {
            const int fl = s_flag[k], tk = s_t[k], pk = s_p[k];
            rT += (fl & 1) && tk < ti;
            rP += (fl & 2) && pk < pi;
            rC += (fl & 4) && (tk < ti || (tk == ti && pk < pi));
        }
    }
    const double dn = (double)n, log_n = a.lg[n - 1];
    if (fT) s_term[0][rT] = ((double)ai / dn) * (a.lg[ai - 1] - log_n);
    if (fP) s_term[1][rP] = ((double)bi / dn) * (a.lg[bi - 1] - log_n);
    if (fC) {
        const double nm = (double)ci / dn;
        double t = nm * (a.lg[ci - 1] - log_n) + nm * (((-a.lg[ai * bi - 1]) + log_n) + log_n);
        if (fabs(t) < 2.220446049250313e-16) t = 0.0;
        s_term[2][rC] = t;
    }
    __syncthreads();
    if (i < 3) {                                  // three lanes, three lists, each from the left
        const int cnt = s_acc[3 + i];
        double acc = 0.0;
        for (int k = 0; k < n; ++k)
            if (k < cnt) acc = acc + s_term[i][k];
        s_sum[i] = acc;
    }
    __syncthreads();
    if (i == 0) {
        const long long N = n, sa = s_acc[0], sb = s_acc[1], ss = s_acc[2];
        const long long tp = ss - N, fp = sb - ss, fn = sa - ss, tn = N * N - fp - fn - ss;
        const double ari = (fn == 0 && fp == 0) ? 1.0
                                                : (2.0 * (double)(tp * tn - fn * fp)) / (double)((tp + fn) * (fn + tn) + (tp + fp) * (fp + tn));
        const int nT = s_acc[3], nP = s_acc[4];
        const double h_true = nT == 1 ? 0.0 : -s_sum[0], h_pred = nP == 1 ? 0.0 : -s_sum[1];
        const double mi = (nT > 1 && nP > 1 && s_sum[2] > 0.0) ? s_sum[2] : 0.0;
        const double h = h_true != 0.0 ? mi / h_true : 1.0;
        const double c = h_pred != 0.0 ? mi / h_pred : 1.0;
        const double v = (h + c == 0.0) ? 0.0 : ((2.0 * h) * c) / (h + c);
        double *o = a.scores + (size_t)f * 4;
        o[0] = ari, o[1] = h, o[2] = c, o[3] = v;
        a.status[f] = 0;
    }
}

}  // namespace

hipError_t launch_partition_labels(hipStream_t s, int V, const mpe_batch &b, const mpe_partition_labels_args &x) {
    PartLabelsK a{x.n_frames, x.pcap, x.hcap, V, b.d_frame_head_off, x.d_persons, x.d_n_persons, x.d_labels, x.d_count, x.d_status};
    const long long blocks = ((long long)x.n_frames * x.hcap + 255) / 256;
    hipLaunchKernelGGL(k_part_labels, dim3((unsigned)(blocks < 65536 ? blocks : 65536)), dim3(256), 0, s, a);
    return hipGetLastError();
}

hipError_t launch_group_bodies(hipStream_t s, const mpe_group_bodies_args &x) {
    PartGroupK a{x.scap, x.kcap, x.d_xyz, x.d_mask, x.d_nkeys, x.d_order, x.d_m1, x.d_n, x.d_skip_in, x.d_labels, x.d_n_groups, x.d_skip, x.d_status};
    hipLaunchKernelGGL(k_part_group, dim3((unsigned)x.n_frames), dim3(64), 0, s, a);
    return hipGetLastError();
}

hipError_t launch_partition_scores(hipStream_t s, const mpe_partition_scores_args &x, const double *log_table, int n_log) {
    PartScoresK a{x.ld_true, x.ld_pred, n_log, x.d_labels_true, x.d_labels_pred, x.d_count, x.d_count_true, x.d_skip, log_table, x.d_scores, x.d_status};
    if (x.ld_true <= 64 || x.ld_pred <= 64)
        hipLaunchKernelGGL(k_part_scores<64>, dim3((unsigned)x.n_frames), dim3(64), 0, s, a);
    else
        hipLaunchKernelGGL(k_part_scores<MPE_PART_MAX_SAMPLES>, dim3((unsigned)x.n_frames), dim3(MPE_PART_MAX_SAMPLES), 0, s, a);
    return hipGetLastError();
}

}  // namespace mpe
