// The pose document written on the device (include/mpe.h: mpe_json_write_poses; the numpy / json.dumps statement is
// harness/write_poses.py): one line per frame, {"frame": n, "ids": [..], "bodies": [{"<j>": [x, y, z], ..}, ..]}, every
// number the shortest decimal that reads back to the same double (fmt_double.h), every byte where json.dumps puts it.
// Five launches whatever the frames hold; byte positions come from sums and prefix sums, nothing is placed by an atomic,
// and every number is converted once:
//
// k_write_convert   one thread per coordinate.  A coordinate of a row within n_persons whose joint is flagged and in the
//                   mask is scaled (one IEEE multiply) and converted into its 32-byte slot of the scratch; its length
//                   byte says what became of it: 0 not looked at, 1 .. 24 the token's bytes, 255 not finite.
// k_write_rows      one thread per row: the joints whose three lengths are tokens, the bytes of the row's body, and
//                   whether a flagged joint was dropped.
// k_write_frames    one thread per frame: rows written, status and the bytes of the line.
// k_write_scan      one workgroup: the exclusive prefix sum of the line lengths (d_frame_off), the total, the OR of the
//                   statuses and the capacity bit.
// k_write_assemble  one workgroup per frame.  A prefix sum over the rows places the ids and the bodies, then one thread
//                   per (row, joint) copies the three tokens with their punctuation.  A line of up to
//                   MPE_JSON_WRITE_STAGE_BYTES is put together in LDS, at the offset that gives LDS and global address
//                   the same remainder mod 16, and leaves in 16-byte stores (bytes at the two ends); a longer line is
//                   written to global memory byte by byte.  Nothing is stored at or behind text_cap on either path.
#include "mpe_internal.h"
#include "pose_rows.h"
#include "fmt_double.h"

#pragma clang fp contract(off)

namespace mpe {

namespace {

constexpr int WR_SLOT = MPE_JSON_WRITE_SLOT_BYTES;
constexpr int WR_PCAP = MPE_JSON_WRITE_MAX_PERSONS;
constexpr int WR_STAGE = MPE_JSON_WRITE_STAGE_BYTES;
constexpr uint8_t WR_NONFINITE = 255;

struct WriteK : PoseRows {
    uint32_t jmask;                  // joint_mask, cut to the J joints
    int64_t frame_start;
    double scale;
    char *text;
    uint64_t text_cap;
    int64_t *frame_off;
    uint32_t *extent;
    int32_t *rows_written, *status;
    int64_t *total;
    // scratch
    char *slots;                     // [n_frames][pcap][J][3][32]
    uint8_t *len;                    // [n_frames][pcap][J][3]
    uint32_t *row_len, *row_mask;    // [n_frames][pcap]: bytes of the body with its braces (0: not written), written joints
    uint8_t *row_stat;               // [n_frames][pcap]
    int64_t *frame_len;              // [n_frames]
};

template <typename T>
__device__ inline uint64_t scaled_bits(T x, double scale) {
    const double v = (double)x * scale;
    uint64_t b;
    __builtin_memcpy(&b, &v, 8);
    return b;
}

template <typename T>
__global__ void __launch_bounds__(256) k_write_convert(WriteK a, size_t n) {
    const size_t i = (size_t)blockIdx.x * 256 + threadIdx.x;
    if (i >= n) return;
    const size_t e = i / 3, fp = e / a.J;
    const int j = (int)(e - fp * a.J), f = (int)(fp / a.pcap), p = (int)(fp - (size_t)f * a.pcap);
    uint8_t l = 0;
    if (p < rows_in_frame(a, f) && ((a.jmask >> j) & 1u) && (a.joint_flags ? a.flags[e] : a.flags[fp])) {
        const int t = fmt_double(scaled_bits(static_cast<const T *>(a.poses)[i], a.scale), a.slots + i * WR_SLOT);
        l = t ? (uint8_t)t : WR_NONFINITE;
    }
    a.len[i] = l;
}

__global__ void __launch_bounds__(256) k_format_f64(const double *v, size_t n, char *slots, uint8_t *len) {
    const size_t i = (size_t)blockIdx.x * 256 + threadIdx.x;
    if (i >= n) return;
    len[i] = (uint8_t)fmt_double(scaled_bits(v[i], 1.0), slots + i * WR_SLOT);
}

// `"<j>": [x, y, z]`
__device__ inline uint32_t joint_bytes(int j, const uint8_t *l) { return (j < 10 ? 3u : 4u) + 8u + l[0] + l[1] + l[2]; }

__global__ void __launch_bounds__(256) k_write_rows(WriteK a, size_t n_rows) {
    const size_t fp = (size_t)blockIdx.x * 256 + threadIdx.x;
    if (fp >= n_rows) return;
    const int f = (int)(fp / a.pcap), p = (int)(fp - (size_t)f * a.pcap);
    uint32_t wm = 0, bytes = 0;
    uint8_t st = 0;
    if (p < rows_in_frame(a, f))
        for (int j = 0; j < a.J; ++j) {
            const uint8_t *l = a.len + (fp * a.J + j) * 3;
            if (!l[0]) continue;                         // the three coordinates of a joint are looked at together
            if (l[0] == WR_NONFINITE || l[1] == WR_NONFINITE || l[2] == WR_NONFINITE) {
                st = MPE_WRITE_NONFINITE;
                continue;
            }
            bytes += (wm ? 2u : 0u) + joint_bytes(j, l);
            wm |= 1u << j;
        }
    a.row_len[fp] = wm ? bytes + 2u : 0u;
    a.row_mask[fp] = wm;
    a.row_stat[fp] = st;
}

// the bytes in front of the ids and of the bodies: `{"frame": `, `, "ids": [`, `, "bodies": [`; behind them `]` and `]}\n`
constexpr uint32_t WR_HEAD = 10, WR_IDS = 10, WR_BODIES = 13, WR_TAIL = 3;

__global__ void __launch_bounds__(256) k_write_frames(WriteK a) {
    const int f = blockIdx.x * 256 + threadIdx.x;
    if (f >= a.n_frames) return;
    int nw = 0, st = 0;
    int64_t body = 0, idb = 0;
    for (int p = 0; p < a.pcap; ++p) {
        const size_t fp = (size_t)f * a.pcap + p;
        st |= a.row_stat[fp];
        const uint32_t rl = a.row_len[fp];
        if (!rl) continue;
        ++nw;
        body += rl;
        if (a.tid) idb += fmt_int64_len(a.tid[fp]);
    }
    const int64_t sep = nw ? 2 * (nw - 1) : 0;
    int64_t len = WR_HEAD + fmt_int64_len(a.frame_start + f) + WR_BODIES + body + sep + WR_TAIL;
    if (a.tid) len += WR_IDS + idb + sep + 1;
    a.rows_written[f] = nw;
    a.status[f] = st;
    a.frame_len[f] = len;
}

// inclusive prefix sum over the 1024 threads of a workgroup; s_w holds one value per wave
__device__ inline int64_t block_scan_1024(int64_t v, int64_t *s_w) {
    const int lane = threadIdx.x & 63, w = threadIdx.x >> 6;
    for (int d = 1; d < 64; d <<= 1) {
        const int64_t u = __shfl_up(v, d, 64);
        if (lane >= d) v += u;
    }
    __syncthreads();                                     // s_w of the round before has been read
    if (lane == 63) s_w[w] = v;
    __syncthreads();
    for (int k = 0; k < w; ++k) v += s_w[k];
    return v;
}

__global__ void __launch_bounds__(1024) k_write_scan(WriteK a) {
    __shared__ int64_t s_w[16];
    __shared__ int s_st[16];
    int64_t base = 0;
    int st = 0;
    for (int f0 = 0; f0 < a.n_frames; f0 += 1024) {
        const int f = f0 + threadIdx.x;
        const int64_t len = f < a.n_frames ? a.frame_len[f] : 0;
        if (f < a.n_frames) st |= a.status[f];
        const int64_t incl = block_scan_1024(len, s_w);
        if (f < a.n_frames) a.frame_off[f] = base + incl - len;
        int64_t all = 0;
        for (int k = 0; k < 16; ++k) all += s_w[k];
        base += all;
    }
    for (int d = 1; d < 64; d <<= 1) st |= __shfl_xor(st, d, 64);
    if ((threadIdx.x & 63) == 0) s_st[threadIdx.x >> 6] = st;
    __syncthreads();
    if (threadIdx.x == 0) {
        for (int k = 1; k < 16; ++k) st |= s_st[k];
        if ((uint64_t)base > a.text_cap) st |= MPE_WRITE_CAPACITY;
        a.frame_off[a.n_frames] = base;
        a.total[0] = base;
        a.total[1] = st;
    }
}

// where the bytes of a line go: LDS (the line leaves later, in wide pieces) or global memory, below text_cap only
template <bool STAGED>
struct LineOut {
    char *lds;                       // STAGED: byte 0 of the line
    char *g;                         // byte 0 of the line in d_text
    uint32_t room;                   // STAGED: the bytes of the line; otherwise those of them below text_cap
    __device__ inline void put(uint32_t at, char c) const {
        if (at >= room) return;
        if (STAGED) lds[at] = c;
        else g[at] = c;
    }
    __device__ inline uint32_t str(uint32_t at, const char *s, uint32_t n) const {
        for (uint32_t k = 0; k < n; ++k) put(at + k, s[k]);
        return at + n;
    }
    __device__ inline uint32_t num(uint32_t at, int64_t v) const {
        char t[20];
        const int n = fmt_int64(v, t);
        for (int k = 0; k < n; ++k) put(at + k, t[k]);
        return at + n;
    }
};

template <bool STAGED>
__device__ inline void assemble_line(const WriteK &a, int f, const LineOut<STAGED> &o, uint32_t len, int64_t off, uint32_t *s_boff, uint64_t *s_w) {
    const int tx = threadIdx.x, pcap = a.pcap, J = a.J;
    const size_t row0 = (size_t)f * pcap;
    const bool ids = a.tid != nullptr;
    // the rows of thread tx: per = ceil(pcap / 256) consecutive ones; {id bytes, body bytes} of the written ones, each with
    // the two bytes of a separator, summed as one 64-bit pair (ids high: both stay far below 2^32)
    const int per = (pcap + 255) / 256, p0 = tx * per, p1 = min(p0 + per, pcap);
    uint64_t mine = 0;
    for (int p = p0; p < p1; ++p) {
        const uint32_t rl = a.row_len[row0 + p];
        if (!rl) continue;
        mine += (uint64_t)(rl + 2u);
        if (ids) mine += (uint64_t)(fmt_int64_len(a.tid[row0 + p]) + 2) << 32;
    }
    uint64_t incl = mine;
    const int lane = tx & 63, w = tx >> 6;
    for (int d = 1; d < 64; d <<= 1) {
        const uint64_t u = __shfl_up(incl, d, 64);
        if (lane >= d) incl += u;
    }
    if (lane == 63) s_w[w] = incl;
    __syncthreads();
    uint64_t all = 0;
    for (int k = 0; k < 4; ++k) {
        if (k < w) incl += s_w[k];
        all += s_w[k];
    }
    uint64_t before = incl - mine;
    // the fixed parts
    const uint32_t nf = (uint32_t)fmt_int64_len(a.frame_start + f);
    const uint32_t id_all = (uint32_t)(all >> 32), body_all = (uint32_t)all;
    const uint32_t ids_at = WR_HEAD + nf + WR_IDS;                                   // first byte behind `"ids": [`
    const uint32_t list_at = WR_HEAD + nf + (ids ? WR_IDS + (id_all ? id_all - 2u : 0u) + 1u : 0u) + WR_BODIES - 1u;   // the `[` of the bodies
    if (tx == 0) {
        uint32_t at = o.str(0, "{\"frame\": ", WR_HEAD);
        at = o.num(at, a.frame_start + f);
        if (ids) {
            at = o.str(at, ", \"ids\": [", WR_IDS);
            at = o.str(at + (id_all ? id_all - 2u : 0u), "]", 1);
        }
        at = o.str(at, ", \"bodies\": [", WR_BODIES);
        o.str(at + (body_all ? body_all - 2u : 0u), "]}\n", WR_TAIL);
        a.extent[2 * (size_t)f] = (uint32_t)(off + list_at);
        a.extent[2 * (size_t)f + 1] = (uint32_t)(off + len - 2);
    }
    // ids, braces and the separators between rows; s_boff[p]: the `{` of row p
    for (int p = p0; p < p1; ++p) {
        const uint32_t rl = a.row_len[row0 + p];
        if (p < WR_PCAP) s_boff[p] = 0;
        if (!rl) continue;
        const uint32_t b = list_at + 1u + (uint32_t)before, i = ids_at + (uint32_t)(before >> 32);
        if (before) {                                    // the two bytes every earlier row counted behind itself
            o.str(b - 2u, ", ", 2);
            if (ids) o.str(i - 2u, ", ", 2);
        }
        if (ids) o.num(i, a.tid[row0 + p]);
        o.put(b, '{');
        o.put(b + rl - 1u, '}');
        s_boff[p] = b;
        before += (uint64_t)(rl + 2u);
        if (ids) before += (uint64_t)(fmt_int64_len(a.tid[row0 + p]) + 2) << 32;
    }
    __syncthreads();
    // the joints
    for (int i = tx; i < pcap * J; i += 256) {
        const int p = i / J, j = i - p * J;
        const uint32_t wm = a.row_mask[row0 + p];
        if (!((wm >> j) & 1u)) continue;
        const uint8_t *l = a.len + (row0 + p) * J * 3;
        uint32_t at = s_boff[p] + 1u;
        for (int k = 0; k < j; ++k)
            if ((wm >> k) & 1u) at += joint_bytes(k, l + 3 * k) + 2u;
        if (wm & ((1u << j) - 1u)) at = o.str(at - 2u, ", ", 2);
        o.put(at++, '"');
        if (j >= 10) o.put(at++, (char)('0' + j / 10));
        o.put(at++, (char)('0' + j % 10));
        at = o.str(at, "\": [", 4);
        const char *slot = a.slots + ((row0 + p) * J + j) * 3 * WR_SLOT;
        for (int c = 0; c < 3; ++c) {
            if (c) at = o.str(at, ", ", 2);
            at = o.str(at, slot + c * WR_SLOT, l[3 * j + c]);
        }
        o.put(at, ']');
    }
}

__global__ void __launch_bounds__(256) k_write_assemble(WriteK a) {
    __shared__ __attribute__((aligned(16))) char s_line[WR_STAGE + 16];
    __shared__ uint32_t s_boff[WR_PCAP];
    __shared__ uint64_t s_w[4];
    const int f = blockIdx.x;
    const int64_t off = a.frame_off[f];
    const uint32_t len = (uint32_t)a.frame_len[f];
    char *g = a.text + off;
    const uint64_t room = (uint64_t)off < a.text_cap ? min((uint64_t)len, a.text_cap - (uint64_t)off) : 0;
    if (len > (uint32_t)WR_STAGE) {
        assemble_line<false>(a, f, LineOut<false>{nullptr, g, (uint32_t)room}, len, off, s_boff, s_w);
        return;
    }
    const uint32_t shift = (uint32_t)((uintptr_t)g & 15u);       // LDS byte shift + k and global byte k: the same remainder mod 16
    assemble_line<true>(a, f, LineOut<true>{s_line + shift, g, len}, len, off, s_boff, s_w);
    __syncthreads();
    // 16-byte pieces of s_line; piece k covers the bytes 16 k - shift .. 16 k - shift + 15 of the line
    const uint32_t end = shift + (uint32_t)room;
    for (uint32_t k = threadIdx.x; 16u * k < end; k += 256) {
        const uint32_t lo = 16u * k, hi = lo + 16u;
        if (lo >= shift && hi <= end) {
            *reinterpret_cast<uint4 *>(g - shift + lo) = *reinterpret_cast<const uint4 *>(s_line + lo);
        } else {
            for (uint32_t b = max(lo, shift); b < min(hi, end); ++b) g[b - shift] = s_line[b];
        }
    }
}

size_t up16(size_t n) { return (n + 15) & ~(size_t)15; }

}  // namespace

size_t json_write_scratch_bytes(int64_t n_frames, int64_t pcap, int64_t J) {
    const size_t rows = (size_t)n_frames * pcap, n = rows * J * 3;
    return n * WR_SLOT + up16(n) + 2 * up16(rows * 4) + up16(rows) + up16((size_t)n_frames * 8);
}

hipError_t launch_format_f64(hipStream_t s, const double *d_values, int64_t n, char *d_slots, uint8_t *d_len) {
    hipLaunchKernelGGL(k_format_f64, dim3((unsigned)((n + 255) / 256)), dim3(256), 0, s, d_values, (size_t)n, d_slots, d_len);
    return hipGetLastError();
}

hipError_t launch_json_write(hipStream_t s, const mpe_json_write_args &x, int64_t *launches) {
    WriteK a{};
    a.n_frames = x.n_frames; a.pcap = x.pcap; a.J = x.n_joints; a.pose_f64 = x.pose_f64; a.joint_flags = x.joint_flags;
    a.poses = x.d_poses; a.flags = x.d_flags; a.n_persons = x.d_n_persons; a.tid = x.d_track_id;
    a.jmask = x.joint_mask & joint_bits(x.n_joints);
    a.frame_start = x.frame_start;
    a.scale = x.scale;
    a.text = x.d_text; a.text_cap = x.text_cap;
    a.frame_off = x.d_frame_off; a.extent = x.d_bodies_extent; a.rows_written = x.d_rows_written; a.status = x.d_status; a.total = x.d_total;
    const size_t rows = (size_t)x.n_frames * x.pcap, n = rows * x.n_joints * 3;
    char *at = static_cast<char *>(x.d_scratch);
    a.slots = at; at += n * WR_SLOT;
    a.len = reinterpret_cast<uint8_t *>(at); at += up16(n);
    a.row_len = reinterpret_cast<uint32_t *>(at); at += up16(rows * 4);
    a.row_mask = reinterpret_cast<uint32_t *>(at); at += up16(rows * 4);
    a.row_stat = reinterpret_cast<uint8_t *>(at); at += up16(rows);
    a.frame_len = reinterpret_cast<int64_t *>(at);
    hipError_t e;
#define WR_LAUNCH(...)                                   \
    hipLaunchKernelGGL(__VA_ARGS__);                     \
    if ((e = hipGetLastError()) != hipSuccess) return e; \
    ++*launches
    if (x.n_frames > 0) {
        const dim3 gn((unsigned)((n + 255) / 256)), gr((unsigned)((rows + 255) / 256)), gf((unsigned)((x.n_frames + 255) / 256));
        if (x.pose_f64) { WR_LAUNCH(k_write_convert<double>, gn, dim3(256), 0, s, a, n); }
        else { WR_LAUNCH(k_write_convert<float>, gn, dim3(256), 0, s, a, n); }
        WR_LAUNCH(k_write_rows, gr, dim3(256), 0, s, a, rows);
        WR_LAUNCH(k_write_frames, gf, dim3(256), 0, s, a);
    }
    WR_LAUNCH(k_write_scan, dim3(1), dim3(1024), 0, s, a);
    if (x.n_frames > 0) { WR_LAUNCH(k_write_assemble, dim3(x.n_frames), dim3(256), 0, s, a); }
#undef WR_LAUNCH
    return hipSuccess;
}

}  // namespace mpe
