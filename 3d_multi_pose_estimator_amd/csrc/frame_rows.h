// The person rows of one frame as k_regroup and k_consolidate open them, stated once: DESIGN.md 2.2.  One workgroup per
// frame; the rows [pcap][V], one named-bit per head and the persons' pose flags are the caller's LDS arrays, and the caller
// keeps its barriers: one after frame_rows_load (with whatever else it clears), one after frame_rows_mark, and only then
// frame_rows_copy.  Every lane of the workgroup calls all three.  Integer logic only.
#pragma once
#include "mpe_internal.h"
#include "reproject_select.h"

namespace mpe {

constexpr int NAMED_WORDS = 1024;             // one bit per head of a frame: max_heads_per_frame <= 32767 (mpe_create)
static_assert(NAMED_WORDS * 32 > 32767, "a bit for every head of a frame");
// bytes of LDS: the rows, the named bits, the pose flags, the bad-rows word
constexpr int FRAME_ROWS_LDS = MPE_REGROUP_MAX_PERSONS * MPE_MAX_CAMERAS * 4 + NAMED_WORDS * 4 + MPE_REGROUP_MAX_PERSONS + 4;

struct FrameRows {
    int h0, H;                                // the frame's heads: the first, how many
    int np_raw, np;                           // n_persons as given, and held within 0 .. pcap (pose_rows.h: rows_in_frame's rule)
    bool over;                                // more heads than max_heads_per_frame: the frame is copied through
    size_t fp0;                               // f * pcap
};

// the rows into s_row, s_pose[p] = row p has a pose, the named bits of the frame's heads and *s_bad cleared
template <int THREADS>
__device__ inline FrameRows frame_rows_load(const Selection &s, int pcap, int hmax, int f, int32_t *s_row, uint8_t *s_pose, uint32_t *s_named,
                                            int32_t *s_bad) {
    const int tid = threadIdx.x;
    FrameRows r;
    r.h0 = s.frame_head_off[f];
    r.H = s.frame_head_off[f + 1] - r.h0;
    r.np_raw = s.n_persons[f];
    r.np = min(max(r.np_raw, 0), pcap);
    r.over = r.H > hmax;
    r.fp0 = (size_t)f * pcap;
    for (int i = tid; i < pcap * s.V; i += THREADS) s_row[i] = s.persons[r.fp0 * s.V + i];
    for (int p = tid; p < pcap; p += THREADS) s_pose[p] = p < r.np && (s.joint_flags || s.flags[r.fp0 + p] != 0);
    if (!r.over)
        for (int w = tid; w < (r.H + 31) / 32; w += THREADS) s_named[w] = 0;
    if (tid == 0) *s_bad = 0;
    return r;
}

// the rows checked, every named head marked: an entry past the frame's heads, of another camera's head, or naming a head a
// second time sets *s_bad
template <int THREADS>
__device__ inline void frame_rows_mark(const FrameRows &r, int V, const int32_t *head_cam, const int32_t *s_row, uint32_t *s_named, int32_t *s_bad) {
    if (r.over) return;
    for (int i = threadIdx.x; i < r.np * V; i += THREADS) {
        const int e = s_row[i], c = i % V;
        if (e < 0) continue;
        bool bad = e >= r.H || head_cam[r.h0 + e] != c;
        if (!bad) bad = ((atomicOr(&s_named[e >> 5], 1u << (e & 31)) >> (e & 31)) & 1u) != 0;
        if (bad) *s_bad = 1;
    }
}

// the frame is copied through: over the head cap, or its rows are bad
__device__ inline bool frame_rows_copy(const FrameRows &r, const int32_t *s_bad) { return r.over || *s_bad != 0; }

}  // namespace mpe
