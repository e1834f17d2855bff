// The pose rows the sequence stages read (track, relink, smooth, eval, track_score), stated once: DESIGN.md 2.1.
// Integer and predicate logic only.  What makes a row a detection differs from stage to stage and stays in the stage;
// so does every line of arithmetic on the coordinates.  skel.hip keeps its own copy of these fields and tests: with
// PoseRows in front of its kernel arguments k_skel_fit measured 1.9 % slower (profiles/pose_rows_timing.txt).
#pragma once

#include <cstdint>

#include "project64.h"                // Bits<T> and finite3, the one definition of each (every including file has contraction off)

namespace mpe {

struct PoseRows {
    int n_frames, pcap, J, pose_f64, joint_flags;
    const void *poses;               // [n_frames][pcap][J][3] f32, f64 with pose_f64; null in a stage that reads no coordinates
    const uint8_t *flags;            // [n_frames][pcap], with joint_flags [n_frames][pcap][J]
    const int32_t *n_persons;        // [n_frames]
    const int32_t *tid;              // [n_frames][pcap] track ids; null in a stage that reads none
};

// the low J bits
__host__ __device__ inline uint32_t joint_bits(int J) { return J >= 32 ? 0xFFFFFFFFu : (1u << J) - 1u; }

// rows of frame f that can be detections: n_persons, held within 0 .. pcap
__device__ inline int rows_in_frame(const PoseRows &r, int f) { return min(max(r.n_persons[f], 0), r.pcap); }

// the joints the flags of row fp = f * pcap + p name: per-row flags name all J or none, per-joint flags the joints set
__device__ inline uint32_t flag_mask(const PoseRows &r, size_t fp) {
    if (!r.joint_flags) return r.flags[fp] ? joint_bits(r.J) : 0u;
    uint32_t m = 0;
    for (int j = 0; j < r.J; ++j)
        if (r.flags[fp * r.J + j]) m |= 1u << j;
    return m;
}

// joint j of row fp when the row is a detection: a per-row flag stands for every joint
__device__ inline bool joint_flag(const PoseRows &r, size_t fp, int j) { return !r.joint_flags || r.flags[fp * r.J + j] != 0; }

}  // namespace mpe
