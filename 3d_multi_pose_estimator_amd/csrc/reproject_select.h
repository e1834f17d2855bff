// Which (frame, person, camera, joint) entries mpe_reproject_batch counts (include/mpe.h has the rule), in three steps so
// that a kernel can read the per-person and per-camera words once and keep the per-joint test for the lane that owns the
// joint.  reproject.hip (one half wave per (frame, person, camera)), refine.hip (one per (frame, person)), skel_refine.hip
// and calib.hip select by it; regroup.hip and frame_rows.h carry its fields.
#pragma once
#include "mpe_internal.h"

namespace mpe {

struct Selection {
    int V, J, joint_flags;
    uint32_t joint_mask;
    float threshold;
    const int32_t *frame_head_off;
    const uint32_t *head_joint_mask;
    const float *vp;
    const int32_t *persons, *n_persons;
    const uint8_t *flags;
};

// row p of frame f holds a person whose joints may count (fp = f * pcap + p)
__device__ inline bool sel_person(const Selection &s, int f, int p, long long fp) {
    return p < s.n_persons[f] && (s.joint_flags || s.flags[fp] != 0);
}

// the head (index into the batch's per-head arrays) that camera c has for that person, -1 without one; *present: the
// joints of that skeleton that are asked for
__device__ inline int sel_head(const Selection &s, int f, long long fp, int c, uint32_t *present) {
    const int h0 = s.frame_head_off[f], h1 = s.frame_head_off[f + 1];
    const int id = s.persons[fp * s.V + c];
    *present = 0;
    if (id < 0 || id >= h1 - h0) return -1;
    *present = s.head_joint_mask[h0 + id] & s.joint_mask;
    return h0 + id;
}

// joint j of that head counts
__device__ inline bool sel_joint(const Selection &s, long long fp, int j, int head, uint32_t present) {
    bool take = head >= 0 && ((present >> j) & 1u);
    if (take && s.joint_flags) take = s.flags[fp * s.J + j] != 0;
    if (take) take = s.vp[((size_t)head * s.J + j) * 2] > s.threshold;
    return take;
}

}  // namespace mpe
