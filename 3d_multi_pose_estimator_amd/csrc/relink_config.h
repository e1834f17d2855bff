// What mpe_relink_create checks of its configuration and the copy it keeps: host code only, no device call, so a
// stand-alone program can run it under the host sanitizers (tests/native/relink_config_test.cpp).
#pragma once

#include <cmath>
#include <cstdint>
#include <cstdio>
#include <vector>

#include "../../include/mpe.h"

namespace mpe {

// MPE_OK, or the code mpe_relink_create returns with the reason in why[n]
inline int relink_check_config(const mpe_relink_config *cfg, char *why, size_t n) {
    if (!cfg || !cfg->bones) {
        snprintf(why, n, "NULL argument");
        return MPE_ERR_INVALID;
    }
    if (cfg->pcap < 1 || cfg->n_joints < 1 || cfg->n_joints > MPE_MAX_JOINTS || (cfg->pose_f64 & ~1) || cfg->tid_cap < 1 || cfg->n_bones < 1 ||
        cfg->n_bones > MPE_SKEL_MAX_BONES || cfg->max_frames < 1) {
        snprintf(why, n, "pcap %d / joints %d / pose_f64 %d / tid_cap %d / n_bones %d / max_frames %d; joints 1 .. %d, bones 1 .. %d", cfg->pcap,
                 cfg->n_joints, cfg->pose_f64, cfg->tid_cap, cfg->n_bones, cfg->max_frames, MPE_MAX_JOINTS, MPE_SKEL_MAX_BONES);
        return MPE_ERR_INVALID;
    }
    for (int b = 0; b < cfg->n_bones; ++b) {
        const int32_t jp = cfg->bones[2 * b], jc = cfg->bones[2 * b + 1];
        if (jp < 0 || jp >= cfg->n_joints || jc < 0 || jc >= cfg->n_joints || jp == jc) {
            snprintf(why, n, "bone %d is (%d, %d); two different joints within 0 .. %d", b, jp, jc, cfg->n_joints - 1);
            return MPE_ERR_INVALID;
        }
    }
    const double d[4] = {cfg->gate_m, cfg->max_bone_m, cfg->reach_m, cfg->reach_per_frame_m};
    for (int i = 0; i < 4; ++i)
        if (!std::isfinite(d[i]) || d[i] < 0.0 || (i < 2 && !(d[i] > 0.0))) {
            snprintf(why, n, "gate_m %g / max_bone_m %g / reach_m %g / reach_per_frame_m %g; finite, the first two > 0, the others >= 0", d[0], d[1],
                     d[2], d[3]);
            return MPE_ERR_INVALID;
        }
    if (cfg->min_gap < 1 || cfg->max_gap < cfg->min_gap || cfg->max_gap > MPE_RELINK_MAX_GAP || cfg->min_samples < 1 || cfg->min_bones < 1 ||
        cfg->min_bones > cfg->n_bones) {
        snprintf(why, n, "min_gap %d / max_gap %d / min_samples %d / min_bones %d; 1 <= min_gap <= max_gap <= %d, min_samples >= 1, min_bones 1 .. %d",
                 cfg->min_gap, cfg->max_gap, cfg->min_samples, cfg->min_bones, MPE_RELINK_MAX_GAP, cfg->n_bones);
        return MPE_ERR_INVALID;
    }
    if (cfg->pcap > MPE_TRACK_MAX_PERSONS || cfg->tid_cap > MPE_RELINK_MAX_TID_CAP || cfg->max_frames > (1 << 23)) {
        snprintf(why, n, "pcap %d / tid_cap %d / max_frames %d over %d / %d / 2^23", cfg->pcap, cfg->tid_cap, cfg->max_frames, MPE_TRACK_MAX_PERSONS,
                 MPE_RELINK_MAX_TID_CAP);
        return MPE_ERR_CAPACITY;
    }
    return MPE_OK;
}

// the copy the state keeps: the bone list moves into `bones` and the copy points at it
inline mpe_relink_config relink_copy_config(const mpe_relink_config &cfg, std::vector<int32_t> *bones) {
    bones->assign(cfg.bones, cfg.bones + 2 * (size_t)cfg.n_bones);
    mpe_relink_config c = cfg;
    c.bones = bones->data();
    return c;
}

}  // namespace mpe
