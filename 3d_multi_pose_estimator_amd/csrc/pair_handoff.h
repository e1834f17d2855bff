// The bookkeeping of the pair hand-off between mpe_match_batch and mpe_mlp3d_batch (small batches): which batch the pair
// solves of k_lat_tail belong to, and when they may be fetched.  Host code only, no device call, so a stand-alone program can
// walk the rule under the host sanitizers (tests/native/pair_handoff_test.cpp).
//
// The rule (include/mpe.h states the caller's side of it, at mpe_mlp3d_batch):
//   * mpe_match_batch NOTES the batch whose pairs it solved: every array pointer of the mpe_batch, its generation, its three
//     counts, and the persons / n_persons arrays it wrote.
//   * every entry point that takes an mpe_batch FORGETS the note before it does anything else (mpe_match_batch too: it
//     notes again at its end); so a note survives only from one mpe_match_batch to the very next batch call of the context.
//   * mpe_mlp3d_batch TAKES the note: it fetches when every noted item equals what it was handed, and the note is gone
//     either way -- a hand-off is used once.
// One note per context; two buffers, taken in turn, because the row kernel of batch i may still read its buffer on one stream
// while k_lat_tail of batch i+1 writes on another.
#pragma once

#include <stdint.h>

#include "../../include/mpe.h"

namespace mpe {

struct PairKey {
    const void *arrays[10] = {};      // the batch's ten array pointers, in the order of mpe_batch
    uint64_t generation = 0;          // mpe_batch::generation: the caller changes it when it rewrites the arrays in place
    int32_t n_frames = 0, n_heads = 0, n_edge_nodes = 0;
    const void *persons = nullptr, *n_persons = nullptr;      // what mpe_match_batch wrote / what mpe_mlp3d_batch is handed
};

inline PairKey pair_key(const mpe_batch &b, const void *persons, const void *n_persons) {
    PairKey k;
    const void *a[10] = {b.d_frame_head_off, b.d_frame_en_off, b.d_slot_cam, b.d_slot_n, b.d_head_cam,
                         b.d_joint_mask,     b.d_tri_mask,     b.d_xy,       b.d_vp,     b.d_en_pair};
    for (int i = 0; i < 10; ++i) k.arrays[i] = a[i];
    k.generation = b.generation;
    k.n_frames = b.n_frames;
    k.n_heads = b.n_heads;
    k.n_edge_nodes = b.n_edge_nodes;
    k.persons = persons;
    k.n_persons = n_persons;
    return k;
}

inline bool pair_key_equal(const PairKey &a, const PairKey &b) {
    for (int i = 0; i < 10; ++i)
        if (a.arrays[i] != b.arrays[i]) return false;
    return a.generation == b.generation && a.n_frames == b.n_frames && a.n_heads == b.n_heads && a.n_edge_nodes == b.n_edge_nodes &&
           a.persons == b.persons && a.n_persons == b.n_persons;
}

struct PairHandoff {
    PairKey key;
    int held = -1;                    // the buffer (0 / 1) that holds the noted batch's pairs, -1: no note
    int next = 0;                     // the buffer the next mpe_match_batch writes

    void forget() { held = -1; }
    int write_slot() const { return next; }
    // mpe_match_batch, after the launch that filled buffer write_slot()
    void note(const PairKey &k) {
        key = k;
        held = next;
        next ^= 1;
    }
    // mpe_mlp3d_batch: the buffer to fetch from, or -1 = solve; the note is gone either way
    int take(const PairKey &k) {
        const int slot = (held >= 0 && pair_key_equal(key, k)) ? held : -1;
        held = -1;
        return slot;
    }
};

}  // namespace mpe
