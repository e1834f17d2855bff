// Host build of csrc/pair_handoff.h, the bookkeeping of the pair hand-off between mpe_match_batch and mpe_mlp3d_batch, for a
// run under -fsanitize=address,undefined (tests/test_host_logic.py).  A model context makes the calls api.hip makes (every batch
// call forgets, the matching notes, the MLP stage takes) on model batches that remember WHAT their arrays hold; the scenarios
// of tests/test_gpu_history.py run as sequences of such events, and every one says whether the row kernel may fetch.  A fetch of
// pairs that were solved for other contents than the arrays hold is a failure wherever it happens.
// Prints "ok <checks>" and exits 0, or says what differed and exits 1.
#include <cstddef>
#include <cstdio>
#include <cstring>
#include <memory>
#include <vector>

#include "pair_handoff.h"

// (tests/test_host_logic.py asserts the same two numbers of the ctypes struct)
static_assert(offsetof(mpe_batch, generation) == 96 && sizeof(mpe_batch) == 104, "mpe_batch: the generation is the last field");

namespace {

int checks = 0, failures = 0;

struct Arena {                       // ten device arrays at fixed addresses, and what they hold at the moment
    std::unique_ptr<char[]> mem;
    int content = 0;
    Arena() : mem(new char[10]) {}
};

struct Batch {                       // a caller's mpe_batch over an arena (packing.DeviceBatch)
    mpe_batch s;
    Arena *arena;
    static uint64_t generations;
    Batch(Arena *a, int content, int frames, int heads, int en) : arena(a) {
        memset(&s, 0, sizeof s);
        const char *p = a->mem.get();
        s.d_frame_head_off = reinterpret_cast<const int32_t *>(p);
        s.d_frame_en_off = reinterpret_cast<const int32_t *>(p + 1);
        s.d_slot_cam = reinterpret_cast<const int32_t *>(p + 2);
        s.d_slot_n = reinterpret_cast<const int32_t *>(p + 3);
        s.d_head_cam = reinterpret_cast<const int32_t *>(p + 4);
        s.d_joint_mask = reinterpret_cast<const uint32_t *>(p + 5);
        s.d_tri_mask = reinterpret_cast<const uint32_t *>(p + 6);
        s.d_xy = reinterpret_cast<const double *>(p + 7);
        s.d_vp = reinterpret_cast<const float *>(p + 8);
        s.d_en_pair = nullptr;
        upload(content, frames, heads, en);
    }
    // DeviceBatch.upload / rebind: new contents at the same addresses, a new generation
    void upload(int content, int frames, int heads, int en) {
        arena->content = content;
        s.n_frames = frames;
        s.n_heads = heads;
        s.n_edge_nodes = en;
        s.generation = ++generations;
    }
    // what the caller's rule forbids: new contents, equal counts, nothing told
    void rewrite_silently(int content) { arena->content = content; }
};
uint64_t Batch::generations = 0;

struct Ctx {                         // the calls of api.hip, and what each of the two buffers was solved for
    mpe::PairHandoff h;
    int solved_for[2] = {-1, -1};
    void other(const Batch &) { h.forget(); }                                  // check_batch of any entry point
    void match(const Batch &b, const void *persons, const void *n_persons, bool small = true, bool pairs_ok = true) {
        h.forget();                                                            // check_batch
        if (!small) return;                                                    // (the batch route: no tail launch, no note)
        if (!pairs_ok) return;
        solved_for[h.write_slot()] = b.arena->content;
        h.note(mpe::pair_key(b.s, persons, n_persons));
    }
    // -> fetched?  A fetch of another batch's pairs is counted as a failure here, whatever the scenario expects
    bool mlp3d(const Batch &b, const void *persons, const void *n_persons, const char *what) {
        const int slot = h.take(mpe::pair_key(b.s, persons, n_persons));
        h.forget();                                                            // check_batch
        if (slot >= 0 && solved_for[slot] != b.arena->content) {
            printf("%s: STALE fetch (pairs of contents %d, the arrays hold %d)\n", what, solved_for[slot], b.arena->content);
            ++failures;
        }
        return slot >= 0;
    }
};

void expect(bool got, bool want, const char *what) {
    ++checks;
    if (got != want) {
        printf("%s: %s, expected %s\n", what, got ? "fetched" : "solved", want ? "a fetch" : "no fetch");
        ++failures;
    }
}

enum { A = 1, B, C, D, G };          // contents

}  // namespace

int main() {
    // persons / n_persons arrays: heap blocks, only their addresses matter
    std::vector<std::unique_ptr<int32_t[]>> blocks;
    auto fresh = [&]() { blocks.emplace_back(new int32_t[1]); return static_cast<const void *>(blocks.back().get()); };
    const void *p1 = fresh(), *n1 = fresh(), *p2 = fresh(), *n2 = fresh(), *p3 = fresh(), *n3 = fresh();

    {   // the plain sequence, and single use
        Ctx c; Arena ar; Batch b(&ar, A, 3, 60, 480);
        c.match(b, p1, n1);
        expect(c.mlp3d(b, p1, n1, "plain"), true, "match(A); mlp3d(A, persons of the match)");
        expect(c.mlp3d(b, p1, n1, "plain again"), false, "a second mlp3d(A): the hand-off was used");
        c.match(b, p1, n1);
        expect(c.mlp3d(b, p2, n1, "other persons"), false, "match(A); mlp3d(A, other persons array)");
        expect(c.mlp3d(b, p1, n1, "after a miss"), false, "a miss ends the hand-off too");
        c.match(b, p1, n1);
        expect(c.mlp3d(b, p1, n2, "other n_persons"), false, "match(A); mlp3d(A, other n_persons array)");
        c.match(b, p1, n1, false);
        expect(c.mlp3d(b, p1, n1, "batch route"), false, "a match on the batch route leaves nothing");
        c.match(b, p1, n1);
        c.match(b, p1, n1, true, false);
        expect(c.mlp3d(b, p1, n1, "no pairs"), false, "a match that solved no pairs ends the older note and leaves none");
    }
    {   // the two buffers are written in turn
        Ctx c; Arena ar; Batch b(&ar, A, 3, 60, 480);
        ++checks;
        int seq[4];
        for (int i = 0; i < 4; ++i) {
            seq[i] = c.h.write_slot();
            c.match(b, p1, n1);
        }
        if (seq[0] != 0 || seq[1] != 1 || seq[2] != 0 || seq[3] != 1) {
            printf("write slots %d %d %d %d\n", seq[0], seq[1], seq[2], seq[3]);
            ++failures;
        }
        expect(c.mlp3d(b, p1, n1, "turns"), true, "the last of four matches is the one fetched");
    }
    {   // every item of the key counts
        Arena ar, other;
        for (int k = 0; k < 14; ++k) {
            Ctx c; Batch b(&ar, A, 3, 60, 480);
            c.match(b, p1, n1);
            Batch q = b;
            const char *op = other.mem.get();
            switch (k) {
            case 0: q.s.d_frame_head_off = reinterpret_cast<const int32_t *>(op); break;
            case 1: q.s.d_frame_en_off = reinterpret_cast<const int32_t *>(op); break;
            case 2: q.s.d_slot_cam = reinterpret_cast<const int32_t *>(op); break;
            case 3: q.s.d_slot_n = reinterpret_cast<const int32_t *>(op); break;
            case 4: q.s.d_head_cam = reinterpret_cast<const int32_t *>(op); break;
            case 5: q.s.d_joint_mask = reinterpret_cast<const uint32_t *>(op); break;
            case 6: q.s.d_tri_mask = reinterpret_cast<const uint32_t *>(op); break;
            case 7: q.s.d_xy = reinterpret_cast<const double *>(op); break;
            case 8: q.s.d_vp = reinterpret_cast<const float *>(op); break;
            case 9: q.s.d_en_pair = reinterpret_cast<const int32_t *>(op); break;
            case 10: q.s.n_frames = 2; break;
            case 11: q.s.n_heads = 59; break;
            case 12: q.s.n_edge_nodes = 464; break;
            default: q.s.generation += 1; break;
            }
            char what[64];
            snprintf(what, sizeof what, "key item %d differs", k);
            // (q shares b's arena and contents: only the key decides)
            expect(c.mlp3d(q, p1, n1, what), false, what);
        }
    }
    {   // a: one arena; match(A), upload B, geom_match(B), mlp3d(B, the geometric persons)
        Ctx c; Arena ar; Batch b(&ar, A, 3, 60, 480);
        c.match(b, p1, n1);
        b.upload(B, 3, 60, 480);
        c.other(b);
        expect(c.mlp3d(b, p2, n2, "a"), false, "a: match(A), upload B, geom_match(B), mlp3d(B)");
    }
    {   // b: ... gat_scores(B) + cluster(B), mlp3d(B)
        Ctx c; Arena ar; Batch b(&ar, A, 3, 60, 480);
        c.match(b, p1, n1);
        b.upload(B, 3, 60, 480);
        c.other(b);
        c.other(b);
        expect(c.mlp3d(b, p2, n2, "b"), false, "b: match(A), upload B, gat_scores(B), cluster(B), mlp3d(B)");
    }
    {   // c: no call between the upload and mlp3d; the allocator hands the persons' addresses out again
        Ctx c; Arena ar; Batch b(&ar, A, 3, 60, 480);
        c.match(b, p1, n1);
        b.upload(B, 3, 60, 480);
        expect(c.mlp3d(b, p1, n1, "c"), false, "c: match(A), upload B, mlp3d(B, persons at the old addresses)");
        // the blind spot itself, so that it stays written down: a rewrite the caller did NOT tell is taken for the old batch.
        // (not routed through Ctx::mlp3d, which would count it as the failure it is)
        c.match(b, p1, n1);
        b.rewrite_silently(C);
        ++checks;
        if (c.h.take(mpe::pair_key(b.s, p1, n1)) < 0) {
            printf("c': a silent rewrite was noticed -- by what?\n");
            ++failures;
        }
    }
    {   // d: no arena: copy in place and rebind (counts rewritten to the same values, a new generation)
        Ctx c; Arena ar; Batch b(&ar, A, 3, 60, 480);
        c.match(b, p1, n1);
        b.upload(B, 3, 60, 480);
        c.other(b);
        expect(c.mlp3d(b, p2, n2, "d"), false, "d: match(A), copy B over A + rebind, geom_match(B), mlp3d(B)");
        c.match(b, p1, n1);
        b.upload(A, 3, 60, 480);
        expect(c.mlp3d(b, p1, n1, "d'"), false, "d': rebind alone, same persons addresses");
    }
    for (int order = 0; order < 2; ++order) {   // e: two arenas, both buffers written; C and D uploaded; both orders
        Ctx c; Arena a0, a1; Batch b0(&a0, A, 3, 60, 480), b1(&a1, B, 3, 60, 480);
        c.match(b0, p1, n1);
        c.match(b1, p2, n2);
        b0.upload(C, 3, 60, 480);
        b1.upload(D, 3, 60, 480);
        Batch *first = order ? &b1 : &b0, *second = order ? &b0 : &b1;
        c.other(*first);
        expect(c.mlp3d(*first, p3, n3, "e first"), false, "e: geom_match + mlp3d in the first arena");
        c.other(*second);
        expect(c.mlp3d(*second, p3, n3, "e second"), false, "e: geom_match + mlp3d in the second arena");
        // and with the persons' addresses of the two matches handed out again
        expect(c.mlp3d(b0, p1, n1, "e old persons 0"), false, "e: arena 0 with the first match's persons addresses");
        expect(c.mlp3d(b1, p2, n2, "e old persons 1"), false, "e: arena 1 with the second match's persons addresses");
    }
    {   // f: nothing changed the data; every answer is allowed as long as it is not stale -- this design solves after any call between
        Ctx c; Arena ar; Batch b(&ar, A, 3, 60, 480);
        c.match(b, p1, n1);
        c.other(b);                                                            // geom_match(A)
        expect(c.mlp3d(b, p2, n2, "f geom"), false, "f: mlp3d(A, geometric persons)");
        expect(c.mlp3d(b, p1, n1, "f gat"), false, "f: mlp3d(A, GAT persons) after other calls");
    }
    {   // g: the control whose counts differ
        Ctx c; Arena ar; Batch b(&ar, A, 3, 60, 480);
        c.match(b, p1, n1);
        b.upload(G, 3, 59, 464);
        c.other(b);
        expect(c.mlp3d(b, p2, n2, "g"), false, "g: match(A), upload a batch of other counts, geom_match, mlp3d");
    }
    {   // h: equal totals, another per-frame layout: the key cannot tell, the calls and the generation do
        Ctx c; Arena ar; Batch b(&ar, A, 3, 60, 480);
        c.match(b, p1, n1);
        b.upload(B, 3, 60, 480);
        c.other(b);
        expect(c.mlp3d(b, p2, n2, "h"), false, "h: (25, 15, 20) heads, then (15, 25, 20) in the same arrays");
    }
    {   // i: sibling contexts keep their notes apart
        Ctx c0, c1; Arena ar; Batch b(&ar, A, 3, 60, 480);
        c0.match(b, p1, n1);
        expect(c1.mlp3d(b, p1, n1, "i sibling"), false, "i: match(A) on context 0, mlp3d(A) on context 1");
        b.upload(B, 3, 60, 480);
        expect(c1.mlp3d(b, p1, n1, "i sibling, B"), false, "i: B in A's arena on context 1");
        expect(c0.mlp3d(b, p1, n1, "i owner, B"), false, "i: and on context 0, whose note names A's generation");
        c0.match(b, p1, n1);
        c1.other(b);
        expect(c0.mlp3d(b, p1, n1, "i owner"), true, "i: another context's calls do not end this context's hand-off");
    }
    {   // the pipelines' order: window after window in two arenas, always match then mlp3d: every window fetches
        Ctx c; Arena a0, a1; Batch b0(&a0, A, 3, 60, 480), b1(&a1, B, 3, 60, 480);
        bool all = true;
        for (int w = 0; w < 8; ++w) {
            Batch &b = (w & 1) ? b1 : b0;
            b.upload(10 + w, 3, 60, 480);
            (w & 1 ? b0 : b1).upload(20 + w, 3, 60, 480);                     // the upload of the NEXT window runs ahead
            c.match(b, p1, n1);
            all = all && c.mlp3d(b, p1, n1, "pipeline");
        }
        expect(all, true, "upload, match, mlp3d per window, the next window's upload ahead: every window fetches");
    }
    if (failures) return 1;
    printf("ok %d\n", checks);
    return 0;
}
