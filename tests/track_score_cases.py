"""Sequences for the track score (include/mpe.h: mpe_track_score_batch; harness/track_score.py): hand-made ones whose
answers the rule alone decides, written out by hand below, and a random generator.  Shared by the CPU test of the numpy
statement and the GPU test of the kernels.  All use pcap = gcap <= 6 and <= 40 frames.

A frame is described as (gt, det[, skip]): gt = [(identity, valid)] per GT row; det = one tuple per pose ROW p,
(track id, assigned GT row, error in mm, invalid, person flag).  With joint_flags == 0 only rows with a person flag are
detections, and assign / err / invalid are indexed by DETECTION (the r-th flagged row), as mpe_eval_batch writes them."""
import numpy as np

ARRAYS = ('flags', 'n_persons', 'track_ids', 'assign', 'err', 'invalid', 'n_res', 'n_gt', 'gt_ids', 'gt_valid')


class Case:
    def __init__(self, frames, expect, joint_flags=0, threshold_mm=150., gid_cap=16, tid_cap=64, cap=4, J=3,
                 frame_counts=None, match_tid=None, use_skip=False):
        B = len(frames)
        self.joint_flags, self.threshold_mm, self.gid_cap, self.tid_cap, self.cap, self.J = joint_flags, threshold_mm, gid_cap, tid_cap, cap, J
        self.expect, self.frame_counts, self.match_tid = expect, frame_counts, match_tid
        self.flags = np.zeros((B, cap, J) if joint_flags else (B, cap), np.uint8)
        self.n_persons, self.n_res, self.n_gt = np.zeros(B, np.int32), np.zeros(B, np.int32), np.zeros(B, np.int32)
        self.track_ids = np.full((B, cap), -1, np.int32)
        self.assign, self.err = np.full((B, cap), -1, np.int32), np.zeros((B, cap), np.float64)
        self.invalid = np.zeros((B, cap), np.uint8)
        self.gt_ids, self.gt_valid = np.full((B, cap), -1, np.int32), np.zeros((B, cap), np.uint8)
        self.skip = np.zeros(B, np.uint8) if use_skip else None
        for f, fr in enumerate(frames):
            gt, det = fr[0], fr[1]
            if len(fr) > 2 and fr[2]:
                self.skip[f] = 1
            self.n_gt[f] = len(gt)
            for g, (o, valid) in enumerate(gt):
                self.gt_ids[f, g], self.gt_valid[f, g] = o, valid
            self.n_persons[f] = len(det)
            r = 0
            for p, (h, g, e_mm, inv, flag) in enumerate(det):
                self.track_ids[f, p] = h
                self.flags[f, p] = flag
                if flag or joint_flags:
                    self.assign[f, r], self.invalid[f, r] = g, inv
                    self.err[f, r] = e_mm if isinstance(e_mm, np.float64) else np.float64(e_mm) / 1000.     # np.float64: metres, as given
                    r += 1
            self.n_res[f] = r

    def arrays(self, lo=0, hi=None):
        return {k: getattr(self, k)[lo:hi] for k in ARRAYS}


def D(h, g, e_mm=20., inv=0, flag=1):
    return (h, g, e_mm, inv, flag)


def hand_made():
    c = {}
    two = [(0, 1), (1, 1)]
    c['perfect'] = Case([(two, [D(10, 0), D(11, 1, 30.)])] * 5,
                        dict(frames=5, n_gt=10, n_pred=10, tp=10, fp=0, fn=0, idsw=0, frag=0, ignored=0, over_ids=0, idtp=10, n_ids=2,
                             n_tracks=2, mt=2, pt=0, ml=0, mota=1.0, idf1=1.0, idp=1.0, idr=1.0, status=0))
    # tracks 10 and 11 exchange identities at frame 3: each identity sees one switch; table = [[3, 3], [3, 3]] -> IDTP 6
    c['exchange'] = Case([(two, [D(10, 0), D(11, 1)])] * 3 + [(two, [D(11, 0), D(10, 1)])] * 3,
                         dict(frames=6, tp=12, fp=0, fn=0, idsw=2, frag=0, idtp=6, n_ids=2, n_tracks=2, mota=1.0 - 2.0 / 12.0, idf1=0.5),
                         frame_counts={3: (2, 0, 0, 2), 2: (2, 0, 0, 0), 4: (2, 0, 0, 0)})
    # the GT rows change places from frame to frame, the ids follow the person: nothing switches
    c['rows_permuted'] = Case([(two, [D(10, 0), D(11, 1)]), ([(1, 1), (0, 1)], [D(10, 1), D(11, 0)])] * 3,
                              dict(frames=6, tp=12, idsw=0, frag=0, idtp=12, mota=1.0, idf1=1.0),
                              match_tid={1: (11, 10, -2, -2), 2: (10, 11, -2, -2)})
    one = [(0, 1)]
    c['miss_same_track'] = Case([(one, [D(10, 0)]), (one, []), (one, [D(10, 0)])],
                                dict(frames=3, n_gt=3, tp=2, fn=1, fp=0, idsw=0, frag=1, idtp=2, mt=0, pt=1, ml=0, mota=1.0 - 1.0 / 3.0),
                                match_tid={1: (-1, -2, -2, -2)})
    c['miss_other_track'] = Case([(one, [D(10, 0)]), (one, []), (one, [D(12, 0)])],
                                 dict(frames=3, tp=2, fn=1, idsw=1, frag=1, idtp=1, n_tracks=2), frame_counts={2: (1, 0, 0, 1)})
    c['absent_other_track'] = Case([(one, [D(10, 0)]), ([], []), ([], []), ([], []), (one, [D(12, 0)])],
                                   dict(frames=5, n_gt=2, tp=2, fn=0, idsw=1, frag=0, idtp=1, mt=1, mota=0.5))
    # an invalid GT body and a detection assigned to it: neither counts; track 11 is never seen
    c['ignore_row'] = Case([([(0, 1), (1, 0)], [D(10, 0), D(11, 1)])],
                           dict(frames=1, n_gt=1, n_pred=1, tp=1, fp=0, fn=0, ignored=1, n_tracks=1, n_ids=1, idtp=1, mota=1.0, idf1=1.0),
                           match_tid={0: (10, -2, -2, -2)})
    # a GT row without an identity is an ignore row as well
    c['ignore_no_identity'] = Case([([(0, 1), (-1, 1)], [D(10, 0), D(11, 1)])], dict(n_gt=1, n_pred=1, tp=1, ignored=1, n_tracks=1))
    # person flags: rows 0 and 1 are no detections (their ids are junk), so detection 0 is row 2 and detection 1 is row 3
    c['flag_rows_in_front'] = Case([(two, [D(33, 0, flag=0), D(34, 1, flag=0), D(10, 0), D(11, 1)])] * 2,
                                   dict(frames=2, n_pred=4, tp=4, fp=0, fn=0, idsw=0, idtp=4, n_tracks=2),
                                   match_tid={0: (10, 11, -2, -2)})
    # e * 1000. == threshold_mm exactly (0.125 * 1000. is exact) is no match; the next float64 below is one
    below = np.nextafter(np.float64(0.125), 0.0)
    assert np.float64(0.125) * 1000. == 125. and below * 1000. < 125.
    c['threshold_edge'] = Case([(one, [D(10, 0, np.float64(0.125))]), (one, [D(10, 0, below)])],
                               dict(frames=2, tp=1, fp=1, fn=1, idsw=0, frag=0, err_sum=float(below), mota=0.0), threshold_mm=125.,
                               frame_counts={0: (0, 1, 1, 0), 1: (1, 0, 0, 0)})
    c['no_track_id'] = Case([(one, [D(-1, 0)])], dict(tp=0, fp=1, fn=1, n_pred=1, n_tracks=0, idtp=0, ml=1, mota=-1.0))
    c['invalid_detection'] = Case([(one, [D(10, 0, inv=1)])], dict(tp=0, fp=1, fn=1, n_pred=1, n_tracks=1, idtp=0), joint_flags=1)
    # the skipped frames hold a detection that would switch the identity: they must change nothing
    c['skipped_between'] = Case([(one, [D(10, 0)]), (one, [D(12, 0)], 1), (one, [], 1), (one, [D(10, 0)])],
                                dict(frames=2, n_gt=2, tp=2, fp=0, fn=0, idsw=0, frag=0, idtp=2, n_tracks=1, mota=1.0), use_skip=True,
                                frame_counts={1: (0, 0, 0, 0), 2: (0, 0, 0, 0)}, match_tid={1: (-2, -2, -2, -2)})
    # identity 8 at gid_cap = 8 and track 16 at tid_cap = 16: frame 0 leaves out both records and track 16's count
    c['over_ids'] = Case([([(8, 1), (0, 1)], [D(10, 0), D(16, 1)]), (one, [D(10, 0)])],
                         dict(frames=2, n_gt=3, n_pred=3, tp=3, fp=0, fn=0, over_ids=3, status=1, n_ids=1, n_tracks=1, idtp=1, idsw=0),
                         gid_cap=8, tid_cap=16, match_tid={0: (10, 16, -2, -2)})
    # an empty frame, a frame with false positives only, a frame with an unassigned detection and a miss
    c['empty_and_fp_only'] = Case([([], []), ([], [D(10, -1), D(11, -1)]), (one, [D(10, -1)])],
                                  dict(frames=3, n_gt=1, n_pred=3, tp=0, fp=3, fn=1, idsw=0, idtp=0, n_tracks=2, mota=-3.0),
                                  frame_counts={0: (0, 0, 0, 0), 1: (0, 2, 0, 0), 2: (0, 1, 1, 0)})
    return c


def random_sequence(seed, joint_flags, B=40, cap=6, tid_cap=4096, gid_cap=16, J=3):
    """Births, deaths, gaps, GT rows permuted per frame, ignore rows (invalid or without identity), -1 track ids, track ids
    in the thousands (a few at or over tid_cap, an identity at gid_cap, now and then one identity on two rows), errors
    around the threshold, invalid marks, skipped frames, rows without a person flag."""
    rng = np.random.RandomState(seed)
    c = Case([([], [])] * B, {}, joint_flags=joint_flags, gid_cap=gid_cap, tid_cap=tid_cap, cap=cap, J=J, use_skip=True)
    people = list(range(gid_cap - 3, gid_cap + 1)) + [2, 5]               # identities; the last of the first four is gid_cap itself
    track_of = {o: 1000 + 517 * k for k, o in enumerate(people)}          # 1000 .. 3585
    alive = {o: rng.rand() < 0.7 for o in people}
    for f in range(B):
        c.skip[f] = rng.rand() < 0.1
        for o in people:
            if rng.rand() < 0.15:
                alive[o] = not alive[o]
            if rng.rand() < 0.1:
                track_of[o] = int(rng.choice([1000 + rng.randint(3200), tid_cap, tid_cap + 7], p=[0.8, 0.1, 0.1]))
        here = [o for o in people if alive[o]][:cap]
        rng.shuffle(here)
        if len(here) >= 2 and rng.rand() < 0.1:
            here[1] = here[0]
        c.n_gt[f] = len(here)
        for g, o in enumerate(here):
            c.gt_ids[f, g] = -1 if rng.rand() < 0.1 else o
            c.gt_valid[f, g] = rng.rand() < 0.85
        rows = []                                                          # (track id, GT row or -1) per pose row
        for g, o in enumerate(here):
            if rng.rand() < 0.8:
                rows.append((-1 if rng.rand() < 0.1 else track_of[o], g))
        while len(rows) < cap and rng.rand() < 0.3:
            rows.append((1000 + rng.randint(3000), int(rng.choice([-1, cap - 1]))))
        rows = rows[:cap]
        rng.shuffle(rows)
        c.n_persons[f] = len(rows)
        r = 0
        for p, (h, g) in enumerate(rows):
            c.track_ids[f, p] = h
            on = True if joint_flags else rng.rand() < 0.85
            c.flags[f, p] = 1 if on else 0
            if on:
                c.assign[f, r], c.err[f, r], c.invalid[f, r] = g, rng.rand() * 0.2, rng.rand() < 0.05
                r += 1
        c.n_res[f] = r if rng.rand() < 0.9 else max(0, r - 1)
    return c


def in_chunks(step, case, chunks):
    """step(arrays, skip) per chunk; -> the outputs concatenated along the frames."""
    B, lo, outs = len(case.n_gt), 0, []
    sizes = list(chunks)
    sizes.append(B - sum(sizes))
    for n in sizes:
        if n <= 0:
            continue
        outs.append(step(case.arrays(lo, lo + n), None if case.skip is None else case.skip[lo:lo + n]))
        lo += n
    assert lo == B
    return {k: np.concatenate([o[k] for o in outs]) for k in ('frame_counts', 'match_tid')}


def check(result, per_frame, case, what=''):
    """The hand-made answers: every expected total and ratio, the listed frames' counts and match_tid rows."""
    for k, v in case.expect.items():
        if isinstance(v, float):
            assert result[k] == v, (what, k, result[k], v)
        else:
            assert int(result[k]) == v, (what, k, result[k], v)
    for f, v in (case.frame_counts or {}).items():
        assert tuple(int(x) for x in per_frame['frame_counts'][f]) == v, (what, f, per_frame['frame_counts'][f], v)
    for f, v in (case.match_tid or {}).items():
        assert tuple(int(x) for x in per_frame['match_tid'][f]) == v, (what, f, per_frame['match_tid'][f], v)
    assert result['tp'] + result['fn'] == result['n_gt'] and result['tp'] + result['fp'] == result['n_pred']
    assert result['idtp'] <= result['tp']


def same(got_frames, got_result, got_state, ref_frames, ref_result, ref_state, what=''):
    """Equality on every integer output, bit equality on err_sum and the ratios (NaN equals NaN)."""
    for k in ('frame_counts', 'match_tid'):
        assert np.array_equal(got_frames[k], ref_frames[k]), (what, k, np.argwhere(got_frames[k] != ref_frames[k])[:4])
    for k in ref_result:
        a, b = got_result[k], ref_result[k]
        if isinstance(b, float):
            assert np.float64(a).tobytes() == np.float64(b).tobytes() or (a != a and b != b), (what, k, a, b)
        else:
            assert int(a) == int(b), (what, k, a, b)
    for k in ref_state:
        assert np.array_equal(got_state[k], ref_state[k]), (what, k)
