"""Sequences for the relink tests (test_relink_host.py: harness/relink.py against answers the rule alone decides;
test_gpu_relink.py: mpe_relink_batch against the same answers and, bit for bit, against harness/relink.py).  Not a test
module.

The hand-made bodies are scaled copies of skel_cases.BODY.  A record built from identical rows has sum / cnt == l exactly
for cnt = 2 (l + l is exact), so a body that returns unchanged costs exactly 0.0; where a case needs a cost it is folded
here in Python floats (`cost_of`), from the stored coordinates, never taken from the statement."""
import math

import numpy as np

import skel_cases as sc
import track_cases as tc

J = tc.J
BONES = ((17, 0), (0, 1), (0, 2), (1, 3), (2, 4), (17, 5), (17, 6), (5, 7), (6, 8), (7, 9), (8, 10), (17, 11), (17, 12),
         (11, 12), (11, 13), (12, 14), (13, 15), (14, 16))                # harness.skeleton.BONES_18, written out
KEYS = ('ids', 'link_cost', 'link_gap', 'counters', 'status')
# the hand-made cases: two lengths make a record's bone count, a return after 2 .. 4 frames links
HAND = {'min_samples': 2, 'min_gap': 2, 'max_gap': 4, 'tid_cap': 8}
NAN = float('nan')


def body(scale=1.0, x=0.0, z=0.0):
    return sc.BODY * scale + np.array([x, 0.0, z])


def without(pose, joints):
    """the pose with NaN coordinates at `joints`: those joints are inactive in both modes"""
    p = np.array(pose, np.float64)
    p[list(joints)] = NAN
    return p


class Case:
    """rows: per frame a list of rows, each None or (id, pose [J,3]).  want: ids per frame (rows past the written ones
    -1); links: {(frame, row): (cost, gap)}; every other detection has cost -1.0 and gap 0."""

    def __init__(self, mode, rows, options, want, links, counters, status=0, pcap=4, state=None):
        self.mode, self.options, self.state_check = mode, dict(HAND, **options), state
        tri = mode == 'tri'
        B = len(rows)
        self.pcap = pcap
        self.poses = np.zeros((B, pcap, J, 3), np.float64 if tri else np.float32)
        self.flags = np.zeros((B, pcap, J) if tri else (B, pcap), np.uint8)
        self.track_ids = np.full((B, pcap), -1, np.int32)
        self.n_persons = np.array([len(r) for r in rows], np.int32)
        for f, fr in enumerate(rows):
            for p, r in enumerate(fr):
                if r is None:
                    continue
                self.track_ids[f, p] = r[0]
                self.poses[f, p] = r[1]
                self.flags[f, p] = 1
        self.want = {'ids': np.full((B, pcap), -1, np.int32), 'link_cost': np.full((B, pcap), -1.0),
                     'link_gap': np.where(self.track_ids >= 0, 0, -1).astype(np.int32),
                     'counters': np.asarray(counters, np.int64), 'status': status}
        for f, fr in enumerate(want):
            self.want['ids'][f, :len(fr)] = fr
        for (f, p), (cost, gap) in links.items():
            self.want['link_cost'][f, p], self.want['link_gap'][f, p] = cost, gap

    def arrays(self):
        return self.poses, self.flags, self.n_persons, self.track_ids


def lengths_of(stored, max_bone=1.0):
    """stored [J,3] in the pose type -> per bone the accepted length as a Python float, None where there is none"""
    x = np.asarray(stored).astype(np.float64)
    out = []
    for jp, jc in BONES:
        d = [float(x[jc, a]) - float(x[jp, a]) for a in range(3)]
        l = math.sqrt((d[0] * d[0] + d[1] * d[1]) + d[2] * d[2]) if all(math.isfinite(v) for v in d) else NAN
        out.append(l if l > 0 and l <= max_bone else None)
    return out


def cost_of(birth, record_rows, min_samples=2, max_bone=1.0):
    """step 4 in Python floats: the stored row of the birth against a record that saw the stored rows `record_rows` in
    order -> (cost, bones that count)"""
    lb = lengths_of(birth, max_bone)
    tot, n = 0.0, 0
    for b in range(len(BONES)):
        s, k = 0.0, 0
        for row in record_rows:
            l = lengths_of(row, max_bone)[b]
            if l is not None:
                s, k = s + l, k + 1
        if lb[b] is not None and k >= min_samples:
            tot, n = tot + abs(lb[b] - s / float(k)), n + 1
    return (tot / float(n) if n else math.inf), n


def stored(pose, mode):
    return np.asarray(pose, np.float64 if mode == 'tri' else np.float32)


def plain_return(mode, gap):
    """A is seen in frames 0 and 1 as id 0 and returns `gap` frames after frame 1 as id 1, empty frames between"""
    A = body()
    rows = [[(0, A)], [(0, A)]] + [[] for _ in range(gap - 1)] + [[(1, A)]]
    link = HAND['min_gap'] <= gap <= HAND['max_gap']
    want = [[0], [0]] + [[] for _ in range(gap - 1)] + [[0 if link else 1]]
    return Case(mode, rows, {}, want, {(gap + 1, 0): (0.0, gap)} if link else {}, [1 if link else 2, int(link), 0])


def cost_at_gate(mode, below):
    """the returning body is 2 % larger: with gate_m equal to the cost there is no link (strict), one ulp above there is"""
    A, A2 = body(), body(1.02, x=1.0)
    c, n = cost_of(stored(A2, mode), [stored(A, mode)] * 2)
    assert n == 18 and 0.004 < c < 0.007
    gate = math.nextafter(c, math.inf) if below else c
    rows = [[(0, A)], [(0, A)], [], [(1, A2)]]
    return Case(mode, rows, {'gate_m': gate}, [[0], [0], [], [0 if below else 1]], {(3, 0): (c, 2)} if below else {},
                [1, 1, 0] if below else [2, 0, 0])


def bone_samples(mode, enough):
    """joint 9 is NaN in one of the record's two frames: bone (7, 9) has min_samples - 1 lengths and does not count, 17
    bones do; min_bones 18 does not link, 17 does"""
    A = body()
    c, n = cost_of(stored(A, mode), [stored(A, mode), stored(without(A, [9]), mode)])
    assert n == 17 and c == 0.0
    rows = [[(0, A)], [(0, without(A, [9]))], [], [(1, A)]]
    return Case(mode, rows, {'min_bones': 17 if enough else 18}, [[0], [0], [], [0 if enough else 1]], {(3, 0): (0.0, 2)} if enough else {},
                [1, 1, 0] if enough else [2, 0, 0])


def common_bones(mode, enough):
    """the birth lacks joints 9 and 10: 16 common bones; min_bones 17 does not link, 16 does"""
    A = body()
    rows = [[(0, A)], [(0, A)], [], [(1, without(A, [9, 10]))]]
    return Case(mode, rows, {'min_bones': 16 if enough else 17}, [[0], [0], [], [0 if enough else 1]], {(3, 0): (0.0, 2)} if enough else {},
                [1, 1, 0] if enough else [2, 0, 0])


def long_bone(mode, accepted):
    """max_bone_m is the longest bone of the stored body or the float below it: in the second case two bones (the neck to
    either hip, equal by symmetry) are not accepted anywhere, 16 bones count and min_bones 17 does not link"""
    A = body()
    ls = lengths_of(stored(A, mode))
    top = max(ls)
    n_top = sum(1 for l in ls if l == top)
    assert n_top >= 1
    max_bone = top if accepted else math.nextafter(top, 0.0)
    rows = [[(0, A)], [(0, A)], [], [(1, A)]]
    return Case(mode, rows, {'max_bone_m': max_bone, 'min_bones': 19 - n_top}, [[0], [0], [], [0 if accepted else 1]],
                {(3, 0): (0.0, 2)} if accepted else {}, [1, 1, 0] if accepted else [2, 0, 0])


def two_births(mode, tie):
    """one record, two births: the lower cost wins (row 1, 1 % larger, against row 0, 2 % larger); on an exact tie (the
    same pose twice) the lower row wins"""
    A = body()
    first, second = (body(1.01, x=2.0), body(1.01, x=2.0)) if tie else (body(1.02, x=1.0), body(1.01, x=2.0))
    c0, _ = cost_of(stored(first, mode), [stored(A, mode)] * 2)
    c1, _ = cost_of(stored(second, mode), [stored(A, mode)] * 2)
    assert (c0 == c1) if tie else (c1 < c0 < 0.02)
    rows = [[(0, A)], [(0, A)], [], [(1, first), (2, second)]]
    want = [[0], [0], [], [0, 2] if tie else [1, 0]]
    return Case(mode, rows, {}, want, {(3, 0 if tie else 1): (c0 if tie else c1, 2)}, [2, 1, 0])


def two_records(mode):
    """two records of equal cost (the same pose under ids 0 and 1), one birth: the lower id wins"""
    A = body()
    rows = [[(0, A), (1, A)], [(0, A), (1, A)], [], [(2, A)]]
    return Case(mode, rows, {}, [[0, 1], [0, 1], [], [0]], {(3, 0): (0.0, 2)}, [2, 1, 0])


def continuing(mode):
    """id 0 is away for two frames and the TRACKER continues it in frame 4 (row 1): the record is present, so the birth
    with the same lengths in row 0 is no return; the next frame neither (the record was seen a frame ago)"""
    A = body()
    rows = [[(0, A)], [(0, A)], [], [], [(1, body(x=3.0)), (0, A)], [(2, body(x=6.0))]]
    return Case(mode, rows, {}, [[0], [0], [], [], [1, 0], [2]], {}, [3, 0, 0])


def chain(mode):
    """A (id 0) is lost, B (id 1, 1 % larger) is linked to it and lost, C (id 2, 0.5 % larger) returns: C gets id 0 and
    the record holds the lengths of all three"""
    A, B, C_ = body(), body(1.01, x=1.0), body(1.005, x=2.0)
    sA, sB, sC = (stored(p, mode) for p in (A, B, C_))
    cB, _ = cost_of(sB, [sA, sA])
    cC, _ = cost_of(sC, [sA, sA, sB, sB])
    assert cB < 0.02 and cC < 0.02
    rows = [[(0, A)], [(0, A)], [], [(1, B)], [(1, B)], [], [], [(2, C_)]]

    def state(st):
        assert st['canon'][:3].tolist() == [0, 0, 0] and st['last_frame'][:3].tolist() == [7, -1, -1] and st['frame'] == 8
        assert (st['cnt'][0] == 5).all() and not st['cnt'][1:].any()
        for b, l in enumerate(zip(lengths_of(sA), lengths_of(sB), lengths_of(sC))):
            assert st['sum'][0, b] == (((l[0] + l[0]) + l[1]) + l[1]) + l[2]
    return Case(mode, rows, {}, [[0], [0], [], [0], [0], [], [], [0]], {(3, 0): (cB, 2), (7, 0): (cC, 3)}, [1, 2, 0], state=state)


def position_gate(mode):
    """reach 0.5 m: the small body returns 0.25 m from where it was (inside), the large one 3 m away (outside, though its
    lengths fit); with 1.5 m per frame of gap on top of it the large one is inside as well"""
    out = {}
    S0, S1 = body(0.8), body(1.2, x=5.0)
    for name, speed in (('', 0.0), ('_speed', 1.5)):
        rows = [[(0, S0), (1, S1)], [(0, S0), (1, S1)], [], [(2, body(0.8, x=0.25)), (3, body(1.2, x=8.0))]]
        c2, _ = cost_of(stored(rows[3][0][1], mode), [stored(S0, mode)] * 2)
        c3, _ = cost_of(stored(rows[3][1][1], mode), [stored(S1, mode)] * 2)
        assert c2 < 0.02 and c3 < 0.02
        links = {(3, 0): (c2, 2)}
        if speed:
            links[(3, 1)] = (c3, 2)
        out['position_gate%s_%s' % (name, mode)] = Case(mode, rows, {'reach_m': 0.5, 'reach_per_frame_m': speed},
                                                        [[0, 1], [0, 1], [], [0, 1 if speed else 3]], links, [3 - len(links) + 1, len(links), 0])
    # the birth has the head joints only, none of them a used joint: bones (0,1) (0,2) (1,3) (2,4) fit, no joint to measure
    head = without(body(), [j for j in range(J) if j not in (0, 1, 2, 3, 4)])
    for name, used, link in (('no_common', sum(1 << j for j in tc.USED) & ~1, False), ('common', sum(1 << j for j in tc.USED), True)):
        rows = [[(0, body())], [(0, body())], [], [(1, head)]]
        out['position_%s_%s' % (name, mode)] = Case(mode, rows, {'reach_m': 0.5, 'min_bones': 4, 'used_joint_mask': used},
                                                    [[0], [0], [], [0 if link else 1]], {(3, 0): (0.0, 2)} if link else {},
                                                    [1, 1, 0] if link else [2, 0, 0])
    return out


def non_finite(mode):
    """a row of NaNs (id 0) is a birth that founds a record nothing can link to: A (id 1) two frames later is a birth, and
    when A returns as id 2 it takes id 1"""
    A = body()
    rows = [[(0, np.full((J, 3), NAN))], [], [(1, A)], [(1, A)], [], [(2, A), (3, np.full((J, 3), NAN))]]

    def state(st):
        assert st['last_frame'][:4].tolist() == [0, 5, -1, 5] and not st['cnt'][0].any() and not st['cnt'][3].any()
        assert (st['cnt'][1] == 3).all() and st['canon'][:4].tolist() == [0, 1, 1, 3]
    return Case(mode, rows, {}, [[0], [], [1], [1], [], [1, 3]], {(5, 0): (0.0, 2)}, [3, 1, 0], state=state)


def over_cap(mode):
    """tid_cap 8: ids 8 and 9 pass through, are counted and set the status, and found no record; a row that repeats an id
    gets the same id; id 7 is the last with a record"""
    A = body()
    rows = [[(8, A), (7, A), (7, body(x=1.0))], [(8, A), (7, A)], [], [(9, A), (6, A), (6, A), None]]
    return Case(mode, rows, {}, [[8, 7, 7], [8, 7], [], [9, 7, 7, -1]], {(3, 1): (0.0, 2)}, [1, 1, 3], status=1)


def one_row(mode):
    """pcap 1, an empty frame in the middle of the record's frames"""
    A = body()
    rows = [[(0, A)], [], [(0, A)], [], [], [(1, A)]]
    return Case(mode, rows, {}, [[0], [], [0], [], [], [0]], {(5, 0): (0.0, 3)}, [1, 1, 0], pcap=1)


def hand_made():
    cases = {}
    for mode in ('mlp', 'tri'):
        for gap in (HAND['min_gap'] - 1, HAND['min_gap'], HAND['max_gap'], HAND['max_gap'] + 1):
            cases['plain_return_%d_%s' % (gap, mode)] = plain_return(mode, gap)
        for make in (cost_at_gate, bone_samples, common_bones, long_bone, two_births):
            for flag in (False, True):
                cases['%s_%d_%s' % (make.__name__, flag, mode)] = make(mode, flag)
        for make in (two_records, continuing, chain, non_finite, over_cap, one_row):
            cases['%s_%s' % (make.__name__, mode)] = make(mode)
        cases.update(position_gate(mode))
    return cases


def run_statement(R, c, chunks=None):
    """a case through harness/relink.py, in one call or in chunks -> (the outputs joined, the last state)"""
    return statement(R, c.arrays(), c.mode, c.options, chunks)


def statement(R, arrays, mode, options, chunks=None):
    poses, flags, n_persons, ids = arrays
    chunks = [len(poses)] if chunks is None else chunks
    outs, st, at = [], None, 0
    for n in chunks:
        o, st = R.relink_sequence(poses[at:at + n], flags[at:at + n], n_persons[at:at + n], ids[at:at + n], mode, BONES, options, st)
        outs.append(o)
        at += n
    assert at == len(poses)
    out = {k: np.concatenate([o[k] for o in outs]) for k in ('ids', 'link_cost', 'link_gap')}
    out['counters'], out['status'] = outs[-1]['counters'], outs[-1]['status']
    return out, st


# ---- sequences with noise: bodies of different scale that leave for longer than the tracker waits ----

TRACK_GATE, TRACK_GAP = 0.5, 2


def walkers(seed, tri, B, pcap, scales, away, sigma, start=None, jump=1.5, drop=0.0):
    """B frames of len(scales) bodies of those scales on random walks of 2 cm per frame, `sigma` metres of seeded Gaussian
    noise on every coordinate, rows permuted per frame.  away: {body: [(first, last)]} frames in which nobody sees it; it
    comes back `jump` metres along x from where it left.  drop (mode 'tri'): share of joints missing.  The tracker's
    statement gives the ids.  -> (poses, flags, n_persons, track ids, who [B,pcap]: the body in each row, -1 none)"""
    T = pkg_tracking()
    rng = np.random.default_rng(seed)
    dt = np.float64 if tri else np.float32
    n = len(scales)
    pos = np.stack([3.0 * np.arange(n), np.zeros(n), 3.0 * (np.arange(n) % 2)], axis=1) if start is None else np.array(start, np.float64)
    poses = np.zeros((B, pcap, J, 3), dt)
    flags = np.zeros((B, pcap, J) if tri else (B, pcap), np.uint8)
    n_persons = np.zeros(B, np.int32)
    who = np.full((B, pcap), -1, np.int32)
    gone = lambda k, f: any(a <= f <= b for a, b in away.get(k, ()))
    for f in range(B):
        step = rng.normal(size=(n, 3)) * np.array([1.0, 0.0, 1.0])
        pos = pos + 0.02 * step / np.linalg.norm(step, axis=1, keepdims=True)
        for k in range(n):
            if any(b + 1 == f for _, b in away.get(k, ())):
                pos[k, 0] += jump
        seen = [k for k in range(n) if not gone(k, f)]
        seen = [seen[i] for i in rng.permutation(len(seen))]
        n_persons[f] = len(seen)
        for p, k in enumerate(seen):
            poses[f, p] = (sc.BODY * scales[k] + pos[k] + rng.normal(0.0, sigma, (J, 3))).astype(dt)
            flags[f, p] = (rng.random(J) >= drop) if tri else 1
            who[f, p] = k
    mode = 'tri' if tri else 'mlp'
    ids = T.track_sequence(poses, flags, n_persons, mode, tc.USED, TRACK_GATE, TRACK_GAP)['ids']
    return poses, flags, n_persons, ids, who


def pkg_tracking():
    from conftest import pkg
    return pkg('harness.tracking')


CHUNKS = tc.CHUNKS + (3,)                                   # track_cases.CHUNKS hold 37 frames; the sequences here have 40
RANDOM_OPTIONS = {'min_samples': 3, 'min_gap': TRACK_GAP + 2, 'max_gap': 30, 'tid_cap': 32}
# departures across every border of track_cases.CHUNKS (frames 1, 2, 7, 23), each longer than the tracker's gap
RANDOM_AWAY = {0: [(5, 12)], 1: [(1, 6), (20, 27)], 2: [(14, 18), (30, 33)], 3: [(22, 36)]}


def random_sequence(seed, tri):
    """40 frames, pcap 6, three to five bodies (by seed) whose scales differ by 8 % or more, 2 mm of noise"""
    n = 3 + seed % 3
    scales = [0.84, 0.92, 1.0, 1.08, 1.16][:n]
    away = {k: v for k, v in RANDOM_AWAY.items() if k < n}
    return walkers(seed, tri, 40, 6, scales, away, 0.002, drop=0.05)[:4]


WIDE_OPTIONS = {'min_samples': 4, 'min_gap': 2, 'max_gap': 8, 'tid_cap': 160}


def wide_sequence(seed, tri, n=80):
    """n tracks alive in 4 frames, two empty frames, then 4 frames in which they are back, shuffled, under new ids: the
    record scan and the reductions run over more than one wave, and the greedy takes n links in one frame.  Scales 0.5 %
    apart, so every birth has a dozen linkable records and the least cost decides; the last body is the first one again,
    pose for pose (a deliberate tie).  Ids as a tracker with no memory of the gap gives them."""
    rng = np.random.default_rng(seed)
    dt = np.float64 if tri else np.float32
    pcap = n
    poses = np.zeros((10, pcap, J, 3), dt)
    flags = np.zeros((10, pcap, J) if tri else (10, pcap), np.uint8)
    ids = np.full((10, pcap), -1, np.int32)
    n_persons = np.zeros(10, np.int32)
    base = np.stack([0.6 * (np.arange(n) % 10), np.zeros(n), 0.6 * (np.arange(n) // 10)], axis=1)
    order = rng.permutation(n)
    for f in (0, 1, 2, 3, 6, 7, 8, 9):
        late = f >= 6
        for p in range(n):
            k = order[p] if late else p
            src = 0 if k == n - 1 else k
            poses[f, p] = (sc.BODY * (0.7 + 0.005 * src) + base[src] + (np.array([0.3, 0.0, 0.0]) if late else 0.0)).astype(dt)
            ids[f, p] = n + p if late else p
        flags[f] = 1
        n_persons[f] = n
    return poses, flags, n_persons, ids


# ---- the behavioural case ----

BEHAVE_SCALES = (0.8, 1.0, 1.2)                              # statures 1.33, 1.66 and 1.99 m
BEHAVE_SIGMA = 0.003
BEHAVE_SEED = 7
BEHAVE_FRAMES = 120
# each body in turn away for longer than the tracker's gap, and the absences overlap, so that a body which returns finds the
# record of another body that is still away (a wrong candidate); body 1 leaves a second time 6 frames after it came back, so
# the fragment the tracker makes of those 6 frames is too short for a length table of 10 samples
BEHAVE_AWAY = {0: [(20, 36), (90, 104)], 1: [(28, 44), (51, 66)], 2: [(60, 78), (96, 110)]}
BEHAVE_OPTIONS = {'min_gap': TRACK_GAP + 2, 'tid_cap': 16}


def behaviour(tri=True):
    return walkers(BEHAVE_SEED, tri, BEHAVE_FRAMES, 4, BEHAVE_SCALES, BEHAVE_AWAY, BEHAVE_SIGMA)


def same(got, want, keys=KEYS, what=''):
    sc.same(got, want, keys, what)
