"""Sequences for the smoothing tests (test_smooth_host.py: harness/smoothing.py against answers the rule alone decides;
test_gpu_smooth.py: mpe_smooth_batch against the same answers and, bit for bit, against harness/smoothing.py).  Not a
test module.

The known answers rest on exact arithmetic: every coordinate is x0 + v * f with x0 and v multiples of 2^-6 on top of
track_cases.SHAPE (multiples of 2^-4), the decay is 1 or 0.5 and the window at most 15, so every weight, every
y_a = x_a - x_r = -v * (a - r) and every product in the sums and in the fit is a dyadic number of fewer than 53 bits.
Then S2*T0 - S1*T1 = v * r * D and S0*T1 - S1*T0 = -v * D exactly: alpha is the true position now, beta is -v."""
import numpy as np

import track_cases as tc

J = tc.J
ALL = (1 << J) - 1
NOISE_SIGMA = 0.01
NOISE_SEED = 11
# the end point of a 7-point line fit has variance 2(2n-1)/(n(n+1)) sigma^2 = 0.464 sigma^2 (n = 7): an RMS of 0.68 sigma
NOISE_BOUND = 0.85 * NOISE_SIGMA


def at(x0, v, f):
    return tc.SHAPE + np.asarray(x0, float) + np.asarray(v, float) * f


class Case:
    """frames: per frame a list of rows, each None or (id, pose [J,3]) or (id, pose, joints present) in mode 'tri'.
    expect: [(frame, row, joints, pose or None (= the input bits), vel [3], flag, n_samples)]."""

    def __init__(self, mode, frames, window, decay, fill, expect, pcap=4, n_persons=None):
        self.mode, self.window, self.decay, self.fill, self.expect = mode, window, decay, fill, expect
        seq = tc.Seq(mode, [[None if r is None else (r[1], r[2] if len(r) > 2 else range(J)) for r in fr] for fr in frames], pcap)
        self.poses, self.flags = seq.poses, seq.flags
        self.n_persons = seq.n_persons if n_persons is None else np.asarray(n_persons, np.int32)
        self.ids = np.full((len(frames), pcap), -1, np.int32)
        for f, fr in enumerate(frames):
            for p, r in enumerate(fr):
                if r is not None:
                    self.ids[f, p] = r[0]


def check(out, case):
    """the outputs of one run over the whole case against its expect list, and what holds for every case"""
    dt = case.poses.dtype
    assert out['poses'].dtype == dt and out['poses'].shape == case.poses.shape
    assert out['flags'].dtype == np.uint8 and out['flags'].shape == case.flags.shape
    assert out['vel'].dtype == np.float64 and out['vel'].shape == case.poses.shape
    assert out['n_samples'].dtype == np.uint8 and out['n_samples'].shape == case.poses.shape[:3]
    no = case.ids < 0                                        # rows that are no detection: copied through
    assert out['poses'][no].tobytes() == case.poses[no].tobytes() and not out['vel'][no].any() and not out['n_samples'][no].any()
    assert out['flags'][no].tobytes() == case.flags[no].tobytes()
    for f, p, joints, pose, vel, flag, n in case.expect:
        for j in joints:
            what = (f, p, j)
            want = case.poses[f, p, j] if pose is None else np.asarray(pose[j], dt)
            assert out['poses'][f, p, j].tobytes() == want.tobytes(), (what, out['poses'][f, p, j], want)
            assert (out['vel'][f, p, j] == np.asarray(vel, float)).all(), (what, out['vel'][f, p, j], vel)
            got_flag = out['flags'][f, p, j] if case.mode == 'tri' else out['flags'][f, p]
            assert got_flag == flag and out['n_samples'][f, p, j] == n, (what, got_flag, flag, out['n_samples'][f, p, j], n)


def linear(mode, window, decay, B=20):
    """id 7 walks, id 3 stands; the first frame of a track is a copy, every later one the exact line"""
    x0, v = (0.5, -0.25, 1.0), (0.046875, -0.015625, 0.03125)
    y0 = (-1.0, 0.25, 0.0)
    frames = [[(7, at(x0, v, f), range(J)), (3, at(y0, 0, f), range(J))] for f in range(B)]
    expect = []
    for f in range(B):
        n = min(f, window) + 1
        expect.append((f, 0, range(J), None, v if n >= 2 else (0, 0, 0), 1, n))
        expect.append((f, 1, range(J), None, (0, 0, 0), 1, n))
    return Case(mode, frames, window, decay, False, expect)


def row_swap(mode):
    """two people on different lines whose rows swap every frame: a filter that followed rows would see a zigzag"""
    a = lambda f: at((0.0, 0.0, 0.0), (0.03125, 0.0, 0.015625), f)
    b = lambda f: at((2.0, 0.5, -1.0), (-0.046875, 0.015625, 0.0), f)
    frames = [[(40, a(f), range(J)), (41, b(f), range(J))] if f % 2 == 0 else [(41, b(f), range(J)), (40, a(f), range(J))]
              for f in range(10)]
    expect = []
    for f in range(1, 10):
        ra, rb = (0, 1) if f % 2 == 0 else (1, 0)
        expect.append((f, ra, range(J), None, (0.03125, 0.0, 0.015625), 1, min(f, 6) + 1))
        expect.append((f, rb, range(J), None, (-0.046875, 0.015625, 0.0), 1, min(f, 6) + 1))
    return Case(mode, frames, 6, 0.5, False, expect)


def fill(on, decay=1.0):
    """mode 'tri', window 6.  Row 0: joint 5 absent in frames 5 and 6 (its stored coordinates are 99 there).  Row 1: joint
    9 seen in frames 0 and 8 only: one sample in the window, never filled."""
    x0, v = (0.25, 0.0, -0.5), (0.015625, 0.03125, -0.015625)
    others = [j for j in range(J) if j != 5]
    frames = []
    for f in range(11):
        pa = at(x0, v, f)
        if f in (5, 6):
            pa[5] = 99.0
        frames.append([(1000, pa, others if f in (5, 6) else range(J)),
                       (2000, at((3.0, 0.0, 0.0), 0, f), range(J) if f in (0, 8) else [j for j in range(J) if j != 9])])
    truth = lambda f: at(x0, v, f)
    expect = [(4, 0, [5], None, v, 1, 5), (7, 0, [5], None, v, 1, 5), (8, 0, [5], None, v, 1, 5), (10, 0, [5], None, v, 1, 5),
              (10, 0, [4], None, v, 1, 7)]
    for f in (5, 6):
        expect.append((f, 0, [5], truth(f), v, 2, 5) if on else (f, 0, [5], None, (0, 0, 0), 0, 5))
        expect.append((f, 0, [4], None, v, 1, f + 1))
    expect += [(1, 1, [9], None, (0, 0, 0), 0, 1), (6, 1, [9], None, (0, 0, 0), 0, 1), (7, 1, [9], None, (0, 0, 0), 0, 0),
               (8, 1, [9], None, (0, 0, 0), 1, 1), (9, 1, [9], None, (0, 0, 0), 0, 1), (9, 1, [8], None, (0, 0, 0), 1, 7)]
    return Case('tri', frames, 6, decay, on, expect)


def gaps(mode):
    """window 4.  A (row order varies): seen in 0-3 and from 7 on, 3 = W - 1 frames away: frame 7 has the samples of ages
    0 and 4.  B: seen in 0-1 and from 8 on, 6 > W frames away: frame 8 starts afresh.  C: always seen but in frame 5,
    which has n_persons = 0 and still counts: frame 6 has ages 0, 2, 3, 4 and the exact velocity only if it does."""
    va, vb, vc = (0.03125, 0.0, 0.0), (0.0, 0.015625, 0.0), (0.0, 0.0, -0.046875)
    A = lambda f: (5, at((0.0, 0.0, 0.0), va, f), range(J))
    Bp = lambda f: (6, at((1.0, 0.0, 0.0), vb, f), range(J))
    Cp = lambda f: (9, at((2.0, 0.0, 0.0), vc, f), range(J))
    frames = []
    for f in range(10):
        if f == 5:
            frames.append([])
            continue
        rows = [Cp(f)]
        if f <= 3 or f >= 7:
            rows.insert(0, A(f))
        if f <= 1 or f >= 8:
            rows.append(Bp(f))
        frames.append(rows)
    expect = [(3, 0, range(J), None, va, 1, 4), (7, 0, range(J), None, va, 1, 2), (8, 0, range(J), None, va, 1, 2),
              (9, 0, range(J), None, va, 1, 3),
              (1, 2, range(J), None, vb, 1, 2), (8, 2, range(J), None, (0, 0, 0), 1, 1), (9, 2, range(J), None, vb, 1, 2),
              (4, 0, range(J), None, vc, 1, 5), (6, 0, range(J), None, vc, 1, 4), (7, 1, range(J), None, vc, 1, 4)]
    return Case(mode, frames, 4, 0.5, False, expect)


def non_finite(mode):
    """window 6, decay 1: a NaN in frame 3, joint 2, y.  Frame 3 copies that joint through (its older samples still
    count in n_samples); every later frame drops that one sample only."""
    x0, v = (0.0, 0.5, 0.0), (0.015625, 0.015625, 0.0)
    frames = []
    for f in range(8):
        p = at(x0, v, f)
        if f == 3:
            p[2, 1] = np.nan
        frames.append([(12, p, range(J))])
    expect = [(3, 0, [2], None, (0, 0, 0), 1, 3), (3, 0, [1, 3], None, v, 1, 4), (4, 0, [2], None, v, 1, 4), (4, 0, [3], None, v, 1, 5),
              (7, 0, [2], None, v, 1, 6), (7, 0, [3], None, v, 1, 7)]
    return Case(mode, frames, 6, 1.0, False, expect)


def hand_made():
    cases = {}
    for mode in ('mlp', 'tri'):
        for window in (2, 6, 15):
            for decay in (1.0, 0.5):
                cases['linear_%s_w%d_%s' % (mode, window, decay)] = linear(mode, window, decay)
        cases['row_swap_' + mode] = row_swap(mode)
        cases['gaps_' + mode] = gaps(mode)
        cases['non_finite_' + mode] = non_finite(mode)
    cases['fill_on'] = fill(True)
    cases['fill_on_decay_0.5'] = fill(True, 0.5)
    cases['fill_off'] = fill(False)
    return cases


def noise(mode, B=40, persons=4):
    """a constant truth plus seeded Gaussian noise of NOISE_SIGMA, rows rotating with the frame -> (truth [B,P,J,3] by
    row, poses, flags, n_persons, ids)"""
    rng = np.random.default_rng(NOISE_SEED)
    tri = mode == 'tri'
    base = np.stack([tc.person(1.5 * k, 0.0, 0.5 * k) for k in range(persons)])
    poses = np.zeros((B, persons, J, 3), np.float64 if tri else np.float32)
    truth = np.zeros((B, persons, J, 3))
    ids = np.zeros((B, persons), np.int32)
    for f in range(B):
        who = (np.arange(persons) + f) % persons
        truth[f] = base[who]
        poses[f] = (base[who] + rng.normal(0.0, NOISE_SIGMA, (persons, J, 3))).astype(poses.dtype)
        ids[f] = 100 + who
    flags = np.ones((B, persons, J) if tri else (B, persons), np.uint8)
    return truth, poses, flags, np.full(B, persons, np.int32), ids


def noise_rms(out_poses, truth, first=6):
    d = np.asarray(out_poses, np.float64)[first:] - truth[first:]
    assert d.size > 7000
    return float(np.sqrt((d * d).mean()))


def spread_ids(ids):
    """the tracker's consecutive ids as ids up to the thousands (the smoother only compares them)"""
    return np.where(ids >= 0, 5 + 211 * ids, -1).astype(np.int32)


def random_sequence(seed, tri, tracking, B=40, pcap=6, away=None):
    """track_cases.random_sequence with the ids of the numpy tracker (births, deaths, gaps, duplicated poses, rows without
    a flag, empty frames; mode 'tri': missing joints), a few coordinates made NaN or infinite -> poses, flags, n_persons, ids"""
    poses, flags, n_persons = tc.random_sequence(seed, tri, B=B, pcap=pcap, away=away)
    ids = spread_ids(tracking.track_sequence(poses, flags, n_persons, 'tri' if tri else 'mlp', tc.USED, 0.5, 3)['ids'])
    rng = np.random.default_rng(seed + 1000)
    for _ in range(B // 2):
        poses[rng.integers(B), rng.integers(pcap), rng.integers(J), rng.integers(3)] = (np.nan, np.inf, -np.inf)[rng.integers(3)]
    return poses, flags, n_persons, ids


def in_chunks(run, arrays, chunks):
    """run(*arrays cut to the chunk) per chunk, in order -> the outputs of the chunks joined."""
    outs, at_ = [], 0
    for n in chunks:
        outs.append(run(*(a[at_:at_ + n] for a in arrays)))
        at_ += n
    assert at_ == len(arrays[0])
    return {k: np.concatenate([o[k] for o in outs]) for k in ('poses', 'flags', 'vel', 'n_samples')}


def same(got, want, what=''):
    for k in ('poses', 'flags', 'vel', 'n_samples'):
        g, w = np.asarray(got[k]), np.asarray(want[k])
        assert g.dtype == w.dtype and g.shape == w.shape, (what, k)
        if g.tobytes() != w.tobytes():
            gb = np.ascontiguousarray(g).reshape(-1).view(np.uint8).reshape(g.size, -1)
            wb = np.ascontiguousarray(w).reshape(-1).view(np.uint8).reshape(w.size, -1)
            bad = np.flatnonzero((gb != wb).any(axis=1))
            at_ = np.unravel_index(bad[0], g.shape)
            assert False, (what, k, len(bad), at_, g[at_], w[at_])
