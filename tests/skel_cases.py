"""Sequences for the skeleton tests (test_skel_host.py: harness/skeleton.py against answers the rule alone decides;
test_gpu_skel.py: mpe_skel_* against the same answers and, bit for bit, against harness/skeleton.py).  Not a test module.

The known answers rest on exact arithmetic: the bin width is 2^-8 m, every coordinate a dyadic number of a few bits and
every hand-made bone lies along one axis, so d, s, l = sqrt(s), q = l / bin, e = (l - L) / l (l a power of two) and every
product of a sweep are exact in float64, and the results are exact in float32 as well."""
import numpy as np

import track_cases as tc

J = tc.J
ALL = (1 << J) - 1
BIN = 2.0 ** -8
L64 = 64.5 * BIN                     # 0.251953125, the centre of bin 64
L32 = 32.5 * BIN                     # 0.126953125
KEYS_LEN = ('len', 'count', 'out_of_range', 'over_ids', 'status')
KEYS_FIT = ('poses', 'err', 'n_bones')

NOISE_SIGMA = 0.01
NOISE_SEED = 23
NOISE_FRAMES = 200
# measured on harness/skeleton.py (200 frames, lengths from the noisy frames themselves, min_samples 10, bin 2 mm, 16
# sweeps): RMS distance to the truth 17.331 mm in, 14.257 mm out in both modes, ratio NOISE_RATIO (seeds 1, 2, 3: 0.8303, 0.8231,
# 0.8261); the worst bone of a row is off by 49.3 mm at most before and 0.37 mm after.  The bound is half way between that
# ratio and 1, the half being the margin for another seed.
NOISE_RATIO = 0.8226
NOISE_BOUND = 0.5 * (NOISE_RATIO + 1.0)

# a standing adult, metres, y up: nose, eyes, ears, shoulders, elbows, wrists, hips, knees, ankles, neck
BODY = np.array([[0.00, 1.62, 0.09], [0.03, 1.66, 0.07], [-0.03, 1.66, 0.07], [0.07, 1.64, 0.00], [-0.07, 1.64, 0.00],
                 [0.19, 1.45, 0.00], [-0.19, 1.45, 0.00], [0.24, 1.17, 0.02], [-0.24, 1.17, 0.02], [0.26, 0.92, 0.08],
                 [-0.26, 0.92, 0.08], [0.10, 0.95, 0.00], [-0.10, 0.95, 0.00], [0.11, 0.52, 0.03], [-0.11, 0.52, 0.03],
                 [0.11, 0.09, 0.00], [-0.11, 0.09, 0.00], [0.00, 1.47, 0.00]])


class Case:
    """rows: per frame a list of rows, each None or (id, pose [J,3]) or (id, pose, joints present) in mode 'tri' (mode
    'mlp': a row given as (id, pose, []) has no flag).  `steps` is what a test runs, in order: ('observe', frames),
    ('update', min_samples), ('set', table), ('fit', frames, iters), ('lengths',); frames is a slice of the case's frames.
    `expect` receives the list of what 'lengths' and 'fit' returned."""

    def __init__(self, mode, rows, bones, steps, expect, tid_cap=8, pcap=4, n_persons=None, joint_mask=ALL, bin_width=BIN):
        self.mode, self.bones, self.steps, self.expect = mode, list(bones), steps, expect
        self.tid_cap, self.pcap, self.joint_mask, self.bin_width = tid_cap, pcap, joint_mask, bin_width
        tri = mode == 'tri'
        B = len(rows)
        self.poses = np.zeros((B, pcap, J, 3), np.float64 if tri else np.float32)
        self.flags = np.zeros((B, pcap, J) if tri else (B, pcap), np.uint8)
        self.ids = np.full((B, pcap), -1, np.int32)
        self.n_persons = np.array([len(r) for r in rows], np.int32) if n_persons is None else np.asarray(n_persons, np.int32)
        for f, fr in enumerate(rows):
            for p, r in enumerate(fr):
                if r is None:
                    continue
                self.ids[f, p] = r[0]
                self.poses[f, p] = r[1]
                joints = list(r[2]) if len(r) > 2 else list(range(J))
                if tri:
                    self.flags[f, p, joints] = 1
                else:
                    self.flags[f, p] = 1 if joints else 0

    def frames(self, sl):
        return self.poses[sl], self.flags[sl], self.n_persons[sl], self.ids[sl]


def run_statement(S, c, bones=None):
    """the steps of a case through harness/skeleton.py -> the list of what 'lengths' and 'fit' returned"""
    st = S.new_state(c.tid_cap, c.bones if bones is None else bones, c.bin_width, J)
    out = []
    for step in c.steps:
        if step[0] == 'observe':
            S.observe_sequence(st, *c.frames(step[1]), c.mode, c.joint_mask)
        elif step[0] == 'update':
            S.length_table(st, step[1])
        elif step[0] == 'set':
            S.set_lengths(st, step[1])
        elif step[0] == 'fit':
            out.append(S.fit_sequence(st, *c.frames(step[1]), c.mode, c.joint_mask, step[2]))
        else:
            out.append({k: (st[k].copy() if isinstance(st[k], np.ndarray) else st[k]) for k in KEYS_LEN})
    return out


def pose(**at):
    """all joints at (9, 9, 9) + 0.25 * j along z (no two together), the named ones (j17=(x, y, z)) where given"""
    p = np.stack([np.full(J, 9.0), np.full(J, 9.0), 9.0 + 0.25 * np.arange(J)], axis=1)
    for k, v in at.items():
        p[int(k[1:])] = v
    return p


def one_bone(mode):
    """twelve frames with the bone at 0.251953125 (the centre of bin 64), then a frame with it at 0.5, one sweep"""
    rows = [[(3, pose(j17=(0, 0, 0), j0=(L64, 0, 0)))] for _ in range(12)] + [[(3, pose(j17=(0, 0, 0), j0=(0.5, 0, 0)))]]

    def expect(out):
        ln, fit = out
        assert ln['len'][3, 0] == L64 == 0.251953125 and ln['count'][3, 0] == 12 and ln['count'].sum() == 12 and not ln['len'][:3].any()
        assert (ln['out_of_range'], ln['over_ids'], ln['status']) == (0, 0, 0)
        assert fit['poses'][0, 0, 17].tolist() == [0.1240234375, 0, 0] and fit['poses'][0, 0, 0].tolist() == [0.3759765625, 0, 0]
        assert fit['err'][0, 0].tolist() == [0.248046875, 0.0] and fit['n_bones'][0].tolist() == [1, 0, 0, 0]
        assert (fit['err'][0, 1:] == -1.0).all()
    return Case(mode, rows, [(17, 0)], [('observe', slice(0, 12)), ('update', 10), ('lengths',), ('fit', slice(12, 13), 1)], expect)


def lower_median(mode):
    """track 0: bins 10 x 3, 20 x 4, 300 x 2 -> bin 20; track 1: bins 10 x 2, 20 x 2 -> bin 10, and none when five are asked for"""
    at = lambda t, k: [(t, pose(j17=(1, 1, 1), j0=(1 + (k + 0.5) * BIN, 1, 1)))]
    rows = [at(0, 10)] * 3 + [at(0, 20)] * 4 + [at(0, 300)] * 2 + [at(1, 10)] * 2 + [at(1, 20)] * 2

    def expect(out):
        first, second = out
        assert first['len'][0, 0] == 20.5 * BIN and first['len'][1, 0] == 10.5 * BIN and first['count'][:2, 0].tolist() == [9, 4]
        assert second['len'][0, 0] == 20.5 * BIN and second['len'][1, 0] == 0.0 and second['count'][:2, 0].tolist() == [9, 4]
        assert first['out_of_range'] == 0 and not first['len'][2:].any()
    return Case(mode, rows, [(17, 0)], [('observe', slice(0, 13)), ('update', 1), ('lengths',), ('update', 5), ('lengths',)], expect)


def bin_edges(mode):
    """track 0: l = 7 bins exactly -> bin 7; track 1: l = 512 bins and track 2: l = 0 -> out of range; track 3: a NaN
    coordinate, no sample; bone (0, 1) has joint 1 outside the mask: no sample for anybody"""
    nan = pose(j17=(1, 1, 1), j0=(1, 1.5, 1))
    nan[0, 2] = np.nan
    rows = [[(0, pose(j17=(1, 1, 1), j0=(1, 1 + 7 * BIN, 1))), (1, pose(j17=(1, 1, 1), j0=(1, 1, 1 + 512 * BIN))),
             (2, pose(j17=(1, 1, 1), j0=(1, 1, 1))), (3, nan)]]

    def expect(out):
        ln, fit = out
        assert ln['count'].sum() == 1 and ln['count'][0, 0] == 1 and ln['len'][0, 0] == 7.5 * BIN and np.count_nonzero(ln['len']) == 1
        assert (ln['out_of_range'], ln['over_ids'], ln['status']) == (2, 0, 0)
        # track 0 is fitted (bone 0 only), the others have no length and are copied through, NaN included
        assert fit['n_bones'][0].tolist() == [1, 0, 0, 0] and fit['err'][0, 0, 0] == 0.5 * BIN
        assert fit['poses'][0, 1:].tobytes() == c.poses[0, 1:].tobytes() and (fit['err'][0, 1:] == -1.0).all()
    c = Case(mode, rows, [(17, 0), (0, 1)], [('observe', slice(0, 1)), ('update', 1), ('lengths',), ('fit', slice(0, 1), 1)], expect,
             joint_mask=ALL & ~(1 << 1))
    return c


def ids_and_rows(mode):
    """ids 5 and 6 with different lengths whose rows swap every frame; id 9 >= tid_cap = 8; in every frame, the fitted one
    included, a row of id 5 at another length that is no sample and is not fitted: in mode 'mlp' it has no flag, in mode
    'tri' its joint 0 is absent; and a row past n_persons with id 6 at yet another length"""
    a = lambda x: pose(j17=(0, 0, 0), j0=(x, 0, 0))
    off = (5, a(0.75), [] if mode == 'mlp' else [j for j in range(J) if j != 0])
    rows = []
    for f in range(12):
        two = [(5, a(L64)), (6, a(L32))]
        rows.append((two if f % 2 == 0 else two[::-1]) + [(9, a(0.375)), off, (6, a(0.625))])
    rows.append([(6, a(0.5)), (5, a(0.5)), (9, a(0.5)), off, (6, a(0.625))])
    n_persons = [4] * 13

    def expect(out):
        ln, fit = out
        assert ln['len'][5, 0] == L64 and ln['len'][6, 0] == L32 and np.count_nonzero(ln['len']) == 2
        assert ln['count'][5, 0] == ln['count'][6, 0] == 12 and ln['count'].sum() == 24          # neither the row without a flag nor the one past n_persons
        assert (ln['out_of_range'], ln['over_ids'], ln['status']) == (0, 12, 1)
        assert fit['poses'][0, 0, 17, 0] == 0.1865234375 and fit['poses'][0, 0, 0, 0] == 0.3134765625
        assert fit['poses'][0, 1, 17, 0] == 0.1240234375 and fit['poses'][0, 1, 0, 0] == 0.3759765625
        assert fit['err'][0].tolist() == [[0.5 - L32, 0.0], [0.5 - L64, 0.0], [-1.0, -1.0], [-1.0, -1.0], [-1.0, -1.0]]
        assert fit['n_bones'][0].tolist() == [1, 1, 0, 0, 0] and fit['poses'][0, 2:].tobytes() == c.poses[12, 2:].tobytes()
        others = [j for j in range(J) if j not in (0, 17)]
        assert fit['poses'][0][:, others].tobytes() == c.poses[12][:, others].tobytes()
    c = Case(mode, rows, [(17, 0)], [('observe', slice(0, 12)), ('update', 10), ('lengths',), ('fit', slice(12, 13), 1)], expect,
             pcap=5, n_persons=n_persons)
    return c


def already_fits(mode):
    """a three-bone axis-aligned chain that has the uploaded lengths: nothing moves, and nothing was observed"""
    p = pose(j17=(1, 1, 1), j0=(1.5, 1, 1), j1=(1.5, 1.25, 1), j3=(1.5, 1.25, 0.875))
    table = np.zeros((8, 3))
    table[2] = (0.5, 0.25, 0.125)
    table[3] = (np.inf, -1.0, np.nan)                        # no lengths

    def expect(out):
        fit, ln = out
        assert fit['poses'].tobytes() == c.poses.tobytes()
        assert fit['err'][0].tolist() == [[0.0, 0.0], [-1.0, -1.0], [-1.0, -1.0], [-1.0, -1.0]] and fit['n_bones'][0].tolist() == [3, 0, 0, 0]
        assert ln['len'].tobytes() == table.tobytes() and not ln['count'].any()
    c = Case(mode, [[(2, p), (3, p)]], [(17, 0), (0, 1), (1, 3)], [('set', table), ('fit', slice(0, 1), 7), ('lengths',)], expect)
    return c


def hand_made():
    cases = {}
    for mode in ('mlp', 'tri'):
        for make in (one_bone, lower_median, bin_edges, ids_and_rows, already_fits):
            cases['%s_%s' % (make.__name__, mode)] = make(mode)
    return cases


def noise(mode='tri', B=NOISE_FRAMES):
    """BODY walking 1 cm per frame and turning 1.5 degrees per frame about the vertical, as track 1 in row 0, with seeded
    Gaussian noise of NOISE_SIGMA per coordinate -> (truth [B,1,J,3], poses, flags, n_persons, ids)"""
    rng = np.random.default_rng(NOISE_SEED)
    tri = mode == 'tri'
    truth = np.zeros((B, 1, J, 3))
    for f in range(B):
        th = np.deg2rad(1.5 * f)
        R = np.array([[np.cos(th), 0, np.sin(th)], [0, 1, 0], [-np.sin(th), 0, np.cos(th)]])
        truth[f, 0] = BODY @ R.T + np.array([0.01 * f, 0.0, 0.5])
    poses = (truth + rng.normal(0.0, NOISE_SIGMA, truth.shape)).astype(np.float64 if tri else np.float32)
    flags = np.ones((B, 1, J) if tri else (B, 1), np.uint8)
    return truth, poses, flags, np.ones(B, np.int32), np.ones((B, 1), np.int32)


def rms(poses, truth):
    d = np.asarray(poses, np.float64) - truth
    return float(np.sqrt((d * d).sum(axis=-1).mean()))


def same(got, want, keys, what=''):
    for k in keys:
        g, w = np.asarray(got[k]), np.asarray(want[k])
        assert g.shape == w.shape and (g.dtype == w.dtype or g.ndim == 0), (what, k, g.dtype, w.dtype, g.shape, w.shape)
        if g.tobytes() != w.tobytes():
            if g.ndim == 0:
                assert False, (what, k, g, w)
            gb = np.ascontiguousarray(g).reshape(-1).view(np.uint8).reshape(g.size, -1)
            wb = np.ascontiguousarray(w).reshape(-1).view(np.uint8).reshape(w.size, -1)
            bad = np.flatnonzero((gb != wb).any(axis=1))
            at_ = np.unravel_index(bad[0], g.shape)
            assert False, (what, k, len(bad), at_, g[at_], w[at_])
