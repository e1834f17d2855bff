"""Inputs for the consolidation tests (test_consolidate_host.py: harness/consolidate.py on its own; test_gpu_consolidate.py:
mpe_consolidate_batch against it).  Built the way regroup_cases.py builds its cases: synthetic frames (seed 1234), the true
rows from the generator's ground-truth pairing, the poses the ground-truth bodies (float64 with joint flags, and rounded to
float32 with person flags).  A body that is split over rows has its own pose in the first row and the pose a few
centimetres off (SHIFT per further row) in the others.  Every case damages the true rows in the way it is named for and
asserts, with the statement's own diagnostics, that the branch it is there for is taken and that the statement gives the
rows it expects: a condition on the seeds, checked on the CPU.  Not a test module."""
import json

import numpy as np

from conftest import env, oracle, pkg
from refine_cases import RIG_FRAMES, only_seen_by
from regroup_cases import drop_skeleton, duplicate_skeleton, keep_joints, rows_from_owners, same_bits  # noqa: F401

J = 18
SHIFT = np.array([0.02, -0.01, 0.015])        # metres between the poses of two rows of one body: 27 mm
NAMES = ('clean', 'split', 'chain', 'shared', 'edge', 'edge_up', 'lost', 'stray', 'short', 'unscored', 'tie', 'full', 'free_cap',
         'bad_rows', 'degenerate', 'arplab', 'explicit', 'lanes', 'ring23', 'arprobot')
KEYS = ('persons', 'n_persons', 'change', 'n_views', 'dist', 'pair', 'free', 'counts', 'status')
_made = {}


def option_sets(params):
    """The three option sets of the GPU tests: the defaults; merge only with a clip; found only on the used joints."""
    return [{}, {'found': False, 'clip_m': 0.3}, {'merge': False, 'joint_mask': sum(1 << j for j in params.used_joints)}]


def spec_of(name):
    """-> (frames, FrameSpec, the number of bodies without a row (the last ones))."""
    syn = pkg('synthetic')
    S = syn.FrameSpec
    if name == 'clean':
        return 3, S(persons=4), 0
    if name in ('split', 'chain', 'shared', 'bad_rows'):
        return 5, S(persons=4, noise_px=1.0), 0
    if name in ('edge', 'edge_up'):
        return 1, S(persons=4, noise_px=1.0), 0
    if name == 'lost':
        return 2, S(persons=10, noise_px=1.0), 1
    if name == 'stray':
        return 3, S(persons=4, noise_px=1.0, spurious=1), 0
    if name == 'short':
        return 6, S(persons=4, noise_px=1.0), 2
    if name in ('unscored', 'tie', 'full', 'explicit'):
        return (1 if name == 'explicit' else 3), S(persons=4, noise_px=1.0), 1
    if name == 'free_cap':
        return 2, S(persons=4, noise_px=1.0), 2
    if name == 'degenerate':
        return 4, S(persons=3, noise_px=1.0), 0
    if name == 'arplab':
        return 3, S(persons=3, noise_px=1.0), 1
    if name == 'lanes':
        return 4, S(persons=10), 0
    if name == 'ring23':
        return 3, S(persons=3, noise_px=1.0), 1                           # (frames 1 and 2: no body has a row)
    if name == 'arprobot':
        return 3, S(persons=3, noise_px=1.0), 1
    raise KeyError(name)


class Case:
    """One batch (`pb`), the rows and counts that go in (`rows`, `n_persons`), both kinds of poses with their flags
    (`kinds()`), the options the case is run with (`opts`), per kind what the statement gives (`statement(kind)`), and the
    rows the merge alone must give (`merged`)."""

    def __init__(self, name, pcap=None):
        syn, onp = pkg('synthetic'), oracle()
        self.name = name
        self.variant = name if name in ('arplab', 'ring23', 'arprobot') else 'panoptic'
        self.env = env(self.variant)
        calib, params = self.calib, self.params = self.env.calib, self.env.params
        cams = list(params.used_cameras_skeleton_matching)
        names = list(params.camera_names)
        self.cams, V = cams, len(cams)
        F, spec, rowless = spec_of(name)
        if name in RIG_FRAMES:
            frames, gts = zip(*[syn.make_frame(calib, i, spec, seed=1234) for i in RIG_FRAMES[name]])
        else:
            frames, gts = syn.make_frames(calib, F, spec, seed=1234)
        frames = [{c: list(v) for c, v in f.items()} for f in frames]
        owners = [{c: list(v) for c, v in g['owner'].items()} for g in gts]
        bodies = [np.asarray(g['persons'], np.float64) for g in gts]
        P = spec.persons
        self.opts = {}

        # what the case does to the frames themselves
        if name == 'stray':
            for f in range(F):
                drop_skeleton(frames[f], owners[f], names[f % V], f % 4)
        if name == 'lost':
            for f in range(F):
                drop_skeleton(frames[f], owners[f], names[1], 3)
                drop_skeleton(frames[f], owners[f], names[1], 4)
        if name == 'short':
            # body 3 keeps the two cameras in which its skeletons fit best: in some frames that pair seeds before any of body 2
            CS = pkg('harness.consolidate')
            pb0 = pkg('packing').pack_frames([onp.processed_input(f) for f in frames], params)
            true0 = rows_from_owners(pb0, owners, [4] * F, 4, cams)
            o, r = CS.G.rays(calib, pb0.head_cam, pb0.xy)
            votes = CS.head_votes(pb0, (1 << J) - 1)
            for f in range(F):
                heads = np.sort(true0[f, 3]).astype(np.int64) + int(pb0.frame_head_off[f])
                cost = CS.pair_costs(o, r, np.asarray(pb0.head_cam, np.int64), votes, heads)
                a, b = np.unravel_index(np.argmin(np.where(cost >= 0, cost, np.inf)), cost.shape)
                only_seen_by(frames[f], owners[f], 3, [names[int(pb0.head_cam[heads[a]])], names[int(pb0.head_cam[heads[b]])]])
            self.opts['found_min_views'] = 3
        if name == 'unscored':
            for f in range(F):
                keep_joints(frames[f], owners[f], names[(f + 2) % V], 3, 2)
        if name == 'tie':
            for f in range(F):
                duplicate_skeleton(frames[f], owners[f], names[(f + 1) % V], 3)
        if name == 'degenerate':
            frames[1], _ = syn.make_frame(calib, 1, syn.FrameSpec(persons=3, empty_cameras=names), seed=1234)
            owners[1] = {c: [] for c in names}
        if name == 'free_cap':
            self.opts['fcap'] = 4
        if name == 'ring23':
            # frame 1: 69 heads less five skeletons, all free: exactly the 64 lanes of a wave, the 64 bits of a word
            for cam, b in ((0, 0), (1, 0), (2, 1), (3, 1), (4, 2)):
                drop_skeleton(frames[1], owners[1], names[cam], b)
            self.opts['fcap'] = 64
        if name == 'arprobot':
            # two frames carry the two used streams only, the third all six
            frames = [{c: v for c, v in fr.items() if c in cams or f == 2} for f, fr in enumerate(frames)]

        self.frames, self.owners, self.bodies = frames, owners, bodies
        self.processed = [onp.processed_input(f) for f in frames]
        if name == 'explicit':
            # heads in person order, a handful of edge-nodes of its own, no slot tables
            heads = []
            for o in range(P):
                for cam in cams:
                    if o in owners[0][cam]:
                        i = owners[0][cam].index(o)
                        heads.append((cam, i, json.loads(frames[0][cam][0])[i]))
            pairs = [(a, b) for a in range(4) for b in range(4, 8) if heads[a][0] != heads[b][0]]
            self.pb = pkg('packing').pack_scenes([{'heads': heads, 'pairs': np.array(pairs, np.int32)}], params)
            assert self.pb.en_pair is not None and self.pb.head_cam[0] != self.pb.head_cam[1]        # not grouped by camera
        else:
            self.pb = pkg('packing').pack_frames(self.processed, params)
        pb = self.pb
        self.most = max([1] + [f[c][0].count('{') for f in self.processed for c in f])
        self.true = true = rows_from_owners(pb, owners, [P] * F, P, cams)                            # [F,P,V]: body o is row o

        # the rows of every frame: the bodies that keep a row, then the parts split off
        plans = []
        for f in range(F):
            keep, splits = list(range(P - rowless)), {}
            if name in ('split', 'edge', 'edge_up', 'free_cap', 'explicit', 'arplab', 'bad_rows'):
                b = f % len(keep)
                held = [c for c in range(V) if true[f, b, c] >= 0]
                splits[b] = [held[2:]]
            if name == 'chain':
                b = f % 4
                held = [c for c in range(V) if true[f, b, c] >= 0]
                splits[b] = [held[2:4], held[4:]]
            if name == 'shared':
                b = f % 4
                splits[b] = [[3, 4]]
            if name == 'degenerate' and f in (2, 3):
                splits[0] = [[2, 3, 4]]
            if name == 'degenerate' and f == 0:
                keep = []
            if name == 'ring23':
                # frame 0: body 0 split into cameras 0..11 and 12..22, body 2 without a row; frames 1 and 2: no rows at all
                if f == 0:
                    splits[0] = [list(range(12, V))]
                else:
                    keep = []
            if name == 'arprobot' and f == 1:
                splits[0] = [[1]]                                         # a row per camera
            plans.append((keep, splits))
        built = []
        for f, (keep, splits) in enumerate(plans):
            rows, body, shift = [true[f, b].copy() for b in keep], list(keep), [0] * len(keep)
            for b, groups in splits.items():
                p = keep.index(b)
                for k, g in enumerate(groups, 1):
                    new = np.full(V, -1, np.int32)
                    for c in g:
                        assert rows[p][c] >= 0, (name, f, b, c)
                        new[c], rows[p][c] = rows[p][c], -1
                    rows.append(new), body.append(b), shift.append(k)
            built.append((rows, body, shift))
        n_rows = [len(b[0]) for b in built]
        if pcap is None:
            pcap = max(n_rows) + (10 if name == 'lanes' else 4)
        if name == 'full':
            n_rows = [pcap] * F                                           # rows without heads and without a pose up to the cap
        assert pcap >= max(n_rows), (name, pcap, n_rows)
        self.pcap = pcap
        self.n_persons = np.asarray(n_rows, np.int32)
        self.rows = rows = np.full((F, pcap, V), -1, np.int32)
        self.merged = merged = np.full((F, pcap, V), -1, np.int32)      # what the merge alone must give
        self.truth = np.zeros((F, pcap, J, 3))
        self.jflags = np.zeros((F, pcap, J), np.uint8)
        self.pflags = np.zeros((F, pcap), np.uint8)
        for f, (rr, body, shift) in enumerate(built):
            for p, (r, b, k) in enumerate(zip(rr, body, shift)):
                rows[f, p] = r
                self.truth[f, p] = bodies[f][b] + k * SHIFT
                self.jflags[f, p] = 1
                self.pflags[f, p] = 1
                if k == 0:
                    merged[f, p] = true[f, b]
        if name in ('degenerate', 'arplab'):
            f, p, j = np.meshgrid(np.arange(F), np.arange(pcap), np.arange(J), indexing='ij')
            self.jflags[((f + 2 * p + j) % 7 == 0) & (self.jflags != 0)] = 0     # joints the triangulation did not give

        # what the case does to the rows
        if name == 'shared':
            for f in range(F):
                b, other = f % 4, (f + 1) % 4
                rows[f, 4, 2], rows[f, other, 2] = rows[f, other, 2], -1  # the split-off row holds a wrong head of camera 2
            merged[...] = rows
        if name == 'lost':
            rows[:, [1, 5]] = -1                                          # two rows that kept their pose and lost their heads
            merged[...] = rows
        if name == 'lanes':
            rows[0] = -1                                                  # K = 50
            rows[1, 3, 2] = -1                                            # K = 1
            rows[2, 4, [0, 3]] = -1                                       # K = 2
            rows[3, :6] = -1
            rows[3, 6, [0, 1, 2]] = -1                                    # K = 33
            merged[...] = rows
        if name == 'bad_rows':
            rows[0, 2, 1] = rows[0, 2, 3]                                 # a head of camera 3 under column 1
            rows[2, 3, 4] = rows[2, 1, 4] if rows[2, 1, 4] >= 0 else rows[2, 0, 4]      # two rows name one head
            rows[3, 1, 0] = pb.frame_counts(3)[1]                         # one past the frame's heads
            merged[[0, 2, 3]] = rows[[0, 2, 3]]
        if name == 'degenerate':
            self.truth[2, 3, 3] = np.nan                                  # frame 2: a joint of the split-off row is not a number
            self.pflags[3, 3] = 0                                         # frame 3: the split-off row has no person flag (kind est)
        self.est = self.truth.astype(np.float32)
        if name in ('edge', 'edge_up'):
            d = pkg('harness.consolidate').dist_table(self.truth, self.jflags, self.n_persons, (1 << J) - 1)[0, 0, 4]
            assert 0.02 < d < 0.04
            self.edge = float(d)
            self.opts['merge_m'] = float(d) if name == 'edge' else float(np.nextafter(d, np.inf))
            if name == 'edge':
                merged[...] = rows
        self._out = {}
        self.check()

    def kinds(self):
        """{kind: (poses, flags, joint mask)} as Engine.consolidate / harness.consolidate take them."""
        return {'triang': (self.truth, self.jflags, (1 << J) - 1),
                'est': (self.est, self.pflags, sum(1 << j for j in self.params.used_joints))}

    def statement(self, kind, rows=None, n_persons=None, **opts):
        """harness.consolidate.consolidate on the case with the case's options (cached for the case's own rows)."""
        poses, flags, mask = self.kinds()[kind]
        opts = dict(self.opts, **opts)
        opts.setdefault('joint_mask', mask)
        CS = pkg('harness.consolidate')
        if rows is not None or 'trace' in opts or 'out' in opts or 'n_out' in opts:
            return CS.consolidate(self.calib, self.pb, self.rows if rows is None else rows, self.n_persons if n_persons is None else n_persons,
                                  poses, flags, **opts)
        key = (kind,) + tuple(sorted(opts.items()))
        if key not in self._out:
            self._out[key] = CS.consolidate(self.calib, self.pb, self.rows, self.n_persons, poses, flags, **opts)
        return self._out[key]

    def heads_of(self, f, b):
        """The frame-local heads of body b of frame f."""
        pb = self.pb
        h0, H, _, _ = pb.frame_counts(f)
        return frozenset(i for i in range(H) if self.owners[f][self.cams[int(pb.head_cam[h0 + i])]][int(pb.skeleton_index[h0 + i])] == b)

    def founded(self, o, f):
        """The rows the statement founded in frame f, as a list of frozensets of heads."""
        n0, n1 = int(self.n_persons[f]), int(o['n_persons'][f])
        return [frozenset(int(h) for h in o['persons'][f, p] if h >= 0) for p in range(n0, n1)]

    def check(self):
        """The branches the case is there for, by the statement's diagnostics (the case's options, f64 poses)."""
        CS = pkg('harness.consolidate')
        name, pb, F = self.name, self.pb, self.pb.n_frames
        trace = []
        o = self.statement('triang', trace=trace)
        only_merge = self.statement('triang', found=False)
        assert np.array_equal(only_merge['persons'], self.merged), (name, 'the merge does not give the expected rows')
        for kind in ('triang', 'est'):
            x = self.statement(kind)
            for k in ('dist', 'pair'):
                assert (x[k][x[k] != -1.0] >= 0.0).all() and np.isfinite(x[k]).all()
        c = o['counts']
        if name == 'clean':
            assert not o['change'].any() and not c[:, :3].any() and not o['status'].any() and np.array_equal(o['n_persons'], self.n_persons)
        if name in ('split', 'edge_up'):
            assert (c == [1, 0, 0, 0]).all() and (o['persons'][:, 4] == -1).all() and np.array_equal(o['persons'][:, :4], self.true)
        if name == 'chain':
            assert (c == [2, 0, 0, 0]).all() and (o['persons'][:, 4:] == -1).all() and np.array_equal(o['persons'][:, :4], self.true)
        if name == 'shared':
            d = np.array([o['dist'][f, f % 4, 4] for f in range(F)])
            assert ((d >= 0) & (d < 0.1)).all() and not c[:, 0].any() and not o['change'].any()
        if name == 'edge':
            assert o['dist'][0, 0, 4] == self.opts['merge_m'] and not o['change'].any()
        if name == 'lost':
            assert pb.max_heads_per_frame() == 48
            for f in range(F):
                assert sorted(self.founded(o, f), key=sorted) == sorted((self.heads_of(f, b) for b in (1, 5, 9)), key=sorted), (name, f)
            assert (c == [0, 3, 15, 0]).all()
            for gate in (0.03, 0.10):
                x = self.statement('triang', found_m=gate)
                assert all(sorted(self.founded(x, f), key=sorted) == sorted(self.founded(o, f), key=sorted) for f in range(F))
        if name == 'stray':
            assert (c == [0, 0, 0, 5]).all() and not o['change'].any()
            scored = o['pair'][o['pair'] >= 0]
            assert len(scored) and scored.min() > 0.1
        if name == 'short':
            assert all(len(self.heads_of(f, 3)) == 2 for f in range(F))
            for f in range(F):
                assert self.founded(o, f) == [self.heads_of(f, 2)] and c[f].tolist() == [0, 1, 5, 2]
            order = [[t[4] for t in trace if t[0] == f] for f in range(F)]
            assert any(s[:2] == [False, True] for s in order), order      # a seed dissolved, a later one founds
            assert all(sorted(s) == [False, True] for s in order)
        if name == 'unscored':
            for f in range(F):
                k = (f + 2) % pb.V
                cut = [h for h in self.heads_of(f, 3) if pb.head_cam[pb.frame_counts(f)[0] + h] == k]
                assert len(cut) == 1 and self.founded(o, f) == [self.heads_of(f, 3) - set(cut)] and c[f].tolist() == [0, 1, 4, 1]
                r = o['free'][f].tolist().index(cut[0])
                assert (o['pair'][f, r] == -1).all() and (o['pair'][f, :, r] == -1).all()
        if name == 'tie':
            for f in range(F):
                body, dup, h0 = self.heads_of(f, 3), sorted(self.heads_of(f, -99)), pb.frame_counts(f)[0]
                assert len(dup) == 1                                      # (duplicate_skeleton gives the copy the owner -99)
                orig = [h for h in body if pb.head_cam[h0 + h] == pb.head_cam[h0 + dup[0]]]
                low = min(orig[0], dup[0])
                assert self.founded(o, f) == [(body - set(orig)) | {low}] and c[f].tolist() == [0, 1, 5, 1]
                ra, rb = o['free'][f].tolist().index(orig[0]), o['free'][f].tolist().index(dup[0])
                rest = [r for r in range(6) if r not in (ra, rb)]
                assert same_bits(np.where(np.arange(6)[rest] < ra, o['pair'][f, rest, ra], o['pair'][f, ra, rest]),
                                 np.where(np.arange(6)[rest] < rb, o['pair'][f, rest, rb], o['pair'][f, rb, rest]))
        if name == 'full':
            assert (self.n_persons == self.pcap).all() and (o['status'] == CS.ROWS_FULL).all() and (c == [0, 0, 0, 5]).all()
            assert not o['change'].any() and (o['pair'] >= 0).any()
        if name == 'free_cap':
            assert (o['status'] == CS.FREE_OVER_CAP).all() and (c == [1, 0, 0, 10]).all() and (o['pair'] == -1).all()
            assert (o['free'] >= 0).all() and o['free'].shape == (F, 4)
        if name == 'bad_rows':
            assert o['status'].tolist() == [1, 0, 1, 1, 0] and c[[0, 2, 3]].sum() == 0 and c[1].tolist() == [1, 0, 0, 0]
            assert (o['dist'][[0, 2, 3]] == -1).all() and (o['pair'][[0, 2, 3]] == -1).all() and (o['free'][[0, 2, 3]] == -1).all()
            assert np.array_equal(o['persons'][[0, 2, 3]], self.rows[[0, 2, 3]])
        if name == 'degenerate':
            assert self.n_persons[0] == 0 and sorted(self.founded(o, 0), key=sorted) == sorted((self.heads_of(0, b) for b in range(3)), key=sorted)
            assert pb.frame_counts(1)[1] == 0 and not c[1].any() and o['n_persons'][1] == 3
            assert c[2].tolist() == [1, 0, 0, 0] and c[3].tolist() == [1, 0, 0, 0]
            e = self.statement('est')
            assert e['counts'][3].tolist() == [0, 0, 0, 0] and (e['dist'][3, :, 3] == -1).all()      # no flag, no pose, no merge
        if name == 'arplab':
            assert pb.V == 6 and (c[:, 0] == 1).all() and (c[:, 1] == 1).all()
            assert all(self.founded(o, f) == [self.heads_of(f, 2)] for f in range(F))
        if name == 'ring23':
            assert pb.V == 23 and [pb.frame_counts(f)[1] for f in range(F)] == [69, 64, 69] and self.n_persons.tolist() == [3, 0, 0]
            # frame 0: the two halves merged into a row of 23 views, body 2 founded with 23 views
            assert c[0].tolist() == [1, 1, 23, 0] and o['status'][0] == 0 and self.founded(o, 0) == [self.heads_of(0, 2)]
            assert o['n_views'][0, [0, 1, 3]].tolist() == [23, 23, 23] and (o['persons'][0, 0] >= 0).all() and (o['persons'][0, 2] == -1).all()
            assert max(len(t[3]) for t in trace if t[0] == 0) == 23
            # frame 1: 64 free heads in 64 slots, status 0, the three bodies founded
            assert o['status'][1] == 0 and (o['free'][1] >= 0).sum() == 64 and o['free'].shape == (F, 64) and (o['pair'][1] >= 0).any()
            assert sorted(self.founded(o, 1), key=sorted) == sorted((self.heads_of(1, b) for b in range(3)), key=sorted)
            assert c[1].tolist() == [0, 3, 64, 0]
            # frame 2: 69 free heads do not fit
            assert o['status'][2] == CS.FREE_OVER_CAP and o['n_persons'][2] == 0 and c[2].tolist() == [0, 0, 0, 69] and (o['pair'][2] == -1).all()
        if name == 'arprobot':
            assert pb.V == 2 and [len(f) for f in self.frames] == [2, 2, 6] and not o['status'].any()
            assert c[:, 0].tolist() == [0, 1, 0] and (c[:, 1:] == [1, 2, 0]).all()
            for f in range(F):
                assert self.founded(o, f) == [self.heads_of(f, 2)] and len(self.heads_of(f, 2)) == 2
                assert [len(t[3]) for t in trace if t[0] == f and t[4]] == [2]        # the seed pair is the whole row: no growth round
        if name == 'explicit':
            assert pb.en_pair is not None and c.tolist() == [[1, 1, 5, 0]] and self.founded(o, 0) == [self.heads_of(0, 3)]
        if name == 'lanes':
            assert pb.max_heads_per_frame() == 50 and c[:, 3].tolist() == [0, 1, 0, 0] and c[:, 2].tolist() == [50, 0, 2, 33]
            assert (o['free'] >= 0).sum(axis=1).tolist() == [50, 1, 2, 33]
            assert sorted(self.founded(o, 0), key=sorted) == sorted((self.heads_of(0, b) for b in range(10)), key=sorted)


def case(name, pcap=None):
    """The case, with its own row capacity or (for an engine's tensors) the one given."""
    if (name, pcap) not in _made:
        _made[name, pcap] = Case(name, pcap)
    return _made[name, pcap]


# ---- the end-to-end input: the `messy` batch of geom_cases with one person's row deleted per frame -----------------------------

def deleted_row(f, n):
    """The row of frame f (of n rows) the end-to-end tests delete."""
    return f % n


def delete_rows(rows, n):
    """-> (rows, n) with row deleted_row(f, n[f]) of every frame gone: the last row takes its place, the count falls by one."""
    rows, n = rows.copy(), n.copy()
    for f in range(len(n)):
        if n[f] > 0:
            rows[f, deleted_row(f, int(n[f]))] = rows[f, n[f] - 1]
            rows[f, n[f] - 1] = -1
            n[f] -= 1
    return rows, n


def triangulated_on_cpu(c, pb, rows, n):
    """The oracle's triangulation (all joints) of the rows -> (poses [F,pcap,J,3] f64, joint flags [F,pcap,J])."""
    onp = oracle()
    cams = list(c.params.used_cameras_skeleton_matching)
    F, pcap = rows.shape[:2]
    poses, jv = np.zeros((F, pcap, J, 3)), np.zeros((F, pcap, J), np.uint8)
    for f in range(F):
        for p in range(int(n[f])):
            skels = {cams[k]: pb.jsons_for_head[f][int(h)] for k, h in enumerate(rows[f, p]) if h >= 0}
            if len(skels) >= 2:
                for j, xyz in onp.triangulate_person(skels, c.calib, all_joints=True).items():
                    poses[f, p, j], jv[f, p, j] = xyz, 1
    return poses, jv


def repaired_on_cpu(c, pb, rows, n):
    """triangulate, regroup, triangulate, consolidate, all on the CPU -> consolidate's outputs."""
    mask = (1 << J) - 1
    poses, jv = triangulated_on_cpu(c, pb, rows, n)
    rg = pkg('harness.regroup').regroup(c.calib, pb, rows, n, poses, jv, mask)
    poses, jv = triangulated_on_cpu(c, pb, rg['persons'], n)
    return pkg('harness.consolidate').consolidate(c.calib, pb, rg['persons'], n, poses, jv, mask)


def messy_restored():
    """Per frame of the `messy` batch: after one row is deleted, the repairs on the CPU give back the partition the rows had
    before the deletion."""
    import regroup_cases as rc
    if 'messy' not in _made:
        c, rows, n, _, _ = rc.messy_on_cpu()
        pb = pkg('packing').pack_frames(c.processed, c.params, keep_json=True)
        cut, n_cut = delete_rows(rows, n)
        o = repaired_on_cpu(c, pb, cut, n_cut)
        _made['messy'] = [rc.partition_of(o['persons'][f], o['n_persons'][f]) == rc.partition_of(rows[f], n[f]) for f in range(pb.n_frames)]
    return _made['messy']
