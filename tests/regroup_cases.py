"""Inputs for the regrouping tests (test_regroup_host.py: harness/regroup.py on its own; test_gpu_regroup.py:
mpe_regroup_batch against it).  Built the way geom_cases.py and refine_cases.py build theirs: synthetic frames, the true
rows from the generator's ground-truth pairing, the poses the ground-truth bodies (float64 with joint flags, and rounded to
float32 with person flags).  Every case damages the true rows in the way it is named for and states the rows it expects
back; every case asserts, with the statement's own diagnostics, that the branch it is there for is taken, and -- for swap,
orphan, noisy and crowd -- that the statement restores the expected rows: a condition on the seeds, not a measurement.
Not a test module."""
import json

import numpy as np

from conftest import env, oracle, pkg
from refine_cases import RIG_FRAMES, behind_camera, same_bits  # noqa: F401  (the GPU tests compare with same_bits)

J = 18
NAMES = ('clean', 'swap', 'orphan', 'stray', 'noisy', 'crowd', 'tie', 'degenerate', 'bad_rows', 'explicit', 'arplab', 'ring23', 'arprobot')
RESTORED = ('swap', 'orphan', 'noisy', 'crowd', 'arplab', 'ring23', 'arprobot')
_made = {}


def option_sets(params):
    """The three option sets of the GPU tests: the defaults; release only with a clip; attach only on the used joints."""
    return [{}, {'attach': False, 'clip_px': 40.0}, {'release': False, 'joint_mask': sum(1 << j for j in params.used_joints)}]


def drop_skeleton(frame, owner, cam, person):
    """The skeleton of `person` removed from camera `cam` (frame and owner lists, in place)."""
    i = owner[cam].index(person)
    sks = json.loads(frame[cam][0])
    del sks[i], owner[cam][i]
    frame[cam][0] = json.dumps(sks)


def keep_joints(frame, owner, cam, person, n):
    """The skeleton of `person` in camera `cam` cut down to its first n joints."""
    i = owner[cam].index(person)
    sks = json.loads(frame[cam][0])
    sks[i] = dict(list(sks[i].items())[:n])
    frame[cam][0] = json.dumps(sks)


def duplicate_skeleton(frame, owner, cam, person):
    """A copy of the skeleton of `person` appended to the list of camera `cam`; nobody owns the copy."""
    sks = json.loads(frame[cam][0])
    sks.append(dict(sks[owner[cam].index(person)]))
    owner[cam].append(-99)
    frame[cam][0] = json.dumps(sks)


def rows_from_owners(pb, owners, n_rows, pcap, cams):
    """rows [F,pcap,V] (frame-local head ids, -1 without one): body o < n_rows[f] of a frame is row o."""
    rows = np.full((pb.n_frames, pcap, pb.V), -1, np.int32)
    for f in range(pb.n_frames):
        h0, H, _, _ = pb.frame_counts(f)
        for i in range(H):
            c = int(pb.head_cam[h0 + i])
            o = owners[f][cams[c]][int(pb.skeleton_index[h0 + i])]
            if 0 <= o < n_rows[f]:
                rows[f, o, c] = i
    return rows


def head_of(rows, f, p, c):
    h = int(rows[f, p, c])
    assert h >= 0, ('no head', f, p, c)
    return h


def swap(rows, f, c, a, b):
    head_of(rows, f, a, c), head_of(rows, f, b, c)
    rows[f, a, c], rows[f, b, c] = rows[f, b, c], rows[f, a, c]


def orphan(rows, f, p, c):
    head_of(rows, f, p, c)
    rows[f, p, c] = -1


class Case:
    """One batch (`pb`, from `processed` unless the case is `explicit`), the rows that go in (`rows`), per kind the rows
    expected under the default options (`want`), and both kinds of poses with their flags (`kinds()`)."""

    def __init__(self, name, pcap=None):
        syn, onp = pkg('synthetic'), oracle()
        self.name = name
        self.variant = name if name in ('arplab', 'ring23', 'arprobot') else 'panoptic'
        self.env = env(self.variant)
        calib, params = self.calib, self.params = self.env.calib, self.env.params
        cams = list(params.used_cameras_skeleton_matching)
        names = list(params.camera_names)
        self.cams, V = cams, len(cams)
        spec = {'clean': (17, syn.FrameSpec(persons=4), 1234), 'swap': (5, syn.FrameSpec(persons=4, noise_px=1.0), 1234),
                'orphan': (5, syn.FrameSpec(persons=4, noise_px=1.0), 1234), 'stray': (3, syn.FrameSpec(persons=4, noise_px=1.0, spurious=1), 1234),
                'noisy': (6, syn.FrameSpec(persons=4, noise_px=2.0, joint_drop=0.3), 1234), 'crowd': (2, syn.FrameSpec(persons=10, noise_px=1.0), 1234),
                'tie': (1, syn.FrameSpec(persons=3, noise_px=1.0), 1234), 'degenerate': (6, syn.FrameSpec(persons=3, noise_px=1.0), 1234),
                'bad_rows': (4, syn.FrameSpec(persons=4, noise_px=1.0), 1234), 'explicit': (1, syn.FrameSpec(persons=4, noise_px=1.0), 1234),
                'arplab': (3, syn.FrameSpec(persons=3, noise_px=1.0), 1234), 'ring23': (3, syn.FrameSpec(persons=3, noise_px=1.0), 1234),
                'arprobot': (3, syn.FrameSpec(persons=3, noise_px=1.0), 1234)}[name]
        if name in RIG_FRAMES:
            frames, gts = zip(*[syn.make_frame(calib, i, spec[1], seed=spec[2]) for i in RIG_FRAMES[name]])
        else:
            frames, gts = syn.make_frames(calib, spec[0], spec[1], seed=spec[2])
        frames = [{c: list(v) for c, v in f.items()} for f in frames]
        owners = [{c: list(v) for c, v in g['owner'].items()} for g in gts]
        bodies = [np.asarray(g['persons'], np.float64) for g in gts]
        n_rows = [len(b) for b in bodies]
        F = len(frames)

        # what the case does to the frames themselves
        if name == 'stray':
            for f in range(F):
                drop_skeleton(frames[f], owners[f], names[f % V], f % 4)
        if name == 'noisy':
            keep_joints(frames[1], owners[1], names[2], 0, 2)             # stays in its row: unscored, kept
            keep_joints(frames[2], owners[2], names[3], 1, 2)             # taken out of its row: unscored, never attached
        if name == 'crowd':
            n_rows = [9, 9]                                               # body 9 has no row: its heads are free everywhere
            for f in range(F):
                drop_skeleton(frames[f], owners[f], names[1], 3)
                drop_skeleton(frames[f], owners[f], names[1], 4)
        if name == 'tie':
            duplicate_skeleton(frames[0], owners[0], names[1], 2)
        if name == 'arprobot':
            # two frames carry the two used streams only, the third all six; frame 0: body 2 has no row and body 1 is
            # missing from the first camera
            frames = [{c: v for c, v in fr.items() if c in cams or f == 2} for f, fr in enumerate(frames)]
            n_rows[0] = 2
            drop_skeleton(frames[0], owners[0], cams[0], 1)
        if name == 'degenerate':
            n_rows[0] = 0
            frames[1] = {names[2]: frames[1][names[2]]}
            owners[1] = {names[2]: owners[1][names[2]]}
            frames[2], _ = syn.make_frame(calib, 2, syn.FrameSpec(persons=3, empty_cameras=names), seed=spec[2])
            owners[2] = {c: [] for c in names}

        self.frames, self.owners, self.bodies = frames, owners, bodies
        self.processed = [onp.processed_input(f) for f in frames]
        if name == 'explicit':
            # heads in person order, a handful of edge-nodes of its own, no slot tables
            heads, pairs = [], []
            for o in range(n_rows[0]):
                for cam in cams:
                    if o in owners[0][cam]:
                        i = owners[0][cam].index(o)
                        heads.append((cam, i, json.loads(frames[0][cam][0])[i]))
            pairs = [(a, b) for a in range(4) for b in range(4, 8) if heads[a][0] != heads[b][0]]
            self.pb = pkg('packing').pack_scenes([{'heads': heads, 'pairs': np.array(pairs, np.int32)}], params)
            assert self.pb.en_pair is not None and (np.asarray(self.pb.slot_cam) == -1).all()
            assert self.pb.head_cam[0] != self.pb.head_cam[1]                 # not grouped by camera
        else:
            self.pb = pkg('packing').pack_frames(self.processed, params)
        pb = self.pb
        self.most = max([1] + [f[c][0].count('{') for f in self.processed for c in f])
        if pcap is None:
            pcap = max(n_rows + [1]) + (2 if name == 'degenerate' else 1)
        assert pcap > max(n_rows)
        self.pcap = pcap
        self.n_persons = np.asarray(n_rows, np.int32)
        self.true = rows_from_owners(pb, owners, n_rows, pcap, cams)
        self.rows = rows = self.true.copy()
        want = self.true.copy()
        self.want = {'triang': want, 'est': want}

        # the poses: the bodies themselves
        self.truth = np.zeros((F, pcap, J, 3))
        for f, b in enumerate(bodies):
            self.truth[f, :n_rows[f]] = b[:n_rows[f]]
        self.jflags = np.zeros((F, pcap, J), np.uint8)
        self.pflags = np.zeros((F, pcap), np.uint8)
        for f in range(F):
            self.jflags[f, :n_rows[f]] = 1
            self.pflags[f, :n_rows[f]] = 1
        if name in ('noisy', 'degenerate', 'arplab'):
            f, p, j = np.meshgrid(np.arange(F), np.arange(pcap), np.arange(J), indexing='ij')
            self.jflags[(f + 2 * p + j) % 7 == 0] = 0                     # joints the triangulation did not give

        # what the case does to the rows, and the rows it expects
        if name in ('swap', 'noisy'):
            for f in range(F):
                swap(rows, f, f % V, f % 3, (f % 3) + 1)
        if name == 'orphan':
            for f in range(F):
                for p in range(n_rows[f]):
                    orphan(rows, f, p, (f + p + 2) % V)
        if name == 'arplab':
            # not every camera of this rig sees every person: the first camera that holds both, the next that holds one
            for f in range(F):
                both = [c for c in range(V) if rows[f, 0, c] >= 0 and rows[f, 1, c] >= 0][f % 2]
                swap(rows, f, both, 0, 1)
                for p in range(n_rows[f]):
                    orphan(rows, f, p, [c for c in range(V) if c != both and rows[f, p, c] >= 0][0])
        if name == 'ring23':
            # the attach phase runs one wave per camera, cameras beyond the kernel's wave count taking turns (4 waves:
            # RG_WAVES = RG_THREADS / 64 in csrc/regroup.hip, camera c += RG_WAVES): frame f orphans person 2 in cameras
            # f + 1 and f + 5 (4 apart: one wave serves both -- were RG_THREADS to change, the pair would have to follow) and
            # person f % 2 in camera 22, and swaps persons 0 and 1 in camera 18 + f
            for f in range(F):
                swap(rows, f, 18 + f, 0, 1)
                orphan(rows, f, 2, f + 1)
                orphan(rows, f, 2, f + 5)
                orphan(rows, f, f % 2, 22)
        if name == 'arprobot':
            # frame 0: row 1 holds body 2's head in the first camera -- released, and nothing fits in its place, so the
            # row is left with one view; frames 1 and 2: a swap
            assert rows[0, 1, 0] == -1
            h0, H, _, _ = pb.frame_counts(0)
            rows[0, 1, 0] = [i for i in range(H) if pb.head_cam[h0 + i] == 0 and owners[0][cams[0]][int(pb.skeleton_index[h0 + i])] == 2][0]
            for f in (1, 2):
                swap(rows, f, f % V, 0, 1)
        if name == 'noisy':
            for f in range(F):
                orphan(rows, f, 3, (f + 1) % V)
            orphan(rows, 2, 1, 3)
            want[2, 1, 3] = -1
        if name == 'stray':
            self.strays = []
            for f in range(F):
                c = f % V
                h0, H, _, _ = pb.frame_counts(f)
                stray = [i for i in range(H) if pb.head_cam[h0 + i] == c and owners[f][cams[c]][int(pb.skeleton_index[h0 + i])] < 0]
                assert len(stray) == 1 and rows[f, f % 4, c] == -1
                rows[f, f % 4, c] = stray[0]
                self.strays.append(stray[0])
        if name == 'crowd':
            for f in range(F):
                for p in (0, 1, 2):
                    orphan(rows, f, p, 0)                                 # camera 0: four free heads, three open persons
                orphan(rows, f, 5, 1)                                     # camera 1: two free heads, three open persons
                swap(rows, f, 2, 6, 7)
                swap(rows, f, 3, 0, 8)
        if name == 'tie':
            orphan(rows, 0, 2, 1)
        if name == 'degenerate':
            # frame 3: row 0 holds row 1's head in camera 1; row 0 has no person flag (kind est)
            rows[3, 0, 1], rows[3, 1, 1] = self.true[3, 1, 1], -1
            self.want = {'triang': want, 'est': want.copy()}
            self.want['est'][3] = rows[3]
            self.pflags[3, 0] = 0
            self.truth[4, 0, 3] = np.nan                                  # frame 4: a joint that is not a number
            self.truth[5, 1] = behind_camera(calib, 2).astype(np.float64)  # frame 5: a pose behind camera 2
            T = pkg('harness.reprojection').engine_calibration(calib)[0]
            self.behind = [bool(T[c, 2, :3] @ self.truth[5, 1, 0] + T[c, 2, 3] <= 0.0) for c in range(V)]
            for c in range(V):
                if not self.behind[c]:
                    want[5, 1, c] = self.want['est'][5, 1, c] = -1
        if name == 'bad_rows':
            for f in range(F):
                swap(rows, f, f % V, 0, 1)
            want[[0, 2, 3]] = -2                                          # set below, once the bad entries are in
            rows[0, 2, 1] = rows[0, 2, 3]                                 # a head of camera 3 under column 1
            rows[2, 3, 4] = rows[2, 2, 4]                                 # two rows name one head
            rows[3, 1, 0] = pb.frame_counts(3)[1]                         # one past the frame's heads
            want[[0, 2, 3]] = rows[[0, 2, 3]]
        if name == 'explicit':
            swap(rows, 0, 1, 0, 2)
            orphan(rows, 0, 3, 4)
        self.est = self.truth.astype(np.float32)
        self._out = {}
        self.check()

    def kinds(self):
        """{kind: (poses, flags, joint mask)} as Engine.regroup / harness.regroup take them."""
        return {'triang': (self.truth, self.jflags, (1 << J) - 1),
                'est': (self.est, self.pflags, sum(1 << j for j in self.params.used_joints))}

    def statement(self, kind, rows=None, **opts):
        """harness.regroup.regroup on the case (cached for the case's own rows)."""
        poses, flags, mask = self.kinds()[kind]
        opts.setdefault('joint_mask', mask)
        key = (kind,) + tuple(sorted(opts.items()))
        if rows is not None:
            return pkg('harness.regroup').regroup(self.calib, self.pb, rows, self.n_persons, poses, flags, **opts)
        if key not in self._out:
            self._out[key] = pkg('harness.regroup').regroup(self.calib, self.pb, self.rows, self.n_persons, poses, flags, **opts)
        return self._out[key]

    def check(self):
        """The branches the case is there for, by the statement's diagnostics (default options)."""
        RG = pkg('harness.regroup')
        name, pb = self.name, self.pb
        out = {k: self.statement(k) for k in ('triang', 'est')}
        for kind, o in out.items():
            if name in RESTORED:
                assert np.array_equal(o['persons'], self.want[kind]), (name, kind, 'the statement does not restore the rows')
            assert (o['cost'][o['cost'] != -1.0] >= 0.0).all() and np.isfinite(o['cost']).all()
        o = out['triang']
        poses, flags, mask = self.kinds()['triang']
        cost, n = RG.cost_table(self.calib, pb, poses, flags, self.n_persons, mask, counts=True)
        if name == 'clean':
            assert pb.n_frames == 17 and pb.max_heads_per_frame() == 20 and not o['change'].any()
        if name == 'swap':
            assert (o['counts'][:, :2] == 2).all() and ((o['change'] == 3).sum(axis=(1, 2)) == 2).all()
        if name == 'orphan':
            assert set(np.unique(o['change'])) == {0, 2} and (o['counts'][:, 1] == 4).all() and not o['counts'][:, 0].any()
        if name == 'noisy':
            assert ((n > 0) & (n < 3)).any() and (cost[(n > 0) & (n < 3)] == -1.0).all()
            h = int(pb.frame_head_off[1]) + int(self.true[1, 0, 2])
            assert 0 < n[h, 0] < 3 and o['persons'][1, 0, 2] == self.true[1, 0, 2]
            h = int(pb.frame_head_off[2]) + int(self.true[2, 1, 3])
            assert 0 < n[h, 1] < 3 and o['persons'][2, 1, 3] == -1 and o['counts'][2, 2] >= 1
        if name == 'crowd':
            assert pb.n_frames == 2 and pb.max_heads_per_frame() == 48 and pb.max_heads_per_frame() * self.pcap > 256
            assert (o['counts'][:, 2] == 5).all()                         # body 9's heads stay free
        if name == 'degenerate':
            assert self.behind[2] and not all(self.behind)
            h0, H, _, _ = pb.frame_counts(4)
            assert (n[h0:h0 + H, 0] < n[h0:h0 + H, 1:3].max(axis=1)).any()
        if name == 'explicit':
            assert o['counts'][0].tolist()[:2] == [2, 3]
        if name == 'arplab':
            assert pb.V == 6 and (o['counts'][:, 0] == 2).all() and (o['counts'][:, 1] == 5).all()
        if name == 'ring23':
            assert pb.V == 23 and pb.max_heads_per_frame() == 69 and pb.max_heads_per_frame() * self.pcap > 256
            assert (o['counts'][:, 0] == 2).all() and (o['counts'][:, 1] == 5).all() and not o['status'].any()
            for f in range(pb.n_frames):
                assert o['change'][f, 0, 18 + f] == 3 and o['change'][f, 2, f + 1] == 2 and o['change'][f, 2, f + 5] == 2
                assert o['change'][f, f % 2, 22] == 2
        if name == 'arprobot':
            assert pb.V == 2 and [len(f) for f in self.frames] == [2, 2, 6] and not o['status'].any()
            assert o['counts'][0].tolist() == [1, 0, 2, 1] and o['n_views'][0, 1] == 1        # one view left, under min_views
            assert (o['counts'][1:, :2] == 2).all() and not o['counts'][1:, 2:].any()


def case(name, pcap=None):
    """The case, with its own row capacity or (for an engine's tensors) the one given."""
    if (name, pcap) not in _made:
        _made[name, pcap] = Case(name, pcap)
    return _made[name, pcap]


# ---- the end-to-end input: the `messy` batch of geom_cases, matched by ray distance and triangulated ---------------------------

def partition_of(rows, n):
    """The rows of a frame as a set of frozensets of heads, rows with fewer than two heads left out."""
    groups = [frozenset(int(h) for h in rows[p] if h >= 0) for p in range(int(n))]
    return {g for g in groups if len(g) >= 2}


def entries_right(c, f, rows, n):
    """Filled (person, camera) entries of frame f whose head belongs to the body most of the row's heads belong to."""
    pb = c.pb
    cams = list(c.params.used_cameras_skeleton_matching)
    h0 = int(pb.frame_head_off[f])
    right = 0
    for p in range(int(n)):
        own = [c.owners[f][cams[int(pb.head_cam[h0 + h])]][int(pb.skeleton_index[h0 + h])] for h in rows[p] if h >= 0]
        real = [o for o in own if o >= 0]
        if real:
            top = max(set(real), key=lambda o: (real.count(o), -o))
            right += sum(o == top for o in own)
    return right


def quality(c, rows, n_persons):
    """-> (frames whose partition is the true one, filled entries that are right) over the batch of geom case c."""
    import geom_cases as gc
    frames = sum(partition_of(rows[f], n_persons[f]) == gc.true_partition(c, f) for f in range(c.pb.n_frames))
    return frames, sum(entries_right(c, f, rows[f], n_persons[f]) for f in range(c.pb.n_frames))


def messy_on_cpu(pcap=None):
    """The `messy` case of geom_cases through the oracle's clustering (on the statement's ray scores) and the oracle's
    triangulation -> (geom case, rows [F,pcap,V], n_persons [F], poses [F,pcap,J,3] f64, joint flags [F,pcap,J])."""
    import geom_cases as gc
    onp = oracle()
    c = gc.case('messy')
    cams = list(c.params.used_cameras_skeleton_matching)
    found = gc.oracle_persons(c, c.statement()['scores'])
    pb = pkg('packing').pack_frames(c.processed, c.params, keep_json=True)
    F = pb.n_frames
    pcap = pcap if pcap is not None else max(len(p) for p in found) + 1
    rows = np.full((F, pcap, pb.V), -1, np.int32)
    poses, jv = np.zeros((F, pcap, J, 3)), np.zeros((F, pcap, J), np.uint8)
    for f in range(F):
        for p, row in enumerate(found[f]):
            rows[f, p] = row
            skels = {cams[k]: pb.jsons_for_head[f][int(h)] for k, h in enumerate(row) if h >= 0}
            for j, xyz in onp.triangulate_person(skels, c.calib, all_joints=True).items():
                poses[f, p, j], jv[f, p, j] = xyz, 1
    return c, rows, np.array([len(p) for p in found], np.int32), poses, jv
