"""Inputs for the geometric-matching tests (test_geom_host.py: harness/geometric.py on its own; test_gpu_geom.py:
mpe_geom_scores_batch / mpe_geom_match_batch against it).  Built the way refine_cases.py builds its own; every case
asserts, with the statement's diagnostics, that the branch it is there for is really taken.  Not a test module."""
import copy
import json

import numpy as np

from conftest import env, oracle, pkg
from refine_cases import RIG_FRAMES, same_bits  # noqa: F401  (the GPU tests compare with it)

J = 18
NAMES = ('c1', 'clean', 'noisy', 'messy', 'far', '5x10', 'arplab', 'explicit', 'ring23', 'arprobot')
_made = {}


def option_sets(params):
    """The three option sets of the GPU tests: the defaults; no clip and three common joints; the used joints at confidence 0.6."""
    return [{}, {'clip': 0.0, 'min_joints': 3}, {'joint_mask': sum(1 << j for j in params.used_joints), 'min_conf': 0.6}]


def far_direction(calib):
    """A unit direction along which a point 1e8 m away is seen by two cameras whose rays to it come out parallel (the
    den < 1e-12 branch): the bisector of two optical axes, the first pair in camera order for which the statement says
    so."""
    syn, G, onp = pkg('synthetic'), pkg('harness.geometric'), oracle()
    P = np.asarray(calib.P, np.float64)
    for a in range(len(P)):
        for b in range(a + 1, len(P)):
            d = P[a, 2, :3] + P[b, 2, :3]
            d = d / np.linalg.norm(d)
            bodies = hand_body()
            bodies[0, 8] = d * 1e8
            frame, _ = syn.frame_from_bodies(calib, 0, bodies)
            if sum('"8"' in frame[c][0] for c in frame) >= 2:
                pb = pkg('packing').pack_frames([onp.processed_input(frame)], calib.params)
                if G.scores(calib, pb)['parallel'][:, 8].any():
                    return d
    raise AssertionError('no direction whose rays come out parallel')


def hand_body():
    return np.stack([0.05 * np.cos(np.arange(J)), -0.6 - 0.05 * np.arange(J), 0.05 * np.sin(np.arange(J))], axis=1)[None].copy()


def no_common_joint(frame):
    """The first skeleton of the first camera keeps its even joints, the first of the second camera its odd ones."""
    for k, cam in enumerate(list(frame)[:2]):
        sks = json.loads(frame[cam][0])
        i = [any(int(q) % 2 == k for q in sk) for sk in sks].index(True)
        sks[i] = {q: v for q, v in sks[i].items() if int(q) % 2 == k}
        frame[cam][0] = json.dumps(sks)


def raw(name):
    """-> (variant, frames in wire format, per frame {camera: person of every skeleton})."""
    syn = pkg('synthetic')
    variant = name if name in ('arplab', 'ring23', 'arprobot') else 'panoptic'
    calib = env(variant).calib
    cams = list(calib.params.camera_names)
    if name == 'c1':
        made = [syn.make_frame(calib, 0, syn.FrameSpec(persons=1, cameras=cams[:2]))]
    elif name in ('clean', 'noisy', 'explicit'):
        fr, gt = syn.make_frames(calib, 1 if name == 'explicit' else 17, syn.FrameSpec(persons=4, noise_px=2.0 if name == 'noisy' else 0.0), seed=1234)
        made = list(zip(fr, gt))
    elif name == 'messy':
        fr, gt = syn.make_frames(calib, 8, syn.FrameSpec(persons=4, noise_px=2.0, joint_drop=0.3, spurious=1), seed=1234)
        fr = [{c: list(v) for c, v in f.items()} for f in fr]
        no_common_joint(fr[0])
        fr[4] = {cams[2]: fr[4][cams[2]]}                    # a single camera: no edge-node, in the middle of the batch
        gt[4] = {'owner': {cams[2]: gt[4]['owner'][cams[2]]}}
        made = list(zip(fr, gt))
    elif name == 'far':
        bodies = hand_body()
        bodies[0, 8] = far_direction(calib) * 1e8
        frame, owner = syn.frame_from_bodies(calib, 0, bodies)
        made = [(frame, {'owner': owner})]
    elif name == '5x10':
        fr, gt = syn.make_frames(calib, 2, syn.FrameSpec(persons=10), seed=1234)
        made = list(zip(fr, gt))
    elif name in RIG_FRAMES:
        made = [syn.make_frame(calib, i, syn.FrameSpec(persons=3, noise_px=1.0), seed=1234) for i in RIG_FRAMES[name]]
        if name == 'arprobot':
            # two frames carry the two used streams only, the third all six (four of them without a slot)
            used = list(calib.params.used_cameras_skeleton_matching)
            made = [({c: v for c, v in fr.items() if c in used or i == 2}, gt) for i, (fr, gt) in enumerate(made)]
    else:
        fr, gt = syn.make_frames(calib, 4, syn.FrameSpec(persons=3, noise_px=1.0), seed=1234)
        made = list(zip(fr, gt))
    return variant, [m[0] for m in made], [m[1]['owner'] for m in made]


class Case:
    def __init__(self, name):
        onp = oracle()
        self.name = name
        self.variant, self.frames, self.owners = raw(name)
        self.env = env(self.variant)
        self.calib, self.params = self.env.calib, self.env.params
        self.processed = [onp.processed_input(f) for f in self.frames]
        self.pb = pkg('packing').pack_frames(self.processed, self.params)
        if name == 'explicit':
            # both orders of the first ten cross-camera pairs and one pair inside a camera
            pb = copy.copy(self.pb)
            first = np.asarray(self.pb.pairs(0), np.int32)[:10]
            assert pb.head_cam[0] == pb.head_cam[1]
            pb.en_pair = np.concatenate([first, first[:, ::-1], np.array([[0, 1]], np.int32)]).astype(np.int32)
            pb.frame_en_off = np.array([0, len(pb.en_pair)], np.int32)
            self.pb = pb
        self.most = max([1] + [f[c][0].count('{') for f in self.processed for c in f])
        self._want = {}
        self.check()

    def statement(self, **opts):
        key = tuple(sorted(opts.items()))
        if key not in self._want:
            self._want[key] = pkg('harness.geometric').scores(self.calib, self.pb, **opts)
        return self._want[key]

    def check(self):
        """The branches the case is there for, by the statement's diagnostics (default options)."""
        w = self.statement()
        name, pb = self.name, self.pb
        if name == 'c1':
            assert pb.n_edge_nodes == 1 and w['n_votes'][0] > 0
        if name in ('clean', 'noisy'):
            assert pb.n_frames == 17 and pb.max_heads_per_frame() == 20
        if name == 'messy':
            assert pb.frame_en_off[5] == pb.frame_en_off[4] and pb.frame_head_off[5] > pb.frame_head_off[4]
            pairs = pkg('harness.geometric').batch_pairs(pb)
            other_cam = pb.head_cam[pairs[:, 0]] != pb.head_cam[pairs[:, 1]]
            assert (other_cam & (w['n_votes'] == 0)).any() and np.all(w['mean'][w['n_votes'] == 0] == -1.0)
            assert w['clamped'].any()
        if name == 'far':
            assert w['parallel'].any() and not w['parallel'][:, [j for j in range(J) if j != 8]].any()
        if name == '5x10':
            assert pb.n_frames == 2 and pb.max_heads_per_frame() == 50
        if name == 'arplab':
            assert pb.V == 6 and pb.n_frames == 4 and w['n_votes'].max() > 0
        if name == 'ring23':
            # 69 heads a frame: 2277 edge-nodes, eight whole chunks of 256 and a partial one
            M = np.diff(np.asarray(pb.frame_en_off))
            assert pb.V == 23 and pb.max_heads_per_frame() == 69 and M.tolist() == [2277] * 3 and 2277 % 256 == 229
            assert (w['n_votes'] == J).all()
        if name == 'arprobot':
            pairs = pkg('harness.geometric').batch_pairs(pb)
            assert pb.V == 2 and [len(f) for f in self.frames] == [2, 2, 6] and np.diff(np.asarray(pb.frame_en_off)).tolist() == [9] * 3
            assert (pb.head_cam[pairs[:, 0]] == 0).all() and (pb.head_cam[pairs[:, 1]] == 1).all() and (w['n_votes'] == J).all()   # one camera pair
        if name == 'explicit':
            assert w['n_votes'][-1] == 0 and w['scores'][-1] == 0.0 and same_bits(w['scores'][:10], w['scores'][10:20])


def case(name):
    if name not in _made:
        _made[name] = Case(name)
    return _made[name]


def oracle_persons(c, scores, thr=0.5):
    """oracle_np.cluster frame by frame on `scores` -> per frame the list of persons (V head ids each, -1 without one)."""
    onp, pb = oracle(), c.pb
    out = []
    for f in range(pb.n_frames):
        h0, H, e0, M = pb.frame_counts(f)
        out.append(onp.cluster(scores[e0:e0 + M], np.asarray(pb.pairs(f)).reshape(-1, 2), H, pb.head_cam[h0:h0 + H], pb.V,
                               min_views=c.params.min_number_of_views, thr=thr) if M else [])
    return out


def true_partition(c, f):
    """The owners' partition of frame f: every person seen by at least two cameras, as a set of frozensets of frame-local heads."""
    pb = c.pb
    sm = list(c.params.used_cameras_skeleton_matching)
    h0, H, _, _ = pb.frame_counts(f)
    groups = {}
    for i in range(H):
        o = c.owners[f][sm[int(pb.head_cam[h0 + i])]][int(pb.skeleton_index[h0 + i])]
        if o >= 0:
            groups.setdefault(o, set()).add(i)
    return {frozenset(g) for g in groups.values() if len(g) >= 2}
