"""Inputs for the refinement tests (test_refine_host.py: harness/refine.py on its own; test_gpu_refine.py: mpe_refine_batch
against it).  The batches follow the recipes of the reprojection tests; persons come from the generator's ground-truth
pairing, so neither file needs the matching network.  Not a test module."""
import json

import numpy as np

from conftest import env, oracle, pkg

J = 18
NAMES = ('messy', '5x10', 'one frame', 'zero frames', 'hand made', 'ring23', 'arprobot')
RIGS = ('ring23', 'arprobot')                    # cases on a rig of their own (conftest.env(name)); every other case is PANOPTIC's
# Engine arguments a case needs.  ring23: 3 x 23 = 69 heads a frame fit in 70, which gives Pcap = 70 // 2 = 35 rows -- odd, and
# 3 frames x 35 rows = 105 is no multiple of 8, so the last workgroup of refine / reproject has idle half-waves
ENGINE = {'ring23': dict(max_heads_per_frame=70)}
# generator frames (seed 1234) of 3 persons whose every joint lies in every used image of the rig: the case modules of all
# stages build their rig cases from these
RIG_FRAMES = {'ring23': (5200, 5201, 5203), 'arprobot': (5304, 5316, 5322)}


def variant_of(name):
    return name if name in RIGS else 'panoptic'


def same_bits(a, b):
    """Bit-equal, NaN matching NaN."""
    a, b = np.asarray(a), np.asarray(b)
    if a.dtype != b.dtype or a.shape != b.shape:
        return False
    if a.dtype.kind != 'f':
        return np.array_equal(a, b)
    nan = np.isnan(a)
    u = {4: np.int32, 8: np.int64}[a.dtype.itemsize]
    return np.array_equal(nan, np.isnan(b)) and np.array_equal(a[~nan].view(u), b[~nan].view(u))


def damaged(frames):
    """Cameras missing and detections that must not count: valid at 0.5, below it, just above it; a joint removed."""
    out = []
    for i, fr in enumerate(frames):
        fr = {c: list(v) for c, v in fr.items()}
        if i % 3 == 0:
            del fr[list(fr)[i % len(fr)]]
        for k, c in enumerate(fr):
            sks = json.loads(fr[c][0])
            for s, sk in enumerate(sks):
                keys = [q for q in sk if q != 'ID']
                for n, q in enumerate(keys):
                    if (n + s + k + i) % 4 == 0:
                        sk[q][3] = [0.5, 0.0, 0.25, 0.5000001, 0.75][(n + i) % 5]
                if keys and (s + i) % 2 == 0:
                    del sk[keys[(s + k) % len(keys)]]
            fr[c][0] = json.dumps(sks)
        out.append(fr)
    return out


def only_seen_by(frame, owner, person, cams):
    """The skeletons of `person` removed from every camera not in `cams` (frame and owner lists, in place)."""
    for cam in frame:
        if cam in cams or person not in owner[cam]:
            continue
        i = owner[cam].index(person)
        sks = json.loads(frame[cam][0])
        del sks[i]
        del owner[cam][i]
        frame[cam][0] = json.dumps(sks)


def hand_made_bodies():
    shape = np.stack([0.05 * np.cos(np.arange(J)), -0.08 * np.arange(J), 0.05 * np.sin(np.arange(J))], axis=1)
    return np.stack([shape + np.array(at) for at in ((-0.5, -0.2, 0.2), (0.4, -0.2, -0.3), (0.0, -0.2, 0.8), (0.8, -0.2, 0.6))])


def raw(name, seed=300):
    """-> (frames in wire format, per frame {camera: person of every skeleton}, per frame the bodies [P,J,3])."""
    syn, calib = pkg('synthetic'), env(variant_of(name)).calib
    if name == 'zero frames':
        return [], [], []
    if name == 'hand made':
        # person 0 in one camera only, person 1 in exactly two, persons 2 and 3 everywhere
        bodies = hand_made_bodies()
        cams = list(calib.params.camera_names)
        frame, owner = syn.frame_from_bodies(calib, 0, bodies)
        only_seen_by(frame, owner, 0, cams[1:2])
        only_seen_by(frame, owner, 1, [cams[0], cams[3]])
        return [frame], [owner], [bodies]
    if name == 'ring23':
        # 23 cameras, 18 joints: cameras 18..22 sit in lanes that own no joint.  Frames 0 and 1: persons 0 and 1 in every
        # camera, person 2 in cameras 19 and 22 only; frame 2: person 1 in camera 22 only, person 2 in cameras 19 and 22
        cams = list(calib.params.camera_names)
        made = [syn.make_frame(calib, i, syn.FrameSpec(persons=3, noise_px=1.0)) for i in RIG_FRAMES[name]]
        for i, (frame, gt) in enumerate(made):
            only_seen_by(frame, gt['owner'], 2, [cams[19], cams[22]])
            if i == 2:
                only_seen_by(frame, gt['owner'], 1, [cams[22]])
        return [m[0] for m in made], [m[1]['owner'] for m in made], [m[1]['persons'] for m in made]
    if name == 'arprobot':
        # six cameras configured, the two robot cameras (calibration indices 4 and 5) used: two frames carry those two
        # streams only, the third all six (the packer drops the four it has no slot for)
        used = list(calib.params.used_cameras_skeleton_matching)
        made = [syn.make_frame(calib, i, syn.FrameSpec(persons=3, noise_px=1.0)) for i in RIG_FRAMES[name]]
        frames = [{c: v for c, v in m[0].items() if c in used or i == 2} for i, m in enumerate(made)]
        return frames, [m[1]['owner'] for m in made], [m[1]['persons'] for m in made]
    if name == 'messy':
        made = [syn.make_frame(calib, seed + i, syn.FrameSpec(persons=3 + i % 3, noise_px=2.0, joint_drop=0.1)) for i in range(12)]
        return damaged([m[0] for m in made]), [m[1]['owner'] for m in made], [m[1]['persons'] for m in made]
    if name == '5x10':
        made = [syn.make_frame(calib, 900 + i, syn.FrameSpec(persons=10, noise_px=1.0)) for i in range(8)]
    else:
        made = [syn.make_frame(calib, 77, syn.FrameSpec(persons=4, noise_px=1.0))]
    return [m[0] for m in made], [m[1]['owner'] for m in made], [m[1]['persons'] for m in made]


def persons_from_owners(pb, owners, n_bodies, pcap, variant='panoptic'):
    """persons [F,pcap,V] (frame-local head ids, -1 without one) and n_persons [F]: body o of a frame is row o."""
    sm = list(env(variant).calib.params.used_cameras_skeleton_matching)
    F = pb.n_frames
    persons = np.full((F, pcap, pb.V), -1, np.int32)
    for f in range(F):
        h0, H, _, _ = pb.frame_counts(f)
        for i in range(H):
            c = int(pb.head_cam[h0 + i])
            o = owners[f][sm[c]][int(pb.skeleton_index[h0 + i])]
            if o >= 0:
                persons[f, o, c] = i
    return persons, np.asarray(n_bodies, np.int32)


class Case:
    """One batch with its persons and two sets of starting poses: `est` (float32, person flags: the bodies moved by a
    few centimetres) and, on request, `tri` (float64, joint flags: the oracle's triangulation)."""

    def __init__(self, name, pcap=None, pb=None, seed=300):
        self.variant = variant_of(name)
        self.env = env(self.variant)
        onp, calib = oracle(), self.env.calib
        self.name, self.calib = name, calib
        self.frames, self.owners, bodies = raw(name, seed)
        self.processed = [onp.processed_input(f) for f in self.frames]
        self.pb = pb if pb is not None else pkg('packing').pack_frames(self.processed, calib.params, keep_json=True)
        F = len(self.frames)
        most = max([0] + [len(b) for b in bodies])
        self.pcap = pcap if pcap is not None else most + 1
        self.persons, self.n_persons = persons_from_owners(self.pb, self.owners, [len(b) for b in bodies], self.pcap, self.variant)
        self.truth = np.zeros((F, self.pcap, J, 3))
        for f, b in enumerate(bodies):
            self.truth[f, :len(b)] = b
        rng = np.random.default_rng(11)
        self.est = (self.truth + rng.uniform(-0.03, 0.03, self.truth.shape)).astype(np.float32)
        self.est_flags = (np.arange(self.pcap)[None, :] < self.n_persons[:, None]).astype(np.uint8)
        if F:
            self.est_flags[0, 0] = name == 'hand made'        # a person without its flag is not touched
        if name == 'hand made':
            self.est[0, 2, 8] = behind_camera(calib, 2)       # seen from everywhere, starts behind camera 2
        self._tri = None

    @property
    def tri(self):
        """(poses [F,pcap,J,3] float64, joint flags [F,pcap,J]) by the oracle's triangulation of reprojection_error."""
        if self._tri is None:
            onp, calib = oracle(), self.calib
            sm = list(calib.params.used_cameras_skeleton_matching)
            poses = np.zeros((len(self.frames), self.pcap, J, 3))
            jv = np.zeros((len(self.frames), self.pcap, J), np.uint8)
            for f in range(len(self.frames)):
                for p in range(int(self.n_persons[f])):
                    skels = {sm[c]: self.pb.jsons_for_head[f][int(self.persons[f, p, c])] for c in range(self.pb.V) if self.persons[f, p, c] >= 0}
                    for j, xyz in onp.triangulate_person(skels, calib, positive_ids_only=True, all_joints=True).items():
                        poses[f, p, j], jv[f, p, j] = xyz, 1
            if self.name == 'hand made':
                poses[0, 2, 8] = behind_camera(calib, 2).astype(np.float64)
            self._tri = poses, jv
        return self._tri


def behind_camera(calib, c):
    """A point one metre behind the camera of slot c, on its axis (float32-exact enough for both pose types)."""
    P = pkg('harness.reprojection').engine_calibration(calib)[0][c]
    centre = -P[:, :3].T @ P[:, 3]
    return (centre - P[2, :3]).astype(np.float32)


def kinds(case, tri=None):
    """{kind: (poses, flags, joint mask)} for Engine.refine / harness.refine: 'est' with the used joints, 'triang' with all."""
    params = case.calib.params
    tri = tri if tri is not None else case.tri
    return {'est': (case.est, case.est_flags, sum(1 << j for j in params.used_joints)),
            'triang': (tri[0], tri[1], (1 << J) - 1)}


def noise_free(case):
    """A copy of the case's batch whose detections are harness.refine.project64 of the bodies, exactly: the minimum of
    every joint's cost is the body's joint, at cost 0."""
    import copy
    RF, calib = pkg('harness.refine'), case.calib
    sm = list(calib.params.used_cameras_skeleton_matching)
    T, kd, K = RF.camera_constants64(calib)
    pb = copy.copy(case.pb)
    pb.xy = np.array(case.pb.xy, np.float64, copy=True)
    for f in range(pb.n_frames):
        h0, H, _, _ = pb.frame_counts(f)
        for i in range(H):
            c = int(pb.head_cam[h0 + i])
            o = case.owners[f][sm[c]][int(pb.skeleton_index[h0 + i])]
            p = RF.project64(T[c], kd[c], K[c], case.truth[f, o, :, 0], case.truth[f, o, :, 1], case.truth[f, o, :, 2])
            pb.xy[h0 + i, :, 0], pb.xy[h0 + i, :, 1] = p['px'], p['py']
    return pb


def head_of(case, f, person, c):
    """Index into the batch's per-head arrays of the skeleton camera c has for `person` in frame f."""
    return int(case.pb.frame_head_off[f]) + int(case.persons[f, person, c])


def check(case):
    """A rig case takes the branches it exists for; asserted on the CPU from the statement's own diagnostics (a condition
    on the seeds).  -> the numbers, for the tests to print."""
    R, RF = pkg('harness.reprojection'), pkg('harness.refine')
    F, V = len(case.frames), case.pb.V
    every = np.ones((F, case.pcap), np.uint8)
    sel, _ = R.selection(case.pb, case.persons, case.n_persons, every, (1 << J) - 1)
    views = sel.sum(axis=2)                                                           # [F, pcap, J]
    seen = sel.any(axis=3)                                                            # [F, pcap, V]
    out = RF.refine(case.calib, case.pb, case.persons, case.n_persons, case.truth, np.repeat(every[..., None], J, axis=2), (1 << J) - 1)
    assert np.array_equal(out['n_views'], views)
    res = R.residuals(case.calib, case.pb, case.persons, case.n_persons, case.truth, every, (1 << J) - 1)
    count = R.stats([res.reshape(-1, V, J)])['count']
    info = {'V': V, 'n_views': [views[f, :3].max(axis=1).tolist() for f in range(F)], 'count': count.tolist(),
            'status': sorted(set(out['status'][:, :3].reshape(-1).tolist()))}
    if case.name == 'ring23':
        assert V == 23 and F == 3 and case.n_persons.tolist() == [3, 3, 3]
        assert (views[:2, :2] == 23).all() and (views[2, 0] == 23).all()              # every joint, every camera
        assert (views[:, 2] == 2).all() and (seen[:, 2] == (np.isin(np.arange(V), (19, 22)))).all()   # lanes 19 and 22 own no joint
        assert (views[2, 1] == 1).all() and seen[2, 1].tolist() == [c == 22 for c in range(V)]
        assert (out['status'][2, 1] == RF.FEW_VIEWS).all() and (out['status'][:, 2] & RF.SOLVED).all()
        assert (count[18:] > 0).all() and len(count) == 23
        pcap = ENGINE['ring23']['max_heads_per_frame'] // case.calib.params.min_number_of_views
        assert pcap % 2 == 1 and (F * pcap) % 8 != 0
        info['pcap'] = pcap
    if case.name == 'arprobot':
        assert V == 2 and F == 3 and [len(f) for f in case.frames] == [2, 2, 6]
        assert R.engine_cameras(case.calib) == [4, 5]
        assert (views[:, :3] == 2).all() and (out['status'][:, :3] & RF.SOLVED).all()  # two views: the smallest solvable problem
        assert (count > 0).all() and len(count) == 2
    return info
