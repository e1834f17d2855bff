"""Inputs for the refinement tests (test_refine_host.py: harness/refine.py on its own; test_gpu_refine.py: mpe_refine_batch
against it).  The batches follow the recipes of the reprojection tests; persons come from the generator's ground-truth
pairing, so neither file needs the matching network.  Not a test module."""
import json

import numpy as np

from conftest import env, oracle, pkg

J = 18
NAMES = ('messy', '5x10', 'one frame', 'zero frames', 'hand made')


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
    syn, calib = pkg('synthetic'), env().calib
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
    if name == 'messy':
        made = [syn.make_frame(calib, seed + i, syn.FrameSpec(persons=3 + i % 3, noise_px=2.0, joint_drop=0.1)) for i in range(12)]
        return damaged([m[0] for m in made]), [m[1]['owner'] for m in made], [m[1]['persons'] for m in made]
    if name == '5x10':
        made = [syn.make_frame(calib, 900 + i, syn.FrameSpec(persons=10, noise_px=1.0)) for i in range(8)]
    else:
        made = [syn.make_frame(calib, 77, syn.FrameSpec(persons=4, noise_px=1.0))]
    return [m[0] for m in made], [m[1]['owner'] for m in made], [m[1]['persons'] for m in made]


def persons_from_owners(pb, owners, n_bodies, pcap):
    """persons [F,pcap,V] (frame-local head ids, -1 without one) and n_persons [F]: body o of a frame is row o."""
    sm = list(env().calib.params.used_cameras_skeleton_matching)
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
        onp, calib = oracle(), env().calib
        self.name = name
        self.frames, self.owners, bodies = raw(name, seed)
        self.processed = [onp.processed_input(f) for f in self.frames]
        self.pb = pb if pb is not None else pkg('packing').pack_frames(self.processed, calib.params, keep_json=True)
        F = len(self.frames)
        most = max([0] + [len(b) for b in bodies])
        self.pcap = pcap if pcap is not None else most + 1
        self.persons, self.n_persons = persons_from_owners(self.pb, self.owners, [len(b) for b in bodies], self.pcap)
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
            onp, calib = oracle(), env().calib
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
    """A point one metre behind camera c, on its axis (float32-exact enough for both pose types)."""
    P = np.asarray(calib.P[c], np.float64).reshape(3, 4)
    centre = -P[:, :3].T @ P[:, 3]
    return (centre - P[2, :3]).astype(np.float32)


def kinds(case, tri=None):
    """{kind: (poses, flags, joint mask)} for Engine.refine / harness.refine: 'est' with the used joints, 'triang' with all."""
    params = env().calib.params
    tri = tri if tri is not None else case.tri
    return {'est': (case.est, case.est_flags, sum(1 << j for j in params.used_joints)),
            'triang': (tri[0], tri[1], (1 << J) - 1)}


def noise_free(case):
    """A copy of the case's batch whose detections are harness.refine.project64 of the bodies, exactly: the minimum of
    every joint's cost is the body's joint, at cost 0."""
    import copy
    RF, calib = pkg('harness.refine'), env().calib
    sm = list(calib.params.used_cameras_skeleton_matching)
    T, kd, K = RF.camera_constants64(calib)
    pb = copy.copy(case.pb)
    pb.xy = np.array(case.pb.xy, np.float64, copy=True)
    for f in range(pb.n_frames):
        h0, H, _, _ = pb.frame_counts(f)
        for i in range(H):
            c = int(pb.head_cam[h0 + i])
            o = case.owners[f][sm[c]][int(pb.skeleton_index[h0 + i])]
            k = calib.index(sm[c])
            p = RF.project64(T[k], kd[k], K[k], case.truth[f, o, :, 0], case.truth[f, o, :, 1], case.truth[f, o, :, 2])
            pb.xy[h0 + i, :, 0], pb.xy[h0 + i, :, 1] = p['px'], p['py']
    return pb


def head_of(case, f, person, c):
    """Index into the batch's per-head arrays of the skeleton camera c has for `person` in frame f."""
    return int(case.pb.frame_head_off[f]) + int(case.persons[f, person, c])
