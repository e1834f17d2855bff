"""Inputs for the time-lag tests (test_lag_host.py: harness/lag.py and csrc/lag_pick.h on their own; test_gpu_lag.py:
mpe_lag_* against them).  Scenes are bodies on seeded walks (synthetic.lagged_recording), every camera seeing them at its
own time; persons and track ids come from the generator's ownership, so neither file needs a matcher or a tracker.
Everything is seeded.  Not a test module."""
import copy

import numpy as np

from calib_cases import ALL_JOINTS, J, same_bits  # noqa: F401  (the tests take them from here)
from conftest import env, oracle, pkg


def LG():
    return pkg('harness.lag')


class Scene:
    """A recording of a rig (`variant`: a fixture variant of conftest.env) whose cameras lag by `lags` frames, packed as one
    batch, with its persons and the table: the true bodies at the integer frames as float64 poses with joint flags
    ('triang') and as float32 poses with row flags ('est'), track id = body.  exact: the detections are the rule's own
    projection (harness.refine.project64) of the bodies each camera saw, to the last bit.  permute: the body of row p
    changes from frame to frame (a seeded permutation of the rows per frame)."""

    def __init__(self, variant, n_frames, lags, n_bodies=2, seed=5100, pcap=None, weave=0.0, exact=True, permute=False, step=0.03):
        syn, onp = pkg('synthetic'), oracle()
        self.variant, self.env = variant, env(variant)
        self.calib = calib = self.env.calib
        self.names = list(calib.params.used_cameras_skeleton_matching)
        self.lags = list(lags)
        self.frames, self.owners, self.bodies, self.seen = syn.lagged_recording(calib, n_frames, lags, n_bodies, seed, step, weave)
        self.processed = [onp.processed_input(f) for f in self.frames]
        self.pb = pkg('packing').pack_frames(self.processed, calib.params, keep_json=True)
        F, P = n_frames, n_bodies
        self.pcap = pcap if pcap is not None else P + 1
        rng = np.random.default_rng(seed + 3)
        self.row_of = np.stack([rng.permutation(P) if permute else np.arange(P) for _ in range(F)])      # [F,P]: the row of body b
        self.persons = np.full((F, self.pcap, self.pb.V), -1, np.int32)
        for f in range(F):
            h0, H, _, _ = self.pb.frame_counts(f)
            for i in range(H):
                c = int(self.pb.head_cam[h0 + i])
                b = self.owners[f][self.names[c]][int(self.pb.skeleton_index[h0 + i])]
                self.persons[f, self.row_of[f, b], c] = i
        self.n_persons = np.full(F, P, np.int32)
        self.truth = np.zeros((F, self.pcap, J, 3))
        self.ids = np.full((F, self.pcap), -1, np.int32)
        for f in range(F):
            self.truth[f, self.row_of[f]] = self.bodies[f]
            self.ids[f, self.row_of[f]] = np.arange(P)
        self.flags = np.zeros((F, self.pcap, J), np.uint8)
        self.flags[:, :P] = 1
        if exact:
            self.pb = self.with_detections()
        used = sum(1 << j for j in calib.params.used_joints)
        self.kinds = {'triang': (self.truth, self.flags, ALL_JOINTS),
                      'est': (self.truth.astype(np.float32), np.ascontiguousarray(self.flags[:, :, 0]), used)}

    def with_detections(self):
        """A copy of the batch whose detections are the rule's own projection of the bodies each camera saw."""
        RF = pkg('harness.refine')
        T = pkg('harness.reprojection').engine_calibration(self.calib)[0]
        _, kd, K = RF.camera_constants64(self.calib)
        pb = copy.copy(self.pb)
        pb.xy = np.array(self.pb.xy, np.float64, copy=True)
        for f in range(pb.n_frames):
            h0, H, _, _ = pb.frame_counts(f)
            for i in range(H):
                c = int(pb.head_cam[h0 + i])
                b = self.owners[f][self.names[c]][int(pb.skeleton_index[h0 + i])]
                X = self.seen[self.names[c]][f][b]
                p = RF.project64(T[c], kd[c], K[c], X[:, 0], X[:, 1], X[:, 2])
                pb.xy[h0 + i, :, 0], pb.xy[h0 + i, :, 1] = p['px'], p['py']
        return pb

    def sub_batch(self, a, b):
        """Frames [a, b) packed on their own, with this scene's detections."""
        sub = pkg('packing').pack_frames(self.processed[a:b], self.calib.params, keep_json=True)
        h0, h1 = int(self.pb.frame_head_off[a]), int(self.pb.frame_head_off[b])
        sub = copy.copy(sub)
        sub.xy = np.array(np.asarray(self.pb.xy, np.float64).reshape(-1, J, 2)[h0:h1], copy=True).reshape(np.asarray(sub.xy).shape)
        return sub

    def one_pass(self, window, sub, kind='triang', huber_px=0.0, frames=None, sums=None, table=None):
        """lag_pass_host over the scene, or over the frames [a, b) of it packed on their own, against the whole table (or
        `table` = (poses, flags, n_persons, ids))."""
        poses, flags, mask = self.kinds[kind]
        tab = (poses, flags, self.n_persons, self.ids) if table is None else table
        a, b = (0, self.pb.n_frames) if frames is None else frames
        pb = self.pb if frames is None else self.sub_batch(a, b)
        return LG().lag_pass_host(self.calib, pb, a, self.persons[a:b], *tab, window, sub, huber_px, sums=sums, joint_mask=mask)


def messy(variant, n_frames, lags, n_bodies=3, seed=5300, pcap=None, weave=0.04):
    """A scene whose table has the rows that can go wrong (frames counted from the middle m of the recording): the rows
    permuted from frame to frame; body 0 absent from frame m (id -1: every window that holds m loses the track); a duplicate
    id in frame m + 2 (the unused row below takes body 1's id and other coordinates: the lowest row stays the track's);
    n_persons negative in frame 1 and far above pcap in frame 2; a NaN coordinate of body 1 in frame m - 2, where no camera
    observes body 1 (so only the neighbours' windows meet it); a joint of body 2 behind the third camera in frame m + 1
    (skipped at the entries that touch it); and for 'triang' about 5 % of the joint flags dropped, for 'est' one row flag."""
    s = Scene(variant, n_frames, lags, n_bodies, seed=seed, pcap=pcap if pcap is not None else n_bodies + 2, weave=weave, permute=True)
    m, P = n_frames // 2, n_bodies
    assert s.pcap >= P + 1 and n_frames >= 8
    row = lambda f, b: int(s.row_of[f, b])                   # noqa: E731
    T = pkg('harness.reprojection').engine_calibration(s.calib)[0]
    c = 2 % len(T)
    behind = -T[c][:, :3].T @ T[c][:, 3] - T[c][2, :3]       # one metre behind camera c
    rng = np.random.default_rng(seed + 11)
    tri, jf = s.truth.copy(), s.flags.copy()
    ids, n_persons, persons = s.ids.copy(), s.n_persons.copy(), s.persons.copy()
    ids[m, row(m, 0)] = -1
    ids[m + 2, P] = 1
    tri[m + 2, P] = tri[m + 2, row(m + 2, 1)] + 0.5
    jf[m + 2, P] = 1
    n_persons[m + 2] = P + 1
    n_persons[1], n_persons[2] = -2, s.pcap + 40
    persons[m - 2, row(m - 2, 1)] = -1
    tri[m - 2, row(m - 2, 1), 4, 1] = np.nan
    tri[m + 1, row(m + 1, 2), 9] = behind
    est = tri.astype(np.float32)
    pf = np.ascontiguousarray(jf[:, :, 0])
    pf[m - 1, row(m - 1, 2)] = 0
    jf = np.where(rng.uniform(size=jf.shape) < 0.05, 0, jf).astype(np.uint8)
    used = sum(1 << j for j in s.calib.params.used_joints)
    s.persons, s.ids, s.n_persons = persons, ids, n_persons
    s.kinds = {'triang': (tri, jf, ALL_JOINTS), 'est': (est, pf, used)}
    return s


ALTERNATION = dict(variant='panoptic', n_frames=24, lags=(0, 2, -1, 0, 1), window=3, sub=4, seed=5200, weave=0.05)


def alternate_host(variant, n_frames, lags, window, sub, seed, weave, rounds=4, min_obs=50, pass_fn=None):
    """The script's alternation by the numpy route alone: per round the recording re-paired by the shifts so far, persons
    and ids by ownership, poses by the oracle's triangulation (all joints) of the desynchronised detections themselves,
    one pass of the statement, the estimate, and the integer parts relative to the first camera applied.
    It stops after the round that applies nothing.  pass_fn(calib, pb, persons, poses, flags, n_persons, ids) -> sums
    replaces the statement's pass.  -> [the shifts each round applied], the total."""
    syn, onp, lag = pkg('synthetic'), oracle(), LG()
    calib = env(variant).calib
    names = list(calib.params.used_cameras_skeleton_matching)
    frames, owners, bodies, _ = syn.lagged_recording(calib, n_frames, lags, 2, seed, weave=weave)
    P, pcap = bodies.shape[1], bodies.shape[1] + 1
    total, applied = [0] * len(names), []
    for _ in range(rounds):
        cur, own = lag.retime_frames(frames, names, total), lag.retime_frames(owners, names, total)
        pb = pkg('packing').pack_frames([onp.processed_input(f) for f in cur], calib.params, keep_json=True)
        persons = np.full((n_frames, pcap, pb.V), -1, np.int32)
        poses, flags = np.zeros((n_frames, pcap, J, 3)), np.zeros((n_frames, pcap, J), np.uint8)
        for f in range(n_frames):
            h0, H, _, _ = pb.frame_counts(f)
            for i in range(H):
                c = int(pb.head_cam[h0 + i])
                persons[f, own[f][names[c]][int(pb.skeleton_index[h0 + i])], c] = i
            for b in range(P):
                skels = {names[c]: pb.jsons_for_head[f][int(h)] for c, h in enumerate(persons[f, b]) if h >= 0}
                if len(skels) >= 2:
                    for j, xyz in onp.triangulate_person(skels, calib, all_joints=True).items():
                        poses[f, b, j], flags[f, b, j] = xyz, 1
        ids = np.where(np.arange(pcap)[None, :] < P, np.arange(pcap)[None, :], -1).astype(np.int32).repeat(n_frames, axis=0)
        n_persons = np.full(n_frames, P, np.int32)
        if pass_fn is None:
            sums = lag.lag_pass_host(calib, pb, 0, persons, poses, flags, n_persons, ids, window, sub)
        else:
            sums = pass_fn(calib, pb, persons, poses, flags, n_persons, ids)
        rep = lag.lag_estimate_host(sums, window, sub, min_obs)
        shifts = lag.relative_shifts(rep['lag_refined'], 0)
        applied.append(shifts)
        total = [a + b for a, b in zip(total, shifts)]
        if not any(shifts):
            break
    return applied, total


def true_k(scene, sub):
    """The grid index (signed) of every camera's true lag; only for lags on the grid."""
    k = [lag * sub for lag in scene.lags]
    assert all(float(x).is_integer() for x in k)
    return [int(x) for x in k]


def curves():
    """Hand-made cost curves for the pick: (name, cost [K], n_obs [K], window, sub, min_obs)."""
    nan, inf = float('nan'), float('inf')
    par = [float((i - 5) ** 2 + 3) for i in range(9)]
    out = [
        ('parabola', par, [10] * 9, 2, 2, 5),
        ('skewed', [9.0, 4.0, 1.5, 1.0, 2.5, 7.0, 12.0], [7, 9, 11, 13, 11, 9, 7], 3, 1, 5),
        ('edge low', [1.0, 2.0, 3.0, 4.0, 5.0], [10] * 5, 2, 1, 5),
        ('edge high', [5.0, 4.0, 3.0, 2.0, 1.0], [10] * 5, 1, 2, 5),
        ('flat', [2.0] * 7, [4] * 7, 3, 1, 1),
        ('tie', [5.0, 1.0, 5.0, 1.0, 5.0], [10] * 5, 2, 1, 5),
        ('nan entries', [nan, 3.0, nan, 2.0, 2.5, nan, 1.0], [10] * 7, 3, 1, 5),
        ('nan neighbour', [4.0, nan, 1.0, 3.0, 5.0], [10] * 5, 2, 1, 5),
        ('all nan', [nan] * 5, [10] * 5, 2, 1, 5),
        ('inf neighbours', [inf, 1.0, inf], [10] * 3, 1, 1, 5),
        ('invalid neighbour', [9.0, 4.0, 1.0, 4.0, 9.0], [10, 10, 10, 4, 10], 2, 1, 5),
        ('invalid zero', [9.0, 1.0, 0.0, 4.0, 9.0], [10, 10, 4, 10, 10], 2, 1, 5),
        ('few', [1.0, 2.0, 3.0], [4, 4, 4], 1, 1, 5),
        ('one entry', [3.0], [6], 0, 1, 5),
        ('half step', [9.0, 1.0, 1.0], [1, 1, 1], 1, 1, 1),
        ('thirds', [8.0, 5.0, 1.0, 0.5, 3.0, 6.0, 9.0], [3, 3, 3, 3, 3, 3, 3], 1, 3, 3),
    ]
    return out
