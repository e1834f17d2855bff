"""Inputs for the body-fit tests (test_skel_refine_host.py: harness/skeleton_refine.py on its own; test_gpu_skel_refine.py:
mpe_body_refine_batch against it, bit for bit).  Not a test module.

Batches, persons and bodies come from refine_cases (the generator's pairing: no matching network); the random tracked
sequence from smooth_cases.  In the known cases every (frame, row) is a track of its own -- the generator draws new bodies
per frame -- and the length table holds the lengths of the row's body."""
import copy

import numpy as np

import refine_cases as rc
import smooth_cases as smc
from conftest import env, pkg

J = rc.J
ALL = (1 << J) - 1
FILLED = 2                                   # MPE_SMOOTH_FILLED
_cache = {}


def mods():
    return pkg('harness.skeleton'), pkg('harness.skeleton_refine')


def base(name):
    """refine_cases.Case(name) and its noise-free batch, built once (a rig case with the row capacity of its engine)"""
    if name not in _cache:
        kw = rc.ENGINE.get(name)
        c = rc.Case(name, pcap=kw['max_heads_per_frame'] // env(rc.variant_of(name)).params.min_number_of_views if kw else None)
        _cache[name] = (c, rc.noise_free(c))
    return _cache[name]


def lengths_of(bodies, bones):
    """bodies [..., J, 3] float64 -> [..., n_bones] by the statement's length lines"""
    S = pkg('harness.skeleton')
    flat = np.asarray(bodies, np.float64).reshape(-1, J, 3)
    return np.array([[S._length(x, jp, jc)[1] for jp, jc in bones] for x in flat]).reshape(np.shape(bodies)[:-2] + (len(bones),))


class Seq:
    """What one call takes: the batch, the rows' heads, the pose rows, the frame map, and the state of the statement."""

    def __init__(self, pb, persons, n_persons, poses, flags, ids, state, mode, frames=None, joint_mask=ALL, truth=None, calib=None):
        self.calib = env().calib if calib is None else calib
        self.pb, self.persons, self.n_persons, self.poses, self.flags, self.ids = pb, persons, n_persons, poses, flags, ids
        self.state, self.mode, self.frames, self.joint_mask, self.truth = state, mode, frames, joint_mask, truth
        self.pcap = poses.shape[1]

    def run(self, **kw):
        SR = pkg('harness.skeleton_refine')
        return SR.refine_sequence(self.state, self.calib, self.pb, self.persons, self.n_persons, self.poses, self.flags, self.ids, self.mode,
                                  self.joint_mask, frames=self.frames, **kw)

    def cut(self, sl):
        """the pose frames of a slice, observed through a frame map into the whole batch"""
        frames = (np.arange(len(self.poses)) if self.frames is None else self.frames)[sl].astype(np.int32)
        return Seq(self.pb, self.persons[sl], self.n_persons[sl], self.poses[sl], self.flags[sl], self.ids[sl], self.state, self.mode, frames,
                   self.joint_mask, None if self.truth is None else self.truth[sl], self.calib)


def known(name, mode, exact=False, start='near', bones=None):
    """The batch `name` of refine_cases with every (frame, row) its own track and the table set from the bodies.  exact:
    the noise-free detections; start: 'near' (refine_cases' est, the bodies moved by up to 3 cm), 'truth' (the bodies)."""
    S, _ = mods()
    c, clean = base(name)
    bones = S.BONES_18 if bones is None else bones
    F, pcap = c.truth.shape[:2]
    tri = mode == 'tri'
    poses = (c.est.astype(np.float64) if start == 'near' else c.truth.copy()).astype(np.float64 if tri else np.float32)
    row = np.arange(pcap)[None, :] < c.n_persons[:, None]
    flags = (np.repeat(row[..., None], J, axis=2) if tri else row).astype(np.uint8)
    ids = np.where(row, np.arange(F * pcap).reshape(F, pcap), -1).astype(np.int32)
    st = S.new_state(max(F * pcap, 1), bones, 0.002, J)
    S.set_lengths(st, lengths_of(c.truth, st['bones']).reshape(F * pcap, -1))
    return Seq(clean if exact else c.pb, c.persons, c.n_persons, poses, flags, ids, st, mode, truth=c.truth, calib=c.calib)


def rig(name, mode):
    """known(name, mode) of a rig case of refine_cases ('ring23', 'arprobot': three frames, every (frame, row) a track) and
    what the statement must show on it -> (Seq, the numbers asserted)"""
    _, SR = mods()
    s = known(name, mode)
    c = base(name)[0]
    info = rc.check(c)
    ref = s.run(sweeps=4)
    nv, st = ref['n_views'], ref['status']
    assert [nv[f, :3].max(axis=1).tolist() for f in range(len(nv))] == info['n_views']
    info['rows'] = nv.shape[0] * nv.shape[1]
    if name == 'ring23':
        assert info['rows'] % 2 == 1                                             # two rows share a wave: the last row is alone
        assert (st[2, 1] & SR.ONE_VIEW).all() and not (st[:, 2] & SR.ONE_VIEW).any() and (st[:, :3] & SR.FREE).all()
    if name == 'arprobot':
        assert (nv[:, :3] == 2).all() and not (st & SR.ONE_VIEW).any() and (st[:, :3] & SR.FREE).all()
    assert (st & SR.MOVED).any() and (ref['n_bones'][:, :3] > 0).all()
    info['status'] = sorted(set(st[:, :3].reshape(-1).tolist()))
    return s, info


def spoiled(name, mode):
    """known(name, mode) with what a row can have wrong: a joint behind camera 2 (BAD_START), a NaN and an infinite
    coordinate, a track without lengths, an id over the table, a negative id, and in mode 'tri' two absent joints"""
    s = known(name, mode)
    s.poses[0, 1, 8] = rc.behind_camera(env().calib, 2)
    s.poses[1, 0, 5, 1] = np.nan
    s.poses[1, 1, 17, 0] = np.inf
    s.state['len'][s.ids[2, 0]] = 0.0
    s.state['len'][s.ids[2, 1], 3:] = (np.inf, -1.0, np.nan) * 5
    s.ids[3, 0] = s.state['tid_cap'] + 7
    s.ids[3, 1] = -1
    if mode == 'tri':
        s.flags[4, 0, [7, 11]] = 0
        s.flags[4, 1, 13] = FILLED
    return s


def camera_centre(c):
    """the centre of the camera of slot c"""
    P = pkg('harness.reprojection').engine_calibration(env().calib)[0][c]
    return -P[:, :3].T @ P[:, 3]


def one_view(offset=0.040):
    """'one frame', noise-free, mode 'tri', the bodies as the start.  Person k (k = 0..3): its elbow (7) and its knee (13)
    are left to one camera -- their `valid` in every other camera's skeleton is 0 -- and start `offset` metres off along
    that camera's ray, with the flag of a filled joint; person k takes the (k // 2)-th camera that sees both and the sign
    (-1)^k.  -> (Seq, [(person, joint, camera)])"""
    s = known('one frame', 'tri', exact=True, start='truth')
    pb = copy.copy(s.pb)
    pb.vp = np.array(s.pb.vp, np.float32, copy=True).reshape(-1, J, 2)
    where = []
    for k in range(int(s.n_persons[0])):
        case = base('one frame')[0]
        cams = [c for c in range(pb.V) if s.persons[0, k, c] >= 0]
        sees = [c for c in cams if all((int(pb.joint_mask[rc.head_of(case, 0, k, c)]) >> j) & 1 and pb.vp[rc.head_of(case, 0, k, c), j, 0] > 0.5
                                       for j in (7, 13))]
        cam = sees[k // 2]
        for j in (7, 13):
            for c in cams:
                if c != cam:
                    pb.vp[rc.head_of(case, 0, k, c), j, 0] = 0.0
            ray = s.truth[0, k, j] - camera_centre(cam)
            s.poses[0, k, j] = s.truth[0, k, j] + (-1.0) ** k * offset * ray / np.linalg.norm(ray)
            s.flags[0, k, j] = FILLED
            where.append((k, j, cam))
    pb.vp = pb.vp.reshape(np.shape(s.pb.vp))
    s.pb = pb
    return s, where


def random_tracked(tri, B=40, seed=40):
    """smooth_cases.random_sequence (births, deaths, gaps, non-finite coordinates, rows without a flag, empty frames; mode
    'tri': missing joints) observed in the '5x10' batch through a frame map that repeats, skips and reverses, the rows'
    heads drawn at random (some outside the frame's heads); lengths learned from the sequence itself, the table small
    enough that some ids are over it, joint 3 outside the mask."""
    S, _ = mods()
    c, _ = base('5x10')
    poses, flags, n_persons, ids = smc.random_sequence(seed + tri, tri, pkg('harness.tracking'), B=B)
    rng = np.random.default_rng(seed)
    nF = c.pb.n_frames
    frames = np.array([(3 * f) % nF if f % 5 else nF - 1 - (f % nF) for f in range(B)], np.int32)
    off = np.asarray(c.pb.frame_head_off)
    persons = np.full((B, poses.shape[1], c.pb.V), -1, np.int32)
    for f in range(B):
        H = int(off[frames[f] + 1] - off[frames[f]])
        persons[f] = rng.integers(-2, H + 2, persons[f].shape)
    mode, mask = 'tri' if tri else 'mlp', ALL & ~(1 << 3)
    st = S.new_state(700, S.BONES_18, 2.0 ** -8)
    S.observe_sequence(st, poses, flags, n_persons, ids, mode, mask)
    S.length_table(st, 3)
    return Seq(c.pb, persons, n_persons, poses, flags, ids, st, mode, frames, mask)


def same(got, want, what=''):
    """the six outputs bit for bit, NaN matching NaN"""
    SR = pkg('harness.skeleton_refine')
    for k in SR.KEYS:
        g, w = np.asarray(got[k]), np.asarray(want[k])
        assert g.dtype == w.dtype and g.shape == w.shape, (what, k, g.dtype, w.dtype, g.shape, w.shape)
        if not rc.same_bits(g, w):
            if g.dtype.kind == 'f':
                bad = np.argwhere(~((g == w) | (np.isnan(g) & np.isnan(w))))
            else:
                bad = np.argwhere(g != w)
            at = tuple(bad[0]) if len(bad) else ()
            assert False, (what, k, len(bad), at, g[at] if at else None, w[at] if at else None)
