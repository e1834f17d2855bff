"""CPU: the camera axis of the statement modules is the engine's camera slot (the index head_cam and the columns of
`persons` hold), not the index into the calibration's arrays.  The two differ on a camera-subset preset: ARPLAB_ROBOT
configures six cameras and uses the two at calibration indices 4 and 5.

The reference is exact.  ARPLAB uses all six cameras, so there the calibration index is the slot.  Frames that carry only
the two robot cameras' skeletons are packed once with ARPLAB_ROBOT (V = 2, slots 0 and 1) and once with ARPLAB (V = 6,
cameras 4 and 5): the same heads under renumbered columns.  Every statement must give the same bits under both packings
once the camera axis is renumbered -- a camera without a head adds nothing to any fold -- and the four extra streams of
a six-stream frame must change nothing."""
import numpy as np
import pytest

import refine_cases as rc
from conftest import env, oracle, pkg

J = rc.J
ALL = (1 << J) - 1
SLOTS = [4, 5]                                   # the calibration indices (= ARPLAB slots) of ARPLAB_ROBOT's slots 0 and 1
FRAMES = rc.RIG_FRAMES['arprobot'][:2]            # generator frames with every joint of 3 persons in both robot images
_made = {}


class Rig:
    """Two frames of 3 persons with 1 px of noise: `two` (the robot streams only) and `six` (all streams) packed with
    ARPLAB_ROBOT, `wide` (the robot streams only) packed with ARPLAB; the true rows, and poses a few millimetres off."""

    def __init__(self):
        syn, onp, packing = pkg('synthetic'), oracle(), pkg('packing')
        self.robot, self.arplab = env('arprobot'), env('arplab')
        used = list(self.robot.params.used_cameras_skeleton_matching)
        assert [self.robot.calib.index(c) for c in used] == SLOTS == [self.arplab.calib.index(c) for c in used]
        made = [syn.make_frame(self.robot.calib, i, syn.FrameSpec(persons=3, noise_px=1.0)) for i in FRAMES]
        six = [m[0] for m in made]
        two = [{c: f[c] for c in used} for f in six]
        assert all(len(f) == 6 for f in six)
        self.two = packing.pack_frames([onp.processed_input(f) for f in two], self.robot.params)
        self.six = packing.pack_frames([onp.processed_input(f) for f in six], self.robot.params)
        self.wide = packing.pack_frames([onp.processed_input(f) for f in two], self.arplab.params)
        assert self.two.V == 2 and self.wide.V == 6 and self.two.n_heads == self.wide.n_heads == 12
        assert np.array_equal(np.asarray(self.wide.head_cam), np.asarray(self.two.head_cam) + 4)
        F, self.pcap = len(FRAMES), 4
        self.n_persons = np.array([3] * F, np.int32)
        self.rows2 = np.full((F, self.pcap, 2), -1, np.int32)
        for f in range(F):
            h0, H, _, _ = self.two.frame_counts(f)
            for i in range(H):
                c = int(self.two.head_cam[h0 + i])
                self.rows2[f, made[f][1]['owner'][used[c]][int(self.two.skeleton_index[h0 + i])], c] = i
        assert (self.rows2[:, :3] >= 0).all()
        self.truth = np.zeros((F, self.pcap, J, 3))
        for f, m in enumerate(made):
            self.truth[f, :3] = m[1]['persons']
        rng = np.random.default_rng(17)
        self.tri = self.truth + rng.uniform(-0.004, 0.004, self.truth.shape)
        self.jflags = np.zeros((F, self.pcap, J), np.uint8)
        self.jflags[:, :3] = 1
        self.jflags[0, 1, 6] = 0
        self.est = (self.truth + rng.uniform(-0.02, 0.02, self.truth.shape)).astype(np.float32)
        self.pflags = (np.arange(self.pcap)[None, :] < self.n_persons[:, None]).astype(np.uint8)
        self.used = sum(1 << j for j in self.robot.params.used_joints)

    def widen(self, rows2):
        """[F,Pcap,2] over the slots of ARPLAB_ROBOT -> [F,Pcap,6] over those of ARPLAB"""
        out = np.full(rows2.shape[:2] + (6,), -1 if rows2.dtype.kind == 'i' else 0, rows2.dtype)
        out[:, :, SLOTS] = rows2
        return out

    def kinds(self):
        return {'triang': (self.tri, self.jflags, ALL), 'est': (self.est, self.pflags, self.used)}

    def packings(self, rows2=None):
        """(calibration, batch, rows) of the three packings; the first is the one the others must equal"""
        rows2 = self.rows2 if rows2 is None else rows2
        return [(self.robot.calib, self.two, rows2), (self.robot.calib, self.six, rows2), (self.arplab.calib, self.wide, self.widen(rows2))]


def rig():
    if 'rig' not in _made:
        _made['rig'] = Rig()
    return _made['rig']


def same(a, b, what):
    assert rc.same_bits(np.asarray(a), np.asarray(b)), what


def test_the_helper_gives_the_engine_order():
    """engine_calibration: row c of every array is the calibration's row of slot c's camera -- what Engine uploads"""
    R, RF, G, CB = (pkg('harness.' + m) for m in ('reprojection', 'refine', 'geometric', 'calibrate'))
    r = rig()
    for e, idx in ((r.robot, SLOTS), (r.arplab, list(range(6))), (env('ring23'), list(range(23)))):
        calib = e.calib
        assert R.engine_cameras(calib) == idx == CB.engine_cameras(calib)
        P, dist, K32 = R.engine_calibration(calib)
        same(P, np.asarray(calib.P, np.float64)[idx], 'P')
        same(dist, np.asarray(calib.dist, np.float64)[idx], 'dist')
        same(K32, np.asarray(calib.K32, np.float32)[idx], 'K32')
        T, kd, K = RF.camera_constants64(calib)
        assert T.shape == (len(idx), 3, 4) and kd.shape == (len(idx), 3) and K.shape == (len(idx), 3, 3)
        same(T, P, 'T64'), same(kd, dist[:, [0, 1, 4]], 'kd64'), same(K, K32.astype(np.float64), 'K64')
        T, kd, K = R.camera_constants(calib)
        same(T, P.astype(np.float32), 'T32'), same(kd, dist[:, [0, 1, 4]].astype(np.float32), 'kd32'), same(K, K32, 'K32')
        Kg, dg, Tg = G.camera_constants(calib)
        same(Kg, K32.astype(np.float64), 'Kg'), same(dg, dist, 'dg'), same(Tg, P, 'Tg')
        same(CB.start_extrinsics(calib), P, 'start')


@pytest.mark.parametrize('kind', ['triang', 'est'])
def test_regroup_cost_table_and_rows(kind):
    """cost_table of the true (head, person) pairs is a pixel or two (it was hundreds: the projection through the first
    two configured cameras) and equal under the three packings; regroup restores a swap instead of releasing every head"""
    RG = pkg('harness.regroup')
    r = rig()
    poses, flags, mask = r.kinds()[kind]
    swapped = r.rows2.copy()
    swapped[0, 0, 1], swapped[0, 1, 1] = r.rows2[0, 1, 1], r.rows2[0, 0, 1]
    swapped[1, 2, 0] = -1
    first = None
    for calib, pb, rows in r.packings(swapped):
        cost, n = RG.cost_table(calib, pb, poses, flags, r.n_persons, mask, counts=True)
        out = RG.regroup(calib, pb, rows, r.n_persons, poses, flags, mask, min_views=2)
        if first is None:
            first = cost, n, out
            off = np.asarray(pb.frame_head_off)
            true = np.array([cost[off[f] + r.rows2[f, p, c], p] for f in range(2) for p in range(3) for c in range(2)])
            print(kind, 'cost of the true pairs', true.min(), true.max())
            assert (true > 0).all() and true.max() < (3.0 if kind == 'triang' else 25.0)
            assert np.array_equal(out['persons'], r.rows2) and out['counts'].tolist() == [[2, 2, 0, 0], [0, 1, 0, 0]]
            continue
        same(cost, first[0], 'cost'), same(n, first[1], 'n')
        wide = rows.shape[2] == 6
        for k in ('persons', 'change'):
            same(out[k][:, :, SLOTS] if wide else out[k], first[2][k], k)
            if wide:
                rest = [c for c in range(6) if c not in SLOTS]
                assert (out[k][:, :, rest] == (-1 if k == 'persons' else 0)).all()
        for k in ('n_views', 'cost', 'counts', 'status'):
            same(out[k], first[2][k], k)


@pytest.mark.parametrize('kind', ['triang', 'est'])
def test_refine(kind):
    """refine ran out of the camera axis (IndexError) on the subset rig; now all six outputs are those of the wide packing"""
    RF = pkg('harness.refine')
    r = rig()
    poses, flags, mask = r.kinds()[kind]
    outs = [RF.refine(calib, pb, rows, r.n_persons, poses, flags, mask, max_iters=10, huber_px=h)
            for h in (0.0, 5.0) for calib, pb, rows in r.packings()]
    for h in (0, 1):
        first = outs[3 * h]
        assert (first['n_views'][:, :3][..., 5] == 2).all() and (first['status'] & RF.MOVED).any()
        assert first['cost1'][first['status'] & RF.SOLVED != 0].max() < first['cost0'].max()
        for other in outs[3 * h + 1:3 * h + 3]:
            for k in ('poses', 'status', 'cost0', 'cost1', 'iters', 'n_views'):
                same(other[k], first[k], (kind, h, k))


@pytest.mark.parametrize('kind', ['triang', 'est'])
def test_residuals(kind):
    """residuals could not broadcast six cameras against two; now [F,Pcap,2,J] equals columns 4 and 5 of the wide packing,
    whose other columns hold the sentinel, and the true poses are within a few pixels"""
    R = pkg('harness.reprojection')
    r = rig()
    poses, flags, mask = r.kinds()[kind]
    res = [R.residuals(calib, pb, rows, r.n_persons, poses, flags, mask) for calib, pb, rows in r.packings()]
    assert res[0].shape == (2, r.pcap, 2, J) and res[2].shape == (2, r.pcap, 6, J)
    same(res[1], res[0], 'six streams')
    same(res[2][:, :, SLOTS], res[0], 'wide')
    assert (res[2][:, :, [0, 1, 2, 3]] == R.SENTINEL).all()
    counted = res[0][res[0] >= 0]
    print(kind, 'counted', len(counted), 'largest', counted.max())
    assert len(counted) > 100 and counted.max() < (6.0 if kind == 'triang' else 40.0)
    st = R.stats([res[0].reshape(-1, 2, J)])
    assert len(st['count']) == 2 and (st['count'] > 0).all()


@pytest.mark.parametrize('mode', ['tri', 'mlp'])
def test_refine_sequence(mode):
    """the body-level fit: every (frame, row) a track with the lengths of its body; all six outputs equal"""
    S, SR = pkg('harness.skeleton'), pkg('harness.skeleton_refine')
    import skel_refine_cases as k
    r = rig()
    poses, flags, mask = r.kinds()['triang' if mode == 'tri' else 'est']
    F, pcap = poses.shape[:2]
    row = np.arange(pcap)[None, :] < r.n_persons[:, None]
    ids = np.where(row, np.arange(F * pcap).reshape(F, pcap), -1).astype(np.int32)
    st = S.new_state(F * pcap, S.BONES_18, 0.002, J)
    S.set_lengths(st, k.lengths_of(r.truth, st['bones']).reshape(F * pcap, -1))
    outs = [SR.refine_sequence(st, calib, pb, rows, r.n_persons, poses, flags, ids, mode, mask, sweeps=4) for calib, pb, rows in r.packings()]
    assert (outs[0]['status'] & SR.MOVED).any() and (outs[0]['n_views'][:, :3][..., 5] == 2).all() and (outs[0]['n_bones'][:, :3] > 0).all()
    for other in outs[1:]:
        k.same(other, outs[0], mode)


def test_ray_scores():
    """the ray scores of harness/geometric.py on the shared edge-nodes: the same pairs, every joint voting, and scores,
    votes, means and distances equal under the three packings (the module took its constants in camera-slot order before
    the helper existed, so this also holds the helper to the order that was right)"""
    G = pkg('harness.geometric')
    r = rig()
    outs = [G.scores(calib, pb) for calib, pb, _ in r.packings()]
    pairs = [G.batch_pairs(pb) for _, pb, _ in r.packings()]
    assert len(pairs[0]) == 18 and np.array_equal(pairs[0], pairs[1]) and np.array_equal(pairs[0], pairs[2])
    assert (outs[0]['n_votes'] == J).all() and (outs[0]['scores'] > 0).all() and (outs[0]['mean'] > 0).all()
    for other in outs[1:]:
        for key in ('scores', 'n_votes', 'mean', 'dist'):
            same(other[key], outs[0][key], key)


def test_consolidate_and_calibration_sums():
    """consolidate founds body 2 from its two free heads and gives equal rows, tables and counts under the three
    packings; the sums of a calibration pass at moved extrinsics are equal per camera, and the wide packing's four
    unused cameras have no observation (a camera mapped twice would project through the wrong constants)"""
    CS, CB = pkg('harness.consolidate'), pkg('harness.calibrate')
    r = rig()
    poses, flags, mask = r.kinds()['triang']
    rows2 = r.rows2.copy()
    rows2[:, 2] = -1                                          # body 2 without a row: founded from its two free heads
    n = np.array([2, 2], np.int32)
    outs = [CS.consolidate(calib, pb, rows, n, poses, flags, mask) for calib, pb, rows in r.packings(rows2)]
    assert outs[0]['counts'][:, 1].tolist() == [1, 1] and np.array_equal(outs[0]['persons'][:, :3], r.rows2[:, :3])
    for other in outs[1:]:
        wide = other['persons'].shape[2] == 6
        same(other['persons'][:, :, SLOTS] if wide else other['persons'], outs[0]['persons'], 'persons')
        for key in ('n_persons', 'n_views', 'dist', 'pair', 'free', 'counts', 'status'):
            same(other[key], outs[0][key], key)
    sums = []
    for calib, pb, rows in r.packings():
        E = moved(CB, calib)
        sums.append(CB.calib_pass_host(calib, E, pb, rows, r.n_persons, poses, flags, mask, huber_px=5.0))
    assert sums[0]['acc'].shape == (2, CB.SUMS) and sums[0]['n_obs'].min() > 40
    for key in ('acc', 'n_obs', 'n_skipped'):
        same(sums[1][key], sums[0][key], key)
        same(sums[2][key][SLOTS], sums[0][key], key)
    assert not sums[2]['n_obs'][:4].any()


def moved(CB, calib):
    """the engine's extrinsics, every camera moved by half a degree and a centimetre, seeded by the camera (not the slot)"""
    E = CB.start_extrinsics(calib)
    return np.stack([CB.perturbed(E[c], 0.5, 10.0, 40 + k) for c, k in enumerate(CB.engine_cameras(calib))])
