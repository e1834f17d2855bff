"""harness/skeleton_refine.py, the numpy statement of mpe_body_refine_batch, against what the rule alone decides: it is the
verified per-joint refinement when the bones weigh nothing, the bodies are its fixed point, it recovers a joint one camera
saw, it never raises a row's cost, and its colours separate the ends of every bone."""
import numpy as np
import pytest

import refine_cases as rc
import skel_refine_cases as k
from conftest import env, pkg


@pytest.mark.parametrize('mode', ['mlp', 'tri'])
@pytest.mark.parametrize('huber', [0.0, 5.0])
@pytest.mark.parametrize('sweeps', [1, 10])
def test_without_bone_weight_it_is_the_per_joint_refinement(mode, huber, sweeps):
    """bone_weight = 0: a sweep is one iteration of harness.refine.refine; every joint two or more cameras saw has that
    statement's bits, poses and MOVED alike ('messy': cameras missing, detections that must not count)"""
    SR, RF = pkg('harness.skeleton_refine'), pkg('harness.refine')
    s = k.known('messy', mode)
    out = s.run(sweeps=sweeps, bone_weight=0.0, huber_px=huber)
    ref = RF.refine(env().calib, s.pb, s.persons, s.n_persons, s.poses, s.flags, k.ALL, max_iters=sweeps, step_tol=0.0, huber_px=huber)
    rows = np.arange(s.pcap)[None, :] < s.n_persons[:, None]
    assert ((out['n_bones'] > 0) == rows).all() and rows.sum() > 40                   # every row is processed
    assert np.array_equal(out['n_views'], ref['n_views'])
    m = ref['n_views'] >= 2
    assert m.sum() > 700 and rc.same_bits(out['poses'][m], ref['poses'][m])
    assert np.array_equal((out['status'][m] & SR.MOVED) != 0, (ref['status'][m] & RF.MOVED) != 0)
    assert ((out['status'][m] & SR.MOVED) != 0).sum() > 700 and (out['cost'][rows][:, [1, 3]] == 0.0).all()


def test_the_bodies_are_a_fixed_point():
    """noise-free detections, the lengths of the bodies, a start at the bodies: float64 rows, which alone can hold the
    bodies exactly (a float32 start is the bodies rounded, 1e-7 m off)"""
    s = k.known('messy', 'tri', exact=True, start='truth')
    out = s.run(sweeps=8, bone_weight=300.0)
    proc = out['n_bones'] > 0
    assert proc.sum() > 40
    assert np.linalg.norm(out['poses'] - s.poses, axis=-1).max() <= 1e-9
    assert (out['cost'][proc][:, 2:].sum(axis=1) <= 1e-12).all() and (out['cost'][~proc] == -1.0).all()


def test_a_joint_one_camera_saw_is_recovered():
    """An elbow (7) and a knee (13) of each of four bodies, seen by one camera only and seeded 40 mm off along that
    camera's ray (two cameras or more, both signs) with the flag of a filled joint: after 8 sweeps at 300 px/m every one lies
    within 1 mm of the body's joint.  Measured on this rig with the statement: 12.4 mm at most after 1 sweep, 4.0 after 2,
    0.44 after 4, 0.0054 after 8.  The per-joint refinement declines them all."""
    SR, RF = pkg('harness.skeleton_refine'), pkg('harness.refine')
    s, where = k.one_view()
    assert len(where) == 8 and len({c for _, _, c in where}) >= 2
    out = s.run(sweeps=8, bone_weight=300.0)
    ref = RF.refine(env().calib, s.pb, s.persons, s.n_persons, s.poses, s.flags, k.ALL, max_iters=8)
    for p, j, _ in where:
        before = np.linalg.norm(s.poses[0, p, j] - s.truth[0, p, j])
        after = np.linalg.norm(out['poses'][0, p, j] - s.truth[0, p, j])
        print(p, j, before, after)
        assert abs(before - 0.040) < 1e-12 and after < 0.001
        assert out['n_views'][0, p, j] == 1 and out['status'][0, p, j] & (SR.ONE_VIEW | SR.MOVED) == SR.ONE_VIEW | SR.MOVED
        assert ref['status'][0, p, j] == RF.FEW_VIEWS and ref['poses'][0, p, j].tobytes() == s.poses[0, p, j].tobytes()


@pytest.mark.parametrize('mode', ['mlp', 'tri'])
def test_no_row_costs_more_and_the_bones_come_closer(mode):
    """'messy' with its noise: every accepted update lowers the local cost and with it the row's, so no processed row ends
    above its start (no allowance was needed on the statement), and the worst bone of a row comes closer on average"""
    s = k.known('messy', mode)
    out = s.run(sweeps=8, bone_weight=300.0)
    proc = out['n_bones'] > 0
    c = out['cost'][proc]
    assert proc.sum() > 40 and (c[:, 2] + c[:, 3] <= c[:, 0] + c[:, 1]).all()
    assert c[:, 2:].sum() < c[:, :2].sum()
    err = out['err'][proc]
    assert err[:, 1].mean() < err[:, 0].mean()


def test_colours():
    S, SR = pkg('harness.skeleton'), pkg('harness.skeleton_refine')
    chain = [(j, j + 1) for j in range(17)]
    star = [(4, j) for j in range(18) if j != 4]
    repeated = [(0, 1), (1, 2), (0, 1), (2, 0), (5, 6)]
    for bones, n in ((S.BONES_18, 3), (chain, 2), (star, 2), (repeated, 3)):
        col = SR.colours(bones, 18)
        assert col.shape == (18,) and col.min() == 0 and col.max() == n - 1
        assert all(col[a] != col[b] for a, b in bones)
        touched = {j for b in bones for j in b}
        assert all(col[j] == 0 for j in range(18) if j not in touched)
    # the hips and the neck form a triangle
    assert len({int(SR.colours(S.BONES_18, 18)[j]) for j in (11, 12, 17)}) == 3
    # the incident lists keep list order
    assert SR.incident(repeated, 18)[0] == [(0, 1), (2, 1), (3, 2)]


def test_arguments_the_call_declines():
    s = k.known('one frame', 'tri')
    for bad in (dict(sweeps=0), dict(sweeps=65), dict(bone_weight=-1.0), dict(bone_weight=float('nan')), dict(huber_px=-1.0), dict(threshold=-0.5)):
        with pytest.raises(ValueError):
            s.run(**bad)
    with pytest.raises(ValueError):
        k.Seq(s.pb, s.persons[:0], s.n_persons[:0], s.poses[:0], s.flags[:0], s.ids[:0], s.state, 'tri').run()


def test_frame_map_and_rows_that_are_not_fitted():
    """a bad entry of the frame map copies its frame through with BAD_FRAME; a row without lengths, over the table or
    without an id is copied through with cost -1"""
    SR = pkg('harness.skeleton_refine')
    s = k.spoiled('messy', 'tri')
    F = len(s.poses)
    s.frames = np.arange(F, dtype=np.int32)
    s.frames[5], s.frames[6] = F, -1
    out = s.run(sweeps=3)
    for f in (5, 6):
        assert (out['status'][f] == SR.BAD_FRAME).all() and out['poses'][f].tobytes() == s.poses[f].tobytes() and (out['cost'][f] == -1.0).all()
    for f, p in ((2, 0), (3, 0), (3, 1)):
        assert out['n_bones'][f, p] == 0 and not out['status'][f, p].any() and out['poses'][f, p].tobytes() == s.poses[f, p].tobytes()
        assert (out['cost'][f, p] == -1.0).all() and (out['err'][f, p] == -1.0).all()
    assert out['n_bones'][2, 1] == 3 and out['status'][0, 1, 8] & SR.BAD_START and out['poses'][0, 1, 8].tobytes() == s.poses[0, 1, 8].tobytes()
    assert not out['status'][1, 0, 5] and out['n_bones'][1, 0] < 18 and out['status'][4, 1, 13] & SR.FREE
    ident = s.run(sweeps=3)
    s.frames = None
    k.same(k.Seq(s.pb, s.persons, s.n_persons, s.poses, s.flags, s.ids, s.state, 'tri',
                 np.arange(F, dtype=np.int32)).run(sweeps=3), s.run(sweeps=3), 'identity')
    assert ident['status'][5, 0, 0] == SR.BAD_FRAME


@pytest.mark.parametrize('mode', ['mlp', 'tri'])
@pytest.mark.parametrize('name', ['ring23', 'arprobot'])
def test_rig_sequences_take_their_branches(name, mode):
    """the tracked sequences on the 23-camera and the camera-subset rig: views per row, ONE_VIEW where a single camera
    sees the person, an odd number of rows on the ring (asserted in skel_refine_cases.rig)"""
    s, info = k.rig(name, mode)
    print(name, mode, info)
    assert info['rows'] == len(s.poses) * s.pcap
