"""harness/reprojection.py, the host statement of mpe_reproject_batch / mpe_residual_stats, and the --showgt
bookkeeping of harness/reprojection_error.py with the oracle as the inference side (no GPU)."""
import argparse
import copy
import json
import os

import numpy as np
import pytest

from conftest import GOLDEN, env, harness_model_files, oracle, pkg

HD = os.path.join(GOLDEN, 'harness')


def scalar_project(T, kd, K, p):
    """The formula of include/mpe.h as a plain scalar loop: np.float32 scalars, one operation per statement."""
    f32 = np.float32
    X, Y, Z = f32(p[0]), f32(p[1]), f32(p[2])
    with np.errstate(all='ignore'):
        pc = []
        for i in range(3):
            a = f32(T[i][0] * X)
            b = f32(T[i][1] * Y)
            s = f32(a + b)
            s = f32(s + f32(T[i][2] * Z))
            pc.append(f32(s + T[i][3]))
        h0 = f32(pc[0] / pc[2])
        h1 = f32(pc[1] / pc[2])
        n = f32(np.sqrt(f32(f32(h0 * h0) + f32(h1 * h1))))
        r = f32(n * n)
        t1 = f32(f32(1) + f32(kd[0] * r))
        t2 = f32(f32(kd[1] * r) * r)
        t3 = f32(f32(f32(kd[2] * r) * r) * r)
        f = f32(f32(t1 + t2) + t3)
        d0 = f32(h0 * f)
        d1 = f32(h1 * f)
        u = [f32(f32(f32(K[i][0] * d0) + f32(K[i][1] * d1)) + K[i][2]) for i in range(3)]
        return f32(u[0] / u[2]), f32(u[1] / u[2])


@pytest.mark.parametrize('variant', ['panoptic', 'arplab'])
def test_host_statement_equals_scalar_loop(variant):
    """1: vectorised statement == scalar loop, bit for bit, on random poses for every camera of the rig."""
    R = pkg('harness.reprojection')
    calib = env(variant).calib
    assert calib.n_cameras == (5 if variant == 'panoptic' else 6)
    T, kd, K = R.camera_constants(calib)
    assert T.dtype == kd.dtype == K.dtype == np.float32
    assert np.array_equal(T, calib.T_d[:, :3].astype(np.float32))
    rng = np.random.default_rng(17)
    pts = np.concatenate([rng.uniform(-3, 3, (200, 3)), rng.normal(0, 30, (40, 3)), np.zeros((1, 3))]).astype(np.float32)
    obs = rng.uniform(0, 1920, (len(pts), 2))
    for c in range(calib.n_cameras):
        px, py = R.project(T[c], kd[c], K[c], pts[:, 0], pts[:, 1], pts[:, 2])
        sq, res = R.pixel_distance(px, py, obs[:, 0], obs[:, 1])
        for i, p in enumerate(pts):
            sx, sy = scalar_project(T[c], kd[c], K[c], p)
            assert sx.tobytes() == px[i].tobytes() and sy.tobytes() == py[i].tobytes(), (variant, c, i)
            dx, dy = float(sx) - obs[i, 0], float(sy) - obs[i, 1]
            s = dx * dx + dy * dy
            assert np.float64(s).tobytes() == sq[i].tobytes()
            assert np.float64(np.sqrt(np.float64(s))).tobytes() == res[i].tobytes()


def _models(tmp_path, exp):
    import pickle
    import torch
    mdir = harness_model_files(str(tmp_path), exp['inputs'])
    prm = pickle.load(open(os.path.join(mdir, 'skeleton_matching.prms'), 'rb'))
    prm = dict(prm, nonlinearity=prm['nonlinearity'].negative_slope)
    gat_sd = {k: v.numpy() for k, v in torch.load(os.path.join(mdir, 'skeleton_matching.tch')).items()}
    mlp_sd = {k: v.numpy() for k, v in torch.load(os.path.join(mdir, 'pose_estimator.pytorch'))['model_state_dict'].items()}
    return prm, gat_sd, mlp_sd


def oracle_infer_arrays(calib, prm, gat_sd, mlp_sd):
    """The oracle as the inference side, in the batch arrays evaluate_arrays takes."""
    onp = oracle()
    params = calib.params
    sm = list(params.used_cameras_skeleton_matching)
    V, J = len(sm), len(params.joint_list)

    def infer(frames, owners):
        pb = pkg('packing').pack_frames(frames, params)
        results = [onp.run_frame(f, calib, gat_sd, prm, mlp_sd, mode='mlp') for f in frames]
        B = len(frames)
        pcap = max([1] + [len(r['persons']) for r in results if r is not None])
        a = {'pb': pb, 'persons': np.full((B, pcap, V), -1, np.int32), 'n_persons': np.zeros(B, np.int32),
             'poses': np.zeros((B, pcap, J, 3), np.float32), 'valid': np.zeros((B, pcap), np.uint8),
             'tri': np.zeros((B, pcap, J, 3), np.float64), 'jv': np.zeros((B, pcap, J), np.uint8)}
        for f, res in enumerate(results):
            if res is None:
                continue
            a['n_persons'][f] = len(res['persons'])
            k = 0
            for p, person in enumerate(res['persons']):
                a['persons'][f, p] = [-1 if h is None else h for h in person]
                skels = onp.person_skeletons(person, res['graph']['jsons_for_head'], sm)
                if onp.mlp_input_row(skels, calib)[1]:
                    a['poses'][f, p] = res['poses'][k]
                    a['valid'][f, p] = 1
                    k += 1
                for j, v in onp.triangulate_person(skels, calib, positive_ids_only=True, all_joints=True).items():
                    a['tri'][f, p, j] = np.asarray(v).reshape(3)
                    a['jv'][f, p, j] = 1
        return a
    return infer


def check_report(got, want):
    """Medians within rel 2e-4, means within half a decade (tests/test_oracle_golden.py:296-297); the same rows."""
    rows = {(kind, cam) for cam, kinds in want.items() for kind in kinds}
    assert set(got) == rows, (sorted(set(got) ^ rows))
    for cam, kinds in want.items():
        for kind, (mean, median) in kinds.items():
            g = got[(kind, cam)]
            print(cam, kind, 'got', g, 'reference', (mean, median))
            assert g[1] == pytest.approx(median, rel=2e-4), (cam, kind, g, median)
            assert abs(np.log10(g[0]) - np.log10(mean)) < 0.5, (cam, kind, g, mean)


def test_host_statement_reproduces_reference_report(tmp_path):
    """2: the vectorised statement's bookkeeping (no --showgt) against what the reference script printed."""
    rp = pkg('harness.reprojection_error')
    calib = env().calib
    exp = json.load(open(os.path.join(HD, 'harness_expected.json')))
    args = argparse.Namespace(synthetic=0, testfiles=[os.path.join(HD, exp['inputs']['testfile'])], datastep=exp['inputs']['datastep'])
    work = rp.collect_work(args, calib)
    got = rp.evaluate_arrays(work, oracle_infer_arrays(calib, *_models(tmp_path, exp)), calib, showgt=False, batch=6)
    check_report(got, exp['reprojection_error'])


def test_showgt_bookkeeping_reproduces_reference_report(tmp_path):
    """3: --showgt on the derived input (add_joint2_from_minus1 applied to the committed file at run time) against what the
    reference script printed with --showgt (tests/checkers/gen_reprojection_showgt_golden.py): all three rows of all five cameras."""
    rp, R = pkg('harness.reprojection_error'), pkg('harness.reprojection')
    calib = env().calib
    exp = json.load(open(os.path.join(HD, 'reprojection_showgt_expected.json')))
    assert exp['inputs']['transform'] == R.TRANSFORM_NAME
    frames = json.load(open(os.path.join(HD, exp['inputs']['testfile'])))
    assert R.add_joint2_from_minus1(frames) == exp['inputs']['bodies_changed']
    derived = os.path.join(str(tmp_path), exp['inputs']['testfile'])
    json.dump(frames, open(derived, 'w'))
    args = argparse.Namespace(synthetic=0, testfiles=[derived], datastep=exp['inputs']['datastep'], tmdir=[HD])
    work = rp.collect_work_showgt(args, calib)
    assert 0 < len(work) < len(range(0, len(frames), exp['inputs']['datastep']))       # frames 6, 24 (invalid bodies) and 33 (none) go
    base = json.load(open(os.path.join(HD, 'harness_expected.json')))
    got = rp.evaluate_arrays(work, oracle_infer_arrays(calib, *_models(tmp_path, base)), calib, showgt=True, batch=6)
    assert len(exp['reprojection_error']) == 5 and all(set(k) == {'est', 'GT', 'triang'} for k in exp['reprojection_error'].values())
    check_report(got, exp['reprojection_error'])


def test_transform_changes_exactly_the_incomplete_bodies():
    """5: '2' is added to the bodies that have '-1' and lack '2', and to nothing else."""
    R = pkg('harness.reprojection')
    frames = json.load(open(os.path.join(HD, 'syn_pinning_test.json')))
    before = copy.deepcopy(frames)
    want = sum(1 for fr in before for cam in fr for b in fr[cam][3] if '-1' in b and '2' not in b)
    assert R.add_joint2_from_minus1(frames) == want == 606
    untouched = 0
    for fa, fb in zip(frames, before):
        assert list(fa) == list(fb)
        for cam in fa:
            assert fa[cam][:3] == fb[cam][:3] and len(fa[cam][3]) == len(fb[cam][3])
            for a, b in zip(fa[cam][3], fb[cam][3]):
                if '-1' in b and '2' not in b:
                    assert a['2'] == b['-1'] and {k: v for k, v in a.items() if k != '2'} == b
                else:
                    assert a == b
                    untouched += 1
    assert untouched > 0                                     # the bodies of frames 6 and 24 that lost '-1' stay invalid
    assert R.add_joint2_from_minus1(frames) == 0
    J = env().params.joint_list
    oks = [R.showgt_frame_ok(fr, J) for fr in frames]
    assert oks[6] is False and oks[24] is False and oks[33] is False and oks[0] is True
    assert all(R.showgt_frame_ok(fr, J) is False for fr in before)        # the committed file: every frame skipped


def _tiny(calib, bodies, valid_last=1.0, valid_other=1.0):
    """One frame, one person seen exactly (no noise) by cameras 0 and 1; GT bodies as given (dataset == rig calibration)."""
    R = pkg('harness.reprojection')
    params = calib.params
    J = len(params.joint_list)
    T, kd, K = R.camera_constants(calib)
    rng = np.random.default_rng(3)
    pose = (np.array([0.2, 1.0, 0.3]) + rng.uniform(-0.3, 0.3, (J, 3))).astype(np.float32)
    frame = {}
    for c in (0, 1):
        px, py = R.project(T[c], kd[c], K[c], pose[:, 0], pose[:, 1], pose[:, 2])
        sk = {str(j): [j, float(px[j]) + (3.0 if j == J - 1 else 0.0), float(py[j]), valid_last if j == J - 1 else valid_other, 0.9]
              for j in range(J)}
        frame[params.camera_names[c]] = [json.dumps([sk]), 0.0, 'no_image', bodies]
    return frame, pose


def _gt_body(calib, world, drop=(), minus1=True):
    """A GT body in the wire format from world points [J,3]: cm in the dataset's root frame, which the script takes to
    dataset camera 1 and back to the rig's world; here the dataset calibration is the rig's, so the round trip returns the
    points up to float32."""
    body = {str(j): [float(x) * 100.0 for x in world[j]] for j in range(len(world)) if j not in drop}
    if minus1:
        body['-1'] = body.get('0', [0.0, 0.0, 0.0])
    return body


def _run_tiny(calib, frame, pose, showgt=True):
    rp = pkg('harness.reprojection_error')
    params = calib.params
    J, V = len(params.joint_list), len(params.camera_names)
    args = argparse.Namespace(synthetic=0, testfiles=[], datastep=1, tmdir=['.'])
    import torch
    ok = pkg('harness.reprojection').showgt_frame_ok(frame, params.joint_list)
    work = [(frame, None, torch.from_numpy(calib.T_d[1]).type(torch.float32))] if ok else []

    def infer(frames, owners):
        pb = pkg('packing').pack_frames(frames, params)
        persons = np.full((1, 2, V), -1, np.int32)
        persons[0, 0, 0], persons[0, 0, 1] = 0, 1
        poses = np.zeros((1, 2, J, 3), np.float32)
        poses[0, 0] = pose
        return {'pb': pb, 'persons': persons, 'n_persons': np.array([1], np.int32), 'poses': poses, 'valid': np.array([[1, 0]], np.uint8),
                'tri': poses.astype(np.float64), 'jv': np.ones((1, 2, J), np.uint8)}
    return rp.evaluate_arrays(work, infer, calib, showgt=True, batch=4), args


def test_showgt_books_one_joint_per_person_and_camera():
    """4a: the one-joint quirk.  The detections are the exact projections of the pose, except that the LAST joint sits
    3 px to the right in x.  The GT bodies: a far one first, then the pose itself.  The script selects the second body
    (smallest mean distance), projects all its joints but compares only the last key of its dict: one entry per camera,
    equal to 3 px up to the float32 of the projection; est and triang book all used / all joints."""
    calib = env().calib
    params = calib.params
    J = len(params.joint_list)
    frame, pose = _tiny(calib, [])
    bodies = [_gt_body(calib, pose + np.float32(1.5)), _gt_body(calib, pose)]
    for cam in frame:
        frame[cam][3] = bodies
    got, _ = _run_tiny(calib, frame, pose)
    for c in (0, 1):
        cam = params.camera_names[c]
        mean, median, n = got[('GT', cam)]
        assert n == 1 and mean == median and abs(mean - 3.0) < 2e-2, got[('GT', cam)]      # GT went cm -> world in float32
        assert got[('est', cam)][2] == len(params.used_joints) and got[('triang', cam)][2] == J
        # J - 1 joints at 0 px, one at 3 px (if it is a used joint): the median is 0 up to float32 pixels
        assert got[('triang', cam)][1] < 1e-3 and abs(got[('triang', cam)][0] - 3.0 / J) < 1e-3
    assert {cam for _, cam in got} == set(params.camera_names[:2])
    # the last joint's `valid` at 0.5 is not > 0.5: the GT row books nothing and is not printed
    frame2, pose2 = _tiny(calib, bodies, valid_last=0.5)
    got2, _ = _run_tiny(calib, frame2, pose2)
    assert not any(kind == 'GT' for kind, _ in got2)
    assert got2[('triang', params.camera_names[0])][2] == J - 1
    # ... while the other joints' `valid` does not matter to the GT row
    frame3, pose3 = _tiny(calib, bodies, valid_other=0.0)
    got3, _ = _run_tiny(calib, frame3, pose3)
    assert got3[('GT', params.camera_names[0])][2] == 1 and got3[('triang', params.camera_names[0])][2] == 1


def test_showgt_skip_rule():
    """4b: a frame is dropped from ALL rows when a body lacks '-1' or a joint of joint_list, or when there are no bodies."""
    calib = env().calib
    R = pkg('harness.reprojection')
    J = len(calib.params.joint_list)
    frame, pose = _tiny(calib, [])
    good = _gt_body(calib, pose)
    cases = {'complete': ([good], True), 'no bodies': ([], False), 'no -1': ([good, _gt_body(calib, pose, minus1=False)], False),
             'joint 2 missing': ([_gt_body(calib, pose, drop=(2,)), good], False)}
    for name, (bodies, keep) in cases.items():
        fr = copy.deepcopy(frame)
        for cam in fr:
            fr[cam][3] = bodies
        assert R.showgt_frame_ok(fr, calib.params.joint_list) is keep, name
        got, _ = _run_tiny(calib, fr, pose)
        assert bool(got) is keep, (name, got)
    fr = {cam: v[:3] for cam, v in frame.items()}
    assert R.showgt_frame_ok(fr, calib.params.joint_list) is None          # no GT field: the script exits


def test_residual_selection_rules():
    """The sentinel cases of the residual tensor, one by one, on a hand-made batch."""
    R = pkg('harness.reprojection')
    calib = env().calib
    params = calib.params
    J, V = len(params.joint_list), len(params.camera_names)
    frame, pose = _tiny(calib, [])
    sk = json.loads(frame[params.camera_names[1]][0])[0]
    del sk['4']                                              # joint 4 absent from camera 1's skeleton
    sk['5'][3] = 0.5                                         # valid == 0.5 is not > 0.5
    frame[params.camera_names[1]][0] = json.dumps([sk])
    pb = pkg('packing').pack_frames([{c: v[:2] for c, v in frame.items()}], params)
    persons = np.full((1, 3, V), -1, np.int32)
    persons[0, 0, :2] = 0, 1
    persons[0, 1, :2] = 0, 1                                 # second person: flag off
    persons[0, 2, :2] = 0, 1                                 # third slot: beyond n_persons
    poses = np.broadcast_to(pose, (1, 3, J, 3)).copy()
    mask = (1 << J) - 1 - (1 << 7)                           # joint 7 not selected
    res = R.residuals(calib, pb, persons, np.array([2], np.int32), poses, np.array([[1, 0, 1]], np.uint8), mask)
    assert res.shape == (1, 3, V, J)
    want = np.zeros((3, V, J), bool)
    want[0, :2] = True
    want[0, :, 7] = False
    want[0, 1, 4] = want[0, 1, 5] = False
    assert np.array_equal(res[0] >= 0, want) and np.all(res[0][~want] == R.SENTINEL)
    jf = np.ones((1, 3, J), np.uint8)
    jf[0, 0, 9] = 0
    res2 = R.residuals(calib, pb, persons, np.array([2], np.int32), poses.astype(np.float64), jf, mask)
    want2 = want.copy()
    want2[1] = want[0]
    want2[0, :, 9] = False
    assert np.array_equal(res2[0] >= 0, want2)
    st = R.stats([res, res2])
    assert st['count'].tolist() == [int(want[:, c].sum() + want2[:, c].sum()) for c in range(V)]
