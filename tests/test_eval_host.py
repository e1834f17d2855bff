"""CPU: the device evaluation path's host side (harness/assignment.py, pack_ground_truth, DeviceMetrics) against the
host scorer it replaces (harness/common.py: ground_truth, Metrics) and a verbatim restatement of the reference's
permutation loop (metrics_from_model.py:322-337)."""
import copy
import itertools
import json
import os
import re

import numpy as np
import pytest
import torch

from conftest import GOLDEN, ROOT, pkg


def reference_assignment(table):
    G, R = table.shape
    perms = itertools.permutations(range(R), G) if G <= R else itertools.permutations(range(G), G)
    best, best_p = 10000., None
    for p in perms:
        acc = 0
        for i, r in enumerate(p):
            if r < R:
                acc += table[i, r]
        if acc < best:
            best, best_p = acc, p
    return best_p


def random_table(rng, G, R):
    kind = rng.integers(0, 5)
    if kind == 0:                                    # quantized: many exact ties
        t = rng.integers(0, 4, (G, R)) * 0.125
    elif kind == 1:                                  # float32-rounded near-ties
        t = (0.3 + rng.integers(0, 3, (G, R)) * np.float32(1e-7)).astype(np.float32).astype(np.float64)
    elif kind == 2:                                  # diagonal-dominant, like real detections
        t = rng.uniform(0.2, 1.0, (G, R))
        for i in range(min(G, R)):
            t[i, rng.integers(0, R)] = rng.uniform(0.0, 0.05)
    else:
        t = rng.uniform(0.0, 1.0, (G, R))
    if G and rng.random() < 0.3:                     # GT bodies without a used joint
        t[rng.integers(0, G)] = 0.0
    return t


def test_bnb_equals_the_reference_permutation_loop():
    A = pkg('harness.assignment')
    rng = np.random.default_rng(1)
    n = 0
    for _ in range(6000):
        G, R = int(rng.integers(1, 7)), int(rng.integers(0, 7))
        t = random_table(rng, G, R)
        assert A.assign_bnb(t) == reference_assignment(t), (t.tolist(),)
        n += 1
    assert n >= 5000
    # nothing below 10000: None, as the loop leaves it
    assert A.assign_bnb(np.full((2, 2), 6000.)) is None and reference_assignment(np.full((2, 2), 6000.)) is None


def test_bnb_scales_past_the_permutation_loop():
    """G = 10 of R = 25 (P(25, 10) ~ 1.2e13 permutations): the bound finds the diagonal optimum in a few nodes."""
    A = pkg('harness.assignment')
    rng = np.random.default_rng(2)
    t = rng.uniform(0.3, 1.0, (10, 25))
    cols = rng.permutation(25)[:10]
    t[np.arange(10), cols] = rng.uniform(0.0, 0.01, 10)
    assert A.assign_bnb(t, node_budget=10000) == tuple(int(c) for c in cols)


def random_frame(rng, G, R, J, used, tri):
    gt_xyz = rng.uniform(-3, 3, (G, J, 3)).astype(np.float32)
    gt_joint = rng.random((G, J)) < 0.8
    gt_valid = rng.random(G) < 0.85
    dt = np.float64 if tri else np.float32
    poses = np.empty((R, J, 3), dt)
    for r in range(R):
        g = rng.integers(0, G)
        poses[r] = (gt_xyz[g].astype(np.float64) + rng.normal(0, rng.choice([0.005, 0.05, 0.5]), (J, 3))).astype(dt)
    present = rng.random((R, J)) < 0.97 if tri else np.ones((R, J), bool)
    gts = [{j: gt_xyz[g, j] for j in range(J) if gt_joint[g, j]} for g in range(G)]
    results = [{j: poses[r, j] for j in range(J) if present[r, j]} for r in range(R)]
    return gt_xyz, gt_joint, gt_valid, poses, present, gts, results


def ulps(a, b, dt):
    a, b = np.asarray(a, np.float64), np.asarray(b, np.float64)
    return np.abs(a - b) / np.spacing(np.maximum(np.abs(a), np.abs(b)).astype(dt))


@pytest.mark.parametrize('tri', [False, True])
def test_restated_table_equals_metrics(tri):
    """The table of harness/assignment.py against Metrics' own (a one-body, one-detection Metrics frame books the table
    entry itself as acc_err), within 2 ulp; and the whole frame through Metrics books what the restated table with
    assign_bnb's assignment books."""
    common, A = pkg('harness.common'), pkg('harness.assignment')
    params = pkg('parameters').parameters
    J = len(params.joint_list)
    used = np.isin(np.arange(J), params.used_joints)
    rng = np.random.default_rng(3 + tri)
    worst = 0.0
    for _ in range(40):
        G, R = int(rng.integers(1, 6)), int(rng.integers(0, 6))
        gt_xyz, gt_joint, gt_valid, poses, present, gts, results = random_frame(rng, G, R, J, used, tri)
        table, invalid = A.error_table(poses, present, gt_xyz, gt_joint, used)
        for g in range(G):
            for r in range(R):
                m = common.Metrics()
                m.add_frame([gts[g]], [True], [results[r]], triangulation=tri)
                host = m.acc_err if m.n_matching else 0.0
                worst = max(worst, float(ulps(table[g, r], host, np.float64 if tri else np.float32)))
        host = common.Metrics()
        host.add_frame(gts, list(gt_valid), results, triangulation=tri)
        dev = common.DeviceMetrics()
        dev.add_batch(records([(table, invalid, A.assign_bnb(table))]), gt_valid[None], triangulation=tri)
        assert (dev.n_gt, dev.n_poses, dev.n_matching, dev.TP, dev.FP) == (host.n_gt, host.n_poses, host.n_matching, host.TP, host.FP)
        assert abs(dev.acc_err - host.acc_err) <= 1e-12
        if tri:
            want = [any(int(j) in params.used_joints and int(j) not in res for gt in gts for j in gt) for res in results]
            assert list(invalid) == want
    assert worst <= 2.0


def records(frames, pcap=None, gcap=None, status=None):
    """Engine.evaluate's dict (CPU tensors) for frames [(table [G,R], invalid [R], best_p or 'skip' / 'defer')]."""
    B = len(frames)
    pcap = pcap or max([1] + [np.shape(t)[1] for t, _, _ in frames])
    gcap = gcap or max([1] + [np.shape(t)[0] for t, _, _ in frames])
    A = pkg('harness.assignment')
    L = pkg('lib')
    ev = {'table': np.zeros((B, gcap, pcap)), 'assign': np.full((B, pcap), -1, np.int32), 'err': np.zeros((B, pcap)),
          'invalid': np.zeros((B, pcap), np.uint8), 'n_gt': np.zeros(B, np.int32), 'n_res': np.zeros(B, np.int32),
          'status': np.zeros(B, np.int32)}
    for f, (t, inv, best_p) in enumerate(frames):
        if best_p == 'skip':
            ev['status'][f] = L.MPE_EVAL_SKIPPED
            continue
        G, R = np.shape(t)
        ev['n_gt'][f], ev['n_res'][f] = G, R
        ev['table'][f, :G, :R] = t
        ev['invalid'][f, :R] = inv
        if best_p == 'defer':
            ev['status'][f] = L.MPE_EVAL_OVER_BUDGET
            continue
        ev['assign'][f, :R], ev['err'][f, :R] = A.frame_records(t, best_p)
    return {k: torch.from_numpy(v) for k, v in ev.items()}


@pytest.mark.parametrize('tri', [False, True])
def test_device_metrics_report_equals_metrics_report(tri, capsys):
    """DeviceMetrics fed the host's records (the reference loop's assignment on Metrics' arithmetic) prints and returns
    exactly what Metrics does, over batches with skipped frames, invalid GT bodies, invalid detections, G > R, R = 0
    and frames the device declined (finished by assign_bnb)."""
    common, A = pkg('harness.common'), pkg('harness.assignment')
    params = pkg('parameters').parameters
    J = len(params.joint_list)
    used = np.isin(np.arange(J), params.used_joints)
    rng = np.random.default_rng(7 + tri)
    host, dev = common.Metrics(), common.DeviceMetrics()
    for _ in range(12):
        batch, valids = [], []
        for f in range(int(rng.integers(1, 9))):
            G, R = int(rng.integers(1, 6)), int(rng.integers(0, 7))
            gt_xyz, gt_joint, gt_valid, poses, present, gts, results = random_frame(rng, G, R, J, used, tri)
            if rng.random() < 0.1:
                batch.append((np.zeros((0, 0)), np.zeros(0, bool), 'skip'))
            else:
                host.add_frame(gts, list(gt_valid), results, triangulation=tri)
                table, invalid = A.error_table(poses, present, gt_xyz, gt_joint, used)
                best_p = 'defer' if rng.random() < 0.15 else reference_assignment(table)
                batch.append((table, invalid, best_p))
            valids.append(np.pad(gt_valid, (0, 8 - G)))
        dev.add_batch(records(batch, gcap=8), np.array(valids), triangulation=tri)
    capsys.readouterr()
    out_h = host.report()
    text_h = capsys.readouterr().out
    out_d = dev.report()
    text_d = capsys.readouterr().out
    assert host.n_matching > 0
    assert out_d == out_h and text_d == text_h
    assert np.float64(dev.acc_err).tobytes() == np.float64(host.acc_err).tobytes()


def _synthetic_gt_frames(rng, base):
    out = []
    for k in range(20):
        fr = copy.deepcopy(base[k % len(base)])
        bodies = []
        for _ in range(int(rng.integers(0, 7))):
            body = {str(j): list(rng.uniform(-300, 300, 3)) for j in range(19) if rng.random() < 0.8}
            if rng.random() < 0.7:
                body['-1'] = [0.0, 0.0, 0.0]
            bodies.append(body)
        for c in fr:
            fr[c][3] = bodies if c == list(fr)[k % len(fr)] else bodies[:1]
        out.append(fr)
    return out


def test_pack_ground_truth_is_ground_truth():
    common = pkg('harness.common')
    calib = pkg('calibration')
    params = pkg('parameters').parameters
    hd = os.path.join(GOLDEN, 'harness')
    with open(os.path.join(hd, 'syn_pinning_test.json')) as fh:
        frames = json.load(fh)
    T_d1 = torch.from_numpy(calib.load_transform_manager(os.path.join(hd, 'tm_syn_pinning.pickle')).get_transform(
        'root', params.camera_names[1])).type(torch.float32)
    T_i1 = torch.from_numpy(calib.Calibration(params).T_i32[1])
    rng = np.random.default_rng(11)
    for fs in (frames, _synthetic_gt_frames(rng, frames)):
        packed = common.pack_ground_truth(fs, [T_d1] * len(fs), T_i1)
        n_empty = 0
        for f, frame in enumerate(fs):
            gt = common.ground_truth(frame, T_d1, T_i1)
            if gt is None:
                assert packed['n'][f] == 0
                n_empty += 1
                continue
            bodies, valid = gt
            assert packed['n'][f] == len(bodies)
            assert list(packed['valid'][f, :len(bodies)]) == [int(v) for v in valid]
            for b, body in enumerate(bodies):
                assert sorted(np.flatnonzero(packed['joint'][f, b])) == sorted(body)
                for j, xyz in body.items():
                    assert packed['xyz'][f, b, j].tobytes() == np.asarray(xyz, np.float32).tobytes()
        if fs is not frames:
            assert n_empty > 0


def test_eval_symbol_in_header_and_binding():
    L = pkg('lib')
    with open(os.path.join(ROOT, 'include', 'mpe.h')) as fh:
        hdr = fh.read()
    assert re.search(r'\bint mpe_eval_batch\(mpe_ctx \*ctx, void \*stream, const mpe_eval_args \*a\);', hdr)
    assert 'mpe_eval_batch' in L.SYMBOLS
    names = [n for n, _ in L.mpe_eval_args._fields_]
    body = hdr[:hdr.index('} mpe_eval_args;')].rsplit('typedef struct {', 1)[1]
    assert re.findall(r'\b(d_\w+|n_frames|pcap|n_joints|gcap|pose_f64|joint_flags|used_joint_mask)\b', re.sub(r'/\*.*?\*/', '', body, flags=re.S)) == names


def test_device_metrics_flag_is_opt_in():
    common = pkg('harness.common')
    assert common.build_parser('x').parse_args([]).device_metrics is False
    assert common.build_parser('x').parse_args(['--device-metrics']).device_metrics is True
