"""CPU: harness/tracking.py, the numpy statement of mpe_track_batch, on hand-made sequences with written-out ids, and the
pieces around it that need no GPU (declarations, flags, the generator for chosen bodies)."""
import os
import re

import numpy as np
import pytest

import track_cases as tc
from conftest import ROOT, calib, pkg  # noqa: F401

CASES = tc.hand_made()


def run(seq, max_gap, gate, state=None):
    T = pkg('harness.tracking')
    return T.track_sequence(seq.poses, seq.flags, seq.n_persons, seq.mode, tc.USED, gate, max_gap, state)


def test_used_joints_are_the_package_s():
    assert list(pkg('parameters').parameters.used_joints) == tc.USED and len(pkg('parameters').parameters.joint_list) == tc.J


@pytest.mark.parametrize('name', sorted(CASES))
def test_hand_made_sequences(name):
    seq, max_gap, gate, want = CASES[name]
    out = run(seq, max_gap, gate)
    assert np.array_equal(out['ids'], want), (out['ids'].tolist(), want.tolist())
    assert out['ids'].dtype == np.int32 and out['gap'].dtype == np.int32 and out['cost'].dtype == np.float64
    det = want >= 0
    assert np.all(out['gap'][~det] == -1) and np.all(out['cost'][~det] == -1.0) and np.all(out['gap'][det] >= 0)
    assert np.all(out['cost'][out['gap'] == 0] == -1.0) and np.all(out['cost'][out['gap'] > 0] >= 0) and np.all(out['cost'][out['gap'] > 0] < gate)
    assert out['issued'] == want.max() + 1


def test_gaps_and_costs_of_the_gap_limit_case():
    seq, max_gap, gate, _ = CASES['gap_limit']
    out = run(seq, max_gap, gate)
    assert out['gap'][3].tolist() == [1, 3, -1, -1] and out['gap'][7].tolist() == [0, 1, -1, -1]
    # 6 cm along x in float32, every joint alike: the mean of 14 equal distances
    d = float(np.float32(0.06)) - 0.0
    tot = 0.0
    for _ in range(14):
        tot = tot + np.sqrt(d * d)
    assert out['cost'][3, 1] == tot / 14


def test_exact_gate():
    for name in ('cost_equals_gate_mlp', 'cost_equals_gate_tri'):
        seq, max_gap, gate, _ = CASES[name]
        assert run(seq, max_gap, gate)['cost'][1].tolist()[:2] == [-1.0, 0.4375]
        assert run(seq, max_gap, 0.5000001)['ids'][1].tolist()[:2] == [0, 1]


def test_nan_never_links():
    seq, max_gap, gate, _ = CASES['swap_rows']
    seq.poses[1, 0, 5, 1] = np.nan
    try:
        out = run(seq, max_gap, gate)
    finally:
        seq.poses[1, 0, 5, 1] = tc.SHAPE[5, 1]
    assert out['ids'][:3].tolist() == [[0, 1, -1, -1], [2, 0, -1, -1], [0, 1, -1, -1]]


@pytest.mark.parametrize('tri', [False, True])
def test_chunks_with_carried_state_give_the_ids_of_one_call(tri):
    T = pkg('harness.tracking')
    poses, flags, n_persons = tc.random_sequence(5 + tri, tri, B=37, away=tc.AWAY)
    mode = 'tri' if tri else 'mlp'
    whole = T.track_sequence(poses, flags, n_persons, mode, tc.USED, 0.5, 3)
    state = [None]

    def step(p, f, n):
        out = T.track_sequence(p, f, n, mode, tc.USED, 0.5, 3, state[0])
        state[0] = out['state']
        return out
    parts = tc.in_chunks(step, poses, flags, n_persons, tc.CHUNKS)
    for k in ('ids', 'gap', 'cost'):
        assert parts[k].tobytes() == whole[k].tobytes(), k
    assert state[0]['issued'] == whole['issued']
    # the sequence does what it is for: links over more than one frame, births late in the sequence, empty and full frames
    assert (whole['gap'] > 1).any() and (whole['gap'][20:] == 0).any() and n_persons.min() == 0 and n_persons.max() == poses.shape[1]
    for b in (1, 2, 7, 23):                                  # a link reaches across every chunk border
        assert any((whole['gap'][f] > f - b).any() for f in range(b, min(b + 4, 37))), b


def test_summary():
    T = pkg('harness.tracking')
    seq, max_gap, gate, _ = CASES['gap_limit']
    out = run(seq, max_gap, gate)
    s = T.TrackSummary()
    s.add(out['ids'][:3], out['gap'][:3])
    s.add(out['ids'][3:], out['gap'][3:])
    assert s.result() == {'tracks': 3, 'mean_length': 11 / 3, 'late_births': 1}


def test_track_symbols_in_header_and_binding():
    L = pkg('lib')
    with open(os.path.join(ROOT, 'include', 'mpe.h')) as fh:
        hdr = fh.read()
    for name in ('mpe_track_create', 'mpe_track_reset', 'mpe_track_destroy', 'mpe_track_batch', 'mpe_track_launches'):
        assert re.search(r'\bint %s\(mpe_ctx \*ctx, ' % name, hdr) and name in L.SYMBOLS
    names = [n for n, _ in L.mpe_track_args._fields_]
    body = hdr[:hdr.index('} mpe_track_args;')].rsplit('typedef struct {', 1)[1]
    assert re.findall(r'\b(d_\w+|n_frames|pcap|n_joints|pose_f64|joint_flags|used_joint_mask|gate)\b', re.sub(r'/\*.*?\*/', '', body, flags=re.S)) == names
    assert (L.MPE_TRACK_MAX_PERSONS, L.MPE_TRACK_MAX_GAP) == tuple(int(re.search(r'#define %s (\d+)' % n, hdr).group(1))
                                                                   for n in ('MPE_TRACK_MAX_PERSONS', 'MPE_TRACK_MAX_GAP'))


def test_track_flags_are_opt_in():
    a = pkg('harness.common').build_parser('x').parse_args([])
    assert (a.track, a.track_gate, a.track_gap) == (False, 0.5, 2)
    a = pkg('harness.common').build_parser('x').parse_args(['--track', '--track-gate', '0.25', '--track-gap', '4'])
    assert (a.track, a.track_gate, a.track_gap) == (True, 0.25, 4)


def test_frames_from_chosen_bodies(calib):
    """synthetic.frame_from_bodies: the wire format of make_frame for given bodies, list order and hidden persons."""
    import json
    syn = pkg('synthetic')
    bodies = np.stack([tc.person(-0.5, -1.2, 0.2), tc.person(0.4, -1.2, -0.3), tc.person(0.0, -1.2, 0.8)])
    cams = calib.params.camera_names
    frame, owner = syn.frame_from_bodies(calib, 3, bodies, orders={cams[0]: [2, 0, 1]}, hidden=(1,))
    assert list(frame) == list(cams) and owner[cams[0]] == [2, 0] and owner[cams[1]] == [0, 2]
    sk = json.loads(frame[cams[0]][0])
    assert len(sk) == 2 and len(sk[0]) > 10 and sk[0]['5'][4] == float(np.float32(0.5)) and sk[1]['5'][4] == float(np.float32(0.3))
    k = calib.index(cams[0])
    uv, _ = syn.project_panoptic(bodies[2].T, calib.K32[k].astype(np.float64), calib.T_d[k], calib.dist[k])
    assert sk[0]['5'][1:3] == [float(uv[0, 5]), float(uv[1, 5])]
    assert len(frame[cams[0]][3]) == 2 and frame[cams[0]][3][0]['5'] == [float(c) * 100.0 for c in bodies[2, 5]]
