"""GPU: mpe_track_batch (csrc/track.hip) against written-out ids and against its numpy statement (harness/tracking.py),
exactly: ids, gaps and the bits of the costs; chunk invariance, the structure of a call (launches, no synchronisation),
the tracker behind match + triangulate, and the harness's --track."""
import ctypes as C
import importlib
import json
import os

import numpy as np
import pytest
import torch

import track_cases as tc
from conftest import GOLDEN, env, harness_model_files, pkg

pytestmark = pytest.mark.gpu

CASES = tc.hand_made()


@pytest.fixture(scope='module')
def eng():
    e = pkg('pipeline').Engine(pkg('parameters').parameters, max_frames=32, max_persons_per_camera=4)
    assert e.J == tc.J and list(e.params.used_joints) == tc.USED
    yield e
    e.close()


def dev(a):
    return torch.from_numpy(np.ascontiguousarray(a)).cuda()


def update(tr, poses, flags, n_persons):
    out = tr.update(dev(poses), dev(flags), dev(n_persons))
    torch.cuda.synchronize()
    return {k: v.cpu().numpy() for k, v in out.items()}


def same(got, want, what=''):
    """every row of every frame: ids, gaps, and the costs bit for bit"""
    assert got['ids'].shape == want['ids'].shape
    bad = np.flatnonzero((got['ids'] != want['ids']).any(axis=1) | (got['gap'] != want['gap']).any(axis=1))
    assert not len(bad), (what, bad[:5].tolist(), got['ids'][bad[:2]].tolist(), want['ids'][bad[:2]].tolist())
    assert got['cost'].tobytes() == want['cost'].tobytes(), what


def oracle(poses, flags, n_persons, mode, max_gap, gate=0.5):
    return pkg('harness.tracking').track_sequence(poses, flags, n_persons, mode, tc.USED, gate, max_gap)


@pytest.mark.parametrize('name', sorted(CASES))
def test_known_answers(eng, name):
    seq, max_gap, gate, want = CASES[name]
    tr = eng.tracker(seq.mode, max_gap=max_gap, gate=gate, pcap=4)
    try:
        got = update(tr, seq.poses, seq.flags, seq.n_persons)
    finally:
        tr.close()
    assert np.array_equal(got['ids'], want), (got['ids'].tolist(), want.tolist())
    ref = oracle(seq.poses, seq.flags, seq.n_persons, seq.mode, max_gap, gate)
    same(got, ref, name)
    assert got['issued'].tolist() == [ref['issued']]


@pytest.mark.parametrize('max_gap', [0, 1, 3])
@pytest.mark.parametrize('tri', [False, True])
def test_random_sequences(eng, tri, max_gap):
    poses, flags, n_persons = tc.random_sequence(40 + tri, tri)
    assert poses.shape[:2] == (40, 6) and n_persons.min() == 0 and n_persons.max() == 6
    mode = 'tri' if tri else 'mlp'
    tr = eng.tracker(mode, max_gap=max_gap, gate=0.5, pcap=6)
    try:
        got = update(tr, poses, flags, n_persons)
    finally:
        tr.close()
    ref = oracle(poses, flags, n_persons, mode, max_gap)
    same(got, ref)
    assert got['issued'].tolist() == [ref['issued']] and ref['issued'] > 4
    assert (ref['gap'] > 0).sum() > 60 and (max_gap == 0 or (ref['gap'] > 1).any())


@pytest.mark.parametrize('n', [63, 64, 65, 128])
def test_wave_edges(eng, n):
    """n detections per frame at pcap 128: rows and columns on either side of one wave, and the whole table."""
    tri = n % 2 == 0
    poses, flags, n_persons = tc.lattice_sequence(n, n, tri)
    mode = 'tri' if tri else 'mlp'
    tr = eng.tracker(mode, max_gap=1, gate=0.5, pcap=128)
    try:
        got = update(tr, poses, flags, n_persons)
    finally:
        tr.close()
    ref = oracle(poses, flags, n_persons, mode, 1)
    same(got, ref)
    assert ref['issued'] == n and (ref['gap'][1:, :n] == 1).all()          # everybody is followed, the twins included


def test_capacity(eng):
    L = pkg('lib')
    st = C.c_void_p()
    assert eng.lib.mpe_track_create(eng.ctx, 129, tc.J, 2, 0, C.byref(st)) == -2 and not st.value
    assert b'129' in eng.lib.mpe_last_error(eng.ctx)
    assert eng.lib.mpe_track_create(eng.ctx, 128, tc.J, 16, 0, C.byref(st)) == -2 and not st.value
    tr = eng.tracker('mlp', pcap=4)
    try:
        a = L.mpe_track_args()
        a.n_frames, a.pcap, a.n_joints, a.pose_f64, a.gate = 0, 4, tc.J, 1, 0.5          # f64 poses, the state holds f32
        assert eng.lib.mpe_track_batch(eng.ctx, None, tr.state, C.byref(a)) == -1
        assert b'pose_f64' in eng.lib.mpe_last_error(eng.ctx)
        a.pose_f64, a.pcap = 0, 5
        assert eng.lib.mpe_track_batch(eng.ctx, None, tr.state, C.byref(a)) == -1
        with pytest.raises(ValueError):
            tr.update(torch.zeros((1, 4, tc.J, 3), dtype=torch.float64).cuda(), torch.zeros((1, 4), dtype=torch.uint8).cuda(),
                      torch.zeros(1, dtype=torch.int32).cuda())
    finally:
        tr.close()


@pytest.mark.parametrize('tri', [False, True])
def test_chunk_invariance(eng, tri):
    poses, flags, n_persons = tc.random_sequence(5 + tri, tri, B=37, away=tc.AWAY)
    mode = 'tri' if tri else 'mlp'
    ref = oracle(poses, flags, n_persons, mode, 3)
    tr = eng.tracker(mode, max_gap=3, gate=0.5, pcap=6)
    try:
        whole = update(tr, poses, flags, n_persons)
        same(whole, ref, 'one call')
        for chunks in (tc.CHUNKS, (1,) * 37):
            tr.reset()
            issued = []

            def step(p, f, n):
                out = update(tr, p, f, n)
                issued.append(int(out['issued'][0]))
                if len(issued) == 3:                         # a call without frames changes nothing
                    nothing = update(tr, p[:0], f[:0], n[:0])
                    assert nothing['ids'].shape == (0, 6) and nothing['issued'].tolist() == [issued[-1]]
                return out
            same(tc.in_chunks(step, poses, flags, n_persons, chunks), whole, str(chunks[:3]))
            assert issued[-1] == ref['issued'] and issued == sorted(issued)
    finally:
        tr.close()


def test_launches_do_not_grow_with_frames_and_nothing_waits(eng):
    """The structure of a call: max_gap + 7 kernels for 8 frames and for 200, and a call that returns while work queued
    before it is still running (it waits for nothing)."""
    tr = eng.tracker('mlp', max_gap=2, gate=0.5, pcap=6)
    try:
        counts = []
        for B in (8, 200):
            poses, flags, n_persons = tc.random_sequence(3, False, B=B)
            before = tr.launches()
            got = update(tr, poses, flags, n_persons)
            counts.append(tr.launches() - before)
            tr.reset()
            if B == 200:
                same(got, oracle(poses, flags, n_persons, 'mlp', 2))
        assert counts == [2 + 7, 2 + 7], counts
        p, f, n = dev(poses), dev(flags), dev(n_persons)
        x = torch.randn((4096, 4096), device='cuda')
        torch.cuda.synchronize()
        for _ in range(40):                                  # some tens of milliseconds of queued work
            x = torch.mm(x, x).mul_(1e-4)
        busy = torch.cuda.Event()
        busy.record()
        out = tr.update(p, f, n)
        still_running = not busy.query()
        torch.cuda.synchronize()
        assert still_running
        assert np.array_equal(out['ids'].cpu().numpy(), got['ids'])
    finally:
        tr.close()


def test_tracker_behind_match_and_triangulate():
    """24 frames of 3 people walking 2 cm per frame, the skeleton lists of every camera reordered per frame, person 1
    seen by nobody in frames 10-11: with max_gap 2 every body keeps one id, with max_gap 0 person 1 comes back as a new one."""
    e = env()
    syn = pkg('synthetic')
    params, calib = e.params, e.calib
    V, J = len(params.camera_names), len(params.joint_list)
    nf = 2 + V * J * 10
    eng = pkg('pipeline').Engine(params, calib, max_frames=24, max_persons_per_camera=4)
    try:
        eng.load_gat(syn.matcher_gat_state_dict(nf, V, J), syn.gat_params(nf))
        rng = np.random.default_rng(8)
        start = np.array([[-0.8, -1.2, -0.5], [0.0, -1.2, 0.6], [0.8, -1.2, -0.2]])
        heading = np.array([[1.0, 0, 0], [0, 0, -1.0], [-1.0, 0, 0]])
        g = rng.normal(0, 0.12, (3, J, 3))                  # a body: joints spread around its root
        bodies = np.stack([start[:, None] + 0.02 * t * heading[:, None] + g for t in range(24)])          # [24,3,J,3]
        frames = []
        for t in range(24):
            orders = {cam: list(rng.permutation(3)) for cam in params.camera_names}
            frame, _ = syn.frame_from_bodies(calib, t, bodies[t], orders, hidden=(1,) if t in (10, 11) else ())
            frames.append({c: frame[c][:2] for c in frame})
        db = eng.to_device(eng.pack(frames))
        _, persons, n_persons = eng.match(db, want_scores=False)
        poses, jv = eng.triangulate(db, persons, n_persons)
        eng.sync_status()
        h_poses, h_n = poses.cpu().numpy(), n_persons.cpu().numpy()
        assert h_n.tolist() == [3] * 10 + [2] * 2 + [3] * 12
        ids = {}
        for max_gap in (2, 0):
            tr = eng.tracker('tri', max_gap=max_gap, gate=0.5)
            out = tr.update(poses, jv, n_persons)
            torch.cuda.synchronize()
            got = out['ids'].cpu().numpy()
            tr.close()
            same({k: out[k].cpu().numpy() for k in ('ids', 'cost', 'gap')}, oracle(h_poses, jv.cpu().numpy(), h_n, 'tri', max_gap))
            per_body = [[], [], []]
            for t in range(24):
                for b in range(3):
                    if b == 1 and t in (10, 11):
                        continue
                    used = tc.USED
                    d = [np.abs(h_poses[t, p][used] - bodies[t, b][used]).mean() for p in range(h_n[t])]
                    assert min(d) < 0.02
                    per_body[b].append(int(got[t, int(np.argmin(d))]))
            ids[max_gap] = per_body
        for b in range(3):
            assert len(set(ids[2][b])) == 1, (b, ids[2][b])
        assert len({ids[2][b][0] for b in range(3)}) == 3
        assert len(set(ids[0][0])) == 1 and len(set(ids[0][2])) == 1
        assert len(set(ids[0][1][:10])) == 1 and len(set(ids[0][1][10:])) == 1 and ids[0][1][0] != ids[0][1][10]
    finally:
        eng.close()


def test_harness_track_line(tmp_path, capsys):
    """metrics_from_triangulation --track on the committed test file: the same track line whatever --batch is, and every
    other line (the timings apart, which no two runs share) as without the flag."""
    hd = os.path.join(GOLDEN, 'harness')
    with open(os.path.join(hd, 'harness_expected.json')) as fh:
        exp = json.load(fh)
    mdir = harness_model_files(str(tmp_path), exp['inputs'])
    m = importlib.import_module('3d_multi_pose_estimator_amd.harness.metrics_from_triangulation')
    argv = ['--testfiles', os.path.join(hd, exp['inputs']['testfile']), '--tmdir', hd, '--modelsdir', mdir,
            '--datastep', str(exp['inputs']['datastep'])]
    timed = ('Mean time', 'Frames per second')

    def lines(extra):
        capsys.readouterr()
        out = m.main(argv + extra)
        text = capsys.readouterr().out.splitlines()
        return out, [ln for ln in text if not ln.startswith(timed)], [ln for ln in text if ln.startswith(timed)]
    plain, want, want_timed = lines(['--device-metrics', '--batch', '7'])
    tracks = []
    for batch in ('7', '256'):
        out, got, got_timed = lines(['--track', '--batch', batch])
        assert got[-1].startswith('Tracks (gate 0.5 m, gap 2): ') and got[:-1] == want
        assert [ln.rsplit(' ', 1)[0] for ln in got_timed] == [ln.rsplit(' ', 1)[0] for ln in want_timed]
        assert {k: v for k, v in out.items() if k != 'tracks'} == plain
        tracks.append((got[-1], out['tracks']))
    assert tracks[0] == tracks[1]
    assert tracks[0][1]['tracks'] >= 1 and tracks[0][1]['mean_length'] >= 1
