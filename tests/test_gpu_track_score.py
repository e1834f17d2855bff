"""GPU: mpe_track_score_batch / _result (csrc/track_score.hip, csrc/assign_int.h) against answers the rule alone decides
and, exactly on every output, against the numpy statement (harness/track_score.py); chunk invariance, the structure of a
call (launches, no synchronisation), the error codes, the composition with mpe_eval_batch and the two trackers, and the
harness's --track-score."""
import ctypes as C
import importlib
import types

import numpy as np
import pytest
import torch

import track_score_cases as tsc
from conftest import pkg

pytestmark = pytest.mark.gpu

CASES = tsc.hand_made()
OUT = ('frame_counts', 'match_tid')


@pytest.fixture(scope='module')
def eng():
    e = pkg('pipeline').Engine(pkg('parameters').parameters, max_frames=32, max_persons_per_camera=4)
    yield e
    e.close()


def dev(a):
    return torch.from_numpy(np.ascontiguousarray(a)).cuda()


def scorer(eng, c, **kw):
    return eng.track_scorer('tri' if c.joint_flags else 'mlp', threshold_mm=c.threshold_mm, gid_cap=c.gid_cap, tid_cap=c.tid_cap,
                            max_frames=kw.get('max_frames', 40), gcap=c.cap, pcap=c.cap)


def tensors(eng, c, a, skip):
    flags = np.repeat(a['flags'][:, :, :1], eng.J, 2) if c.joint_flags else a['flags']        # the joint flags are not read
    ev = {k: dev(a[k]) for k in ('assign', 'err', 'invalid', 'n_res', 'n_gt')}
    return (ev, dev(flags), dev(a['n_persons']), dev(a['track_ids']), dev(a['gt_ids']), dev(a['gt_valid'])), \
        None if skip is None else dev(skip)


def update(eng, ts, c, a, skip):
    args, sk = tensors(eng, c, a, skip)
    out = ts.update(*args, skip=sk)
    torch.cuda.synchronize()
    return {k: out[k].cpu().numpy() for k in OUT}


def on_device(eng, c, chunks=(), ts=None):
    own = ts is None
    ts = ts or scorer(eng, c)
    try:
        frames = tsc.in_chunks(lambda a, skip: update(eng, ts, c, a, skip), c, chunks)
        return frames, ts.result(), ts.read_state()
    finally:
        if own:
            ts.close()


def in_numpy(c, chunks=()):
    ref = pkg('harness.track_score').TrackScoreRef(c.threshold_mm, c.gid_cap, c.tid_cap)
    frames = tsc.in_chunks(lambda a, skip: ref.update(joint_flags=c.joint_flags, skip=skip, **a), c, chunks)
    return frames, ref.result(), ref.state()


@pytest.mark.parametrize('name', sorted(CASES))
def test_known_answers(eng, name):
    c = CASES[name]
    frames, result, state = on_device(eng, c)
    tsc.check(result, frames, c, name)
    tsc.same(frames, result, state, *in_numpy(c), what=name)


@pytest.mark.parametrize('joint_flags', [0, 1])
@pytest.mark.parametrize('seed', [1, 2, 3])
def test_random_sequences(eng, seed, joint_flags):
    """births, deaths, gaps, row permutations, ignore rows, -1 track ids, track ids in the thousands with tid_cap 4096,
    ids at and over both caps, one identity on two rows, skipped frames"""
    c = tsc.random_sequence(seed, joint_flags)
    got, ref = on_device(eng, c), in_numpy(c)
    assert ref[1]['tp'] > 0 and ref[1]['idsw'] > 0 and ref[2]['pred_count'][1000:].any()
    tsc.same(*got, *ref, what='seed %d' % seed)


@pytest.mark.parametrize('joint_flags', [0, 1])
def test_chunk_invariance_and_reset(eng, joint_flags):
    c = tsc.random_sequence(7 + joint_flags, joint_flags)
    ts = scorer(eng, c)
    try:
        whole = on_device(eng, c, ts=ts)
        tsc.same(*whole, *in_numpy(c), what='one call')
        for chunks in ((1, 7), (1,) * 39, (0, 13, 0, 13)):          # a call without frames changes nothing
            ts.reset()
            tsc.same(*on_device(eng, c, chunks, ts=ts), *whole, what=str(chunks[:4]))
        again = on_device(eng, c, ts=ts)                           # no reset: the totals go on
        assert again[1]['frames'] == 2 * whole[1]['frames'] and again[1]['tp'] == 2 * whole[1]['tp']
    finally:
        ts.close()


def test_launches_do_not_grow_with_frames_and_nothing_waits(eng):
    """The structure of a call: three kernels for 1 frame and for 40, and a call that returns while work queued before it
    is still running (it waits for nothing, so it cannot have read anything back or allocated with a synchronising call)."""
    c = tsc.random_sequence(11, 0)
    ts = scorer(eng, c)
    try:
        counts = []
        for B in (1, 40):
            before = ts.launches()
            got = update(eng, ts, c, c.arrays(0, B), c.skip[:B])
            counts.append(ts.launches() - before)
            ts.reset()
        assert counts == [3, 3], counts
        args, sk = tensors(eng, c, c.arrays(), c.skip)
        x = torch.randn((4096, 4096), device='cuda')
        torch.cuda.synchronize()
        for _ in range(40):                                          # some tens of milliseconds of queued work
            x = torch.mm(x, x).mul_(1e-4)
        busy = torch.cuda.Event()
        busy.record()
        out = ts.update(*args, skip=sk)
        still_running = not busy.query()
        torch.cuda.synchronize()
        assert still_running
        assert all(np.array_equal(out[k].cpu().numpy(), got[k]) for k in OUT)
        tsc.same(got, ts.result(), ts.read_state(), *in_numpy(c))
    finally:
        ts.close()


def test_errors_leave_the_state_usable(eng):
    L = pkg('lib')
    st = C.c_void_p()
    for sizes, code in (((129, 4, 16, 64, 8), -2), ((4, 129, 16, 64, 8), -2), ((4, 4, 2049, 2048, 8), -2), ((4, 4, 0, 64, 8), -1),
                        ((4, 4, 16, 64, 0), -1)):
        assert eng.lib.mpe_track_score_create(eng.ctx, *sizes, C.byref(st)) == code and not st.value, sizes
    assert eng.lib.mpe_track_score_create(eng.ctx, 4, 4, 2048, 2048, 8, C.byref(st)) == 0                 # 2^22 itself fits
    assert eng.lib.mpe_track_score_destroy(eng.ctx, st) == 0
    with pytest.raises(ValueError):
        eng.track_scorer('mlp', threshold_mm=0.)
    with pytest.raises(ValueError):
        eng.track_scorer('gt')
    c = CASES['miss_same_track']
    ts = scorer(eng, c, max_frames=2)
    try:
        first = update(eng, ts, c, c.arrays(0, 2), None)
        (ev, flags, n_persons, ids, gt_ids, gt_valid), _ = tensors(eng, c, c.arrays(2, 3), None)
        counts, mtid = torch.empty((1, 4), dtype=torch.int32, device='cuda'), torch.empty((1, 4), dtype=torch.int32, device='cuda')
        status = torch.zeros((1,), dtype=torch.int32, device='cuda')

        def args(**kw):
            a = L.mpe_track_score_args()
            a.n_frames, a.pcap, a.gcap, a.joint_flags, a.threshold_mm = 1, 4, 4, 0, 150.
            a.d_flags, a.d_n_persons, a.d_track_id = flags.data_ptr(), n_persons.data_ptr(), ids.data_ptr()
            a.d_assign, a.d_err, a.d_invalid = ev['assign'].data_ptr(), ev['err'].data_ptr(), ev['invalid'].data_ptr()
            a.d_n_res, a.d_n_gt, a.d_gt_id, a.d_gt_valid = ev['n_res'].data_ptr(), ev['n_gt'].data_ptr(), gt_ids.data_ptr(), gt_valid.data_ptr()
            a.d_frame_counts, a.d_match_tid, a.d_status = counts.data_ptr(), mtid.data_ptr(), status.data_ptr()
            for k, v in kw.items():
                setattr(a, k, v)
            return a
        before = ts.launches()
        for bad, word in (({'pcap': 5}, b'pcap 5'), ({'gcap': 3}, b'gcap 3'), ({'joint_flags': 2}, b'joint_flags 2'),
                          ({'n_frames': -1}, b'n_frames -1'), ({'threshold_mm': 0.}, b'threshold_mm 0'), ({'threshold_mm': -150.}, b'-150'),
                          ({'threshold_mm': float('nan')}, b'nan'), ({'d_gt_id': None}, b'NULL')):
            assert eng.lib.mpe_track_score_batch(eng.ctx, None, ts.state, C.byref(args(**bad))) == -1, bad
            assert word in eng.lib.mpe_last_error(eng.ctx), (bad, eng.lib.mpe_last_error(eng.ctx))
        assert eng.lib.mpe_track_score_batch(eng.ctx, None, ts.state, C.byref(args(n_frames=3))) == -2                # max_frames is 2
        assert b'3 frames' in eng.lib.mpe_last_error(eng.ctx)
        assert eng.lib.mpe_track_score_batch(eng.ctx, None, ts.state, C.byref(args(n_frames=0, d_assign=None))) == 0
        assert ts.launches() == before
        with pytest.raises(ValueError):
            ts.update(ev, flags, n_persons, ids.long(), gt_ids, gt_valid)
        with pytest.raises(ValueError):
            ts.update(ev, flags, n_persons, ids, gt_ids[:, :3].contiguous(), gt_valid)
        # the recording goes on as if nothing had been; d_invalid may be NULL
        assert eng.lib.mpe_track_score_batch(eng.ctx, None, ts.state, C.byref(args(d_invalid=None))) == 0
        torch.cuda.synchronize()
        frames = {'frame_counts': np.concatenate([first['frame_counts'], counts.cpu().numpy()]),
                  'match_tid': np.concatenate([first['match_tid'], mtid.cpu().numpy()])}
        tsc.check(ts.result(), frames, c)
        assert int(status.item()) == 0
    finally:
        ts.close()


def walk(eng, removed, seed=0):
    """Three GT persons on straight lines for 20 frames; the detections are the GT moved by 1 cm, rows shuffled per frame,
    without the (frame, person) pairs in `removed`.  Through the real kernels: Tracker('mlp'), Engine.evaluate,
    Tracker('gt'), TrackScore.  -> result()"""
    rng = np.random.RandomState(seed)
    B, G, P, J, max_gap = 20, 4, eng.pcap, eng.J, 2
    shape = (rng.rand(J, 3) * 0.4).astype(np.float32)
    start = np.array([[-2., 0., 1.], [0., 1.5, 1.], [2., -1., 1.]], np.float32)
    step = np.array([[0.02, 0.01, 0.], [-0.01, 0.02, 0.], [0.01, -0.02, 0.]], np.float32)
    gt = {'xyz': np.zeros((B, G, J, 3), np.float32), 'joint': np.zeros((B, G, J), np.uint8), 'valid': np.zeros((B, G), np.uint8),
          'n': np.full(B, 3, np.int32)}
    poses, flags, n_persons = np.zeros((B, P, J, 3), np.float32), np.zeros((B, P), np.uint8), np.zeros(B, np.int32)
    for f in range(B):
        for g in range(3):
            gt['xyz'][f, g] = start[g] + np.float32(f) * step[g] + shape
        gt['joint'][f, :3], gt['valid'][f, :3] = 1, 1
        here = [g for g in rng.permutation(3) if (f, g) not in removed]
        for p, g in enumerate(here):
            poses[f, p] = gt['xyz'][f, g] + np.array([0.01, 0., 0.], np.float32)
            flags[f, p] = 1
        n_persons[f] = len(here)
    tr, gtr = eng.tracker('mlp', max_gap=max_gap, gate=0.5), eng.tracker('gt', max_gap=max_gap, gate=0.5, pcap=G)
    ts = eng.track_scorer('mlp', gcap=G, max_frames=B)
    try:
        p, fl, n = dev(poses), dev(flags), dev(n_persons)
        ids = tr.update(p, fl, n)['ids']
        ev = eng.evaluate(types.SimpleNamespace(n_frames=B), p, fl, n, gt, 'mlp', skip=np.zeros(B, np.uint8))
        gt_ids = gtr.update(dev(gt['xyz']), dev(gt['joint']), dev(gt['n']))['ids']
        out = ts.update(ev, fl, n, ids, gt_ids, dev(gt['valid']))
        torch.cuda.synchronize()
        assert np.array_equal(gt_ids.cpu().numpy()[:, :3], np.tile(np.arange(3, dtype=np.int32), (B, 1)))       # the GT keeps its identities
        assert (ev['status'].cpu().numpy() == 0).all()
        r = ts.result()
        assert int(out['frame_counts'].cpu().numpy()[:, 2].sum()) == r['fn']
        return r
    finally:
        for o in (tr, gtr, ts):
            o.close()


def test_composition_on_real_kernels(eng):
    max_gap = 2
    r = walk(eng, set())
    assert (r['tp'], r['fp'], r['fn'], r['idsw'], r['frag'], r['idtp'], r['mt']) == (60, 0, 0, 0, 0, 60, 3) and r['mota'] == 1.0
    assert 9.9 < r['motp_mm'] < 10.1                                # the 1 cm offset, up to float32 rounding of the poses
    r = walk(eng, {(8 + k, 1) for k in range(max_gap)})            # taken up again: the same track
    assert (r['idsw'], r['frag'], r['fn'], r['fp'], r['tp'], r['n_tracks']) == (0, 1, max_gap, 0, 60 - max_gap, 3)
    r = walk(eng, {(8 + k, 1) for k in range(max_gap + 2)})        # lost: a new track
    assert (r['idsw'], r['frag'], r['fn'], r['fp'], r['n_tracks']) == (1, 1, max_gap + 2, 0, 4)
    assert r['idtp'] == 60 - (max_gap + 2) - 8                     # identity 1 keeps the longer of its two tracks (8 frames lost)


def test_harness_track_score_line(capsys, monkeypatch):
    """metrics_from_model --synthetic 24 --random-weights --teacher-scores --track-score: the new line, totals that add
    up, the per-frame counts that add up to them, and the --track line as without the flag."""
    m = importlib.import_module('3d_multi_pose_estimator_amd.harness.metrics_from_model')
    P = pkg('pipeline')
    seen = []
    real_update = P.TrackScore.update

    def recording_update(self, *a, **kw):
        out = real_update(self, *a, **kw)
        torch.cuda.synchronize()
        seen.append(out['frame_counts'].cpu().numpy())
        return out
    monkeypatch.setattr(P.TrackScore, 'update', recording_update)
    argv = ['--synthetic', '24', '--random-weights', '--teacher-scores', '--batch', '16']

    def lines(extra):
        capsys.readouterr()
        out = m.main(argv + extra)
        return out, capsys.readouterr().out.splitlines()
    plain, text = lines(['--track'])
    assert 'track_score' not in plain and not seen and not any(ln.startswith('Track score') for ln in text)
    track_line = [ln for ln in text if ln.startswith('Tracks (')]
    out, text = lines(['--track-score'])
    r = out['track_score']
    assert text[-1] == pkg('harness.track_score').report_line(r, 150.) and text[-1].startswith('Track score (150 mm): MOTA ')
    assert [ln for ln in text if ln.startswith('Tracks (')] == track_line and len(track_line) == 1 and out['tracks'] == plain['tracks']
    assert len(seen) == 2                                            # one scorer call per batch
    per_frame = np.concatenate(seen).astype(np.int64).sum(0)
    assert r['frames'] == out['n_data'] and r['n_gt'] > 0 and r['n_pred'] > 0
    assert r['tp'] + r['fn'] == r['n_gt'] and r['tp'] + r['fp'] == r['n_pred']
    assert per_frame[0] + per_frame[2] == r['n_gt'] and per_frame[0] + per_frame[1] == r['n_pred']
    assert tuple(per_frame) == (r['tp'], r['fp'], r['fn'], r['idsw'])
    assert r['idtp'] <= r['tp'] and r['status'] == 0
