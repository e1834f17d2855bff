"""GPU: mpe_relink_batch (csrc/relink.hip) against answers the rule alone decides and, bit for bit on the ids, the link
costs and gaps, the counters and the status, against the numpy statement (harness/relink.py): the hand-made cases, seeded
sequences and a wide case, in one call and in chunks; reset, the structure of a call (two launches whatever the data, no
synchronisation), the error codes, the behavioural case and what it does for the skeleton table, and the harness's
--relink behind match, triangulate and the tracker."""
import ctypes as C
import importlib
import json
import os

import numpy as np
import pytest
import torch

import relink_cases as rc
from conftest import GOLDEN, harness_model_files, pkg

pytestmark = pytest.mark.gpu

CASES = rc.hand_made()
LAUNCHES = 2                                                 # per update: the rows, the walk


@pytest.fixture(scope='module')
def eng():
    e = pkg('pipeline').Engine(pkg('parameters').parameters, max_frames=128, max_persons_per_camera=4)
    assert e.J == rc.J
    yield e
    e.close()


def dev(a):
    return torch.from_numpy(np.ascontiguousarray(a)).cuda()


def relinker(eng, mode, options, pcap, **kw):
    return eng.relinker(mode, pcap=pcap, **dict(options, **kw))


def feed(rl, arrays, chunks=None):
    """the frames through rl.update in one call or in chunks -> the outputs joined, with the counters and the status"""
    chunks = [len(arrays[0])] if chunks is None else chunks
    outs, at = [], 0
    for n in chunks:
        out = rl.update(*(dev(a[at:at + n]) for a in arrays))
        outs.append({k: v.cpu().numpy() for k, v in out.items()})
        at += n
    assert at == len(arrays[0])
    got = {k: np.concatenate([o[k] for o in outs]) for k in ('ids', 'link_cost', 'link_gap')}
    ctr = rl.counters()
    got['counters'], got['status'] = np.array([ctr['births'], ctr['linked'], ctr['over_ids']], np.int64), ctr['status']
    return got


@pytest.mark.parametrize('name', sorted(CASES))
def test_known_answers(eng, name):
    c = CASES[name]
    ref, _ = rc.run_statement(pkg('harness.relink'), c)
    rl = relinker(eng, c.mode, c.options, c.pcap)
    try:
        got = feed(rl, c.arrays())
        rc.same(got, c.want, what=name)
        rc.same(got, ref, what=name)
        rl.reset()
        rc.same(feed(rl, c.arrays(), [1] * len(c.poses)), ref, what=name + ' frame by frame')
    finally:
        rl.close()


def test_a_call_without_frames(eng):
    c = CASES['chain_tri']
    rl = relinker(eng, 'tri', c.options, c.pcap)
    try:
        n = rl.launches()
        out = rl.update(*(dev(a[:0]) for a in c.arrays()))
        assert out['ids'].shape == (0, c.pcap) and rl.launches() == n
        rc.same(feed(rl, c.arrays(), [3, 0, len(c.poses) - 3, 0]), c.want)
    finally:
        rl.close()


@pytest.mark.parametrize('tri', [False, True])
@pytest.mark.parametrize('seed', [3, 4, 5])
def test_random_sequences_chunks_and_reset(eng, seed, tri):
    R = pkg('harness.relink')
    arrays = rc.random_sequence(seed, tri)
    mode = 'tri' if tri else 'mlp'
    for options in (rc.RANDOM_OPTIONS, dict(rc.RANDOM_OPTIONS, reach_m=1.0, reach_per_frame_m=0.05, tid_cap=4096)):
        ref, _ = rc.statement(R, arrays, mode, options)
        rl = relinker(eng, mode, options, 6)
        try:
            rc.same(feed(rl, arrays), ref, what=(seed, mode, 'one call'))
            for chunks in (rc.CHUNKS, (1,) * 40):
                rl.reset()
                zero = rl.counters()
                assert zero == {'births': 0, 'linked': 0, 'over_ids': 0, 'status': 0}
                rc.same(feed(rl, arrays, chunks), ref, what=(seed, mode, chunks[:3]))
        finally:
            rl.close()
        assert ref['counters'][1] >= 1 and ref['counters'][0] >= 3


@pytest.mark.parametrize('tri', [False, True])
def test_wide_case(eng, tri):
    """80 births against 160 records in one frame: more than one wave of rows, the record scan and the reductions across
    the whole workgroup, 80 rounds of the greedy"""
    R = pkg('harness.relink')
    arrays = rc.wide_sequence(11 + tri, tri)
    mode = 'tri' if tri else 'mlp'
    n = arrays[0].shape[1]
    ref, _ = rc.statement(R, arrays, mode, rc.WIDE_OPTIONS)
    assert ref['counters'].tolist() == [n, n, 0] and n > 64
    rl = relinker(eng, mode, rc.WIDE_OPTIONS, n)
    try:
        rc.same(feed(rl, arrays), ref, what='one call')
        rl.reset()
        rc.same(feed(rl, arrays, (5, 2, 3)), ref, what='chunks')
    finally:
        rl.close()


def test_two_launches_and_nothing_waits(eng):
    """The structure of a call: two kernels for 1 frame and for 40, with and without births and links in them, and an
    update that returns while work queued before it is still running (it waits for nothing)."""
    R = pkg('harness.relink')
    arrays = rc.random_sequence(4, False)
    ref, _ = rc.statement(R, arrays, 'mlp', rc.RANDOM_OPTIONS)
    rl = relinker(eng, 'mlp', rc.RANDOM_OPTIONS, 6)
    try:
        quiet = [a[:1] * 0 for a in arrays]                  # a frame without a detection
        for part in (quiet, [a[:1] for a in arrays], arrays):
            before = rl.launches()
            rl.update(*(dev(a) for a in part))
            assert rl.launches() - before == LAUNCHES
            rl.reset()
            assert rl.launches() - before == LAUNCHES
        p, f, n, i = (dev(a) for a in arrays)
        x = torch.randn((4096, 4096), device='cuda')
        torch.cuda.synchronize()
        for _ in range(40):                                  # some tens of milliseconds of queued work
            x = torch.mm(x, x).mul_(1e-4)
        busy = torch.cuda.Event()
        busy.record()
        out = rl.update(p, f, n, i)
        still_running = not busy.query()
        torch.cuda.synchronize()
        assert still_running
        assert out['ids'].cpu().numpy().tobytes() == ref['ids'].tobytes() and out['link_cost'].cpu().numpy().tobytes() == ref['link_cost'].tobytes()
    finally:
        rl.close()


def test_errors_leave_the_state_usable(eng):
    L = pkg('lib')
    lib, st = eng.lib, C.c_void_p()
    bones = (C.c_int32 * 4)(17, 0, 0, 1)

    def create(bones=bones, **kw):
        cfg = L.mpe_relink_config()
        vals = dict(pcap=4, n_joints=rc.J, pose_f64=0, tid_cap=8, n_bones=2, max_frames=16, min_gap=4, max_gap=150, min_samples=5, min_bones=2,
                    used_joint_mask=1, joint_mask=0xFFFFFFFF, gate_m=0.02, max_bone_m=1.0, reach_m=0.0, reach_per_frame_m=0.0)
        vals.update(kw)
        for k, v in vals.items():
            setattr(cfg, k, v)
        cfg.bones = None if bones is None else C.cast(bones, L.c_i32p)
        code = lib.mpe_relink_create(eng.ctx, C.byref(cfg), C.byref(st))
        assert code == 0 or not st.value
        return code, lib.mpe_last_error(eng.ctx)
    assert lib.mpe_relink_create(eng.ctx, None, C.byref(st)) == -1
    for kw, word in (({'pcap': 129}, b'pcap 129'), ({'tid_cap': 4097}, b'tid_cap 4097'), ({'max_frames': (1 << 23) + 1}, b'max_frames')):
        code, why = create(**kw)
        assert code == -2 and word in why, (kw, why)
    for kw, word in (({'n_bones': 0}, b'n_bones 0'), ({'n_bones': 33}, b'n_bones 33'), ({'tid_cap': 0}, b'tid_cap 0'), ({'n_joints': 33}, b'joints 33'),
                     ({'pose_f64': 2}, b'pose_f64 2'), ({'pcap': 0}, b'pcap 0'), ({'max_frames': 0}, b'max_frames 0'), ({'gate_m': 0.0}, b'gate_m 0'),
                     ({'gate_m': float('nan')}, b'nan'), ({'max_bone_m': float('inf')}, b'inf'), ({'reach_m': -1.0}, b'reach_m -1'),
                     ({'reach_per_frame_m': float('nan')}, b'nan'), ({'min_gap': 0}, b'min_gap 0'), ({'min_gap': 5, 'max_gap': 4}, b'max_gap 4'),
                     ({'max_gap': (1 << 30) + 1}, b'max_gap'), ({'min_samples': 0}, b'min_samples 0'), ({'min_bones': 0}, b'min_bones 0'),
                     ({'min_bones': 3}, b'min_bones 3'), ({'bones': (C.c_int32 * 4)(17, 0, 5, 5)}, b'(5, 5)'),
                     ({'bones': (C.c_int32 * 4)(17, 0, 0, 18)}, b'(0, 18)'), ({'bones': None}, b'NULL')):
        code, why = create(**kw)
        assert code == -1 and word in why, (kw, why)
    for bad in (dict(bones=[(0, 0)]), dict(tid_cap=0), dict(tid_cap=4097), dict(mode='gt'), dict(gate_m=0.0), dict(min_gap=0), dict(max_frames=0),
                dict(reach_m=float('nan')), dict(no_such_option=1)):
        with pytest.raises(ValueError):
            eng.relinker(**dict(dict(mode='mlp'), **bad))
    c = CASES['chain_mlp']
    rl = relinker(eng, 'mlp', c.options, c.pcap, max_frames=8)
    try:
        p, f, n, i = (dev(a) for a in c.arrays())
        ids = torch.empty((8, c.pcap), dtype=torch.int32, device='cuda')
        cost, gap = torch.empty((8, c.pcap), dtype=torch.float64, device='cuda'), torch.empty((8, c.pcap), dtype=torch.int32, device='cuda')

        def args(**kw):
            a = L.mpe_relink_args()
            a.n_frames, a.pcap, a.n_joints, a.pose_f64, a.joint_flags = 8, c.pcap, rc.J, 0, 0
            a.d_poses, a.d_flags, a.d_n_persons, a.d_track_id = p.data_ptr(), f.data_ptr(), n.data_ptr(), i.data_ptr()
            a.d_ids, a.d_link_cost, a.d_link_gap = ids.data_ptr(), cost.data_ptr(), gap.data_ptr()
            for k, v in kw.items():
                setattr(a, k, v)
            return a
        before = rl.launches()
        for bad, word in (({'pose_f64': 1}, b'pose_f64 1'), ({'pcap': 6}, b'pcap 6'), ({'n_joints': rc.J - 1}, b'joints 17'),
                          ({'joint_flags': 2}, b'joint_flags 2'), ({'n_frames': -1}, b'n_frames -1'), ({'d_track_id': None}, b'NULL'),
                          ({'d_ids': None}, b'NULL'), ({'d_link_cost': None}, b'NULL')):
            assert lib.mpe_relink_batch(eng.ctx, None, rl.state, C.byref(args(**bad))) == -1, bad
            assert word in lib.mpe_last_error(eng.ctx), (bad, lib.mpe_last_error(eng.ctx))
        assert lib.mpe_relink_batch(eng.ctx, None, rl.state, C.byref(args(n_frames=9))) == -2          # over max_frames
        assert lib.mpe_relink_batch(eng.ctx, None, rl.state, C.byref(args(n_frames=(1 << 23) + 1))) == -2
        assert lib.mpe_relink_batch(eng.ctx, None, rl.state, C.byref(args(n_frames=0, d_poses=None))) == 0
        assert lib.mpe_relink_batch(eng.ctx, None, rl.state, None) == -1 and lib.mpe_relink_batch(eng.ctx, None, None, C.byref(args())) == -1
        assert lib.mpe_relink_read(eng.ctx, None, None, None, None) == -1
        assert rl.launches() == before
        with pytest.raises(ValueError):
            rl.update(p.double(), f, n, i)
        with pytest.raises(ValueError):
            rl.update(p, f, n, i.long())
        with pytest.raises(ValueError):
            rl.update(p[:, :2].contiguous(), f, n, i)
        with pytest.raises(ValueError):
            rl.update(p.cpu(), f, n, i)
        with pytest.raises(ValueError):
            rl.update(*(torch.cat([t, t]) for t in (p, f, n, i)))        # 16 frames, made for 8
        rc.same(feed(rl, c.arrays()), c.want)                # the sequence runs as if nothing had been
    finally:
        rl.close()
    rl.close()
    with pytest.raises(RuntimeError):
        rl.update(p, f, n, i)
    for method in (rl.counters, rl.launches, rl.reset):
        with pytest.raises(L.MpeError) as err:
            method()
        assert err.value.code == -1 and 'mpe_relink_' in str(err.value)


def test_behaviour_and_the_skeleton_table(eng):
    """The behavioural case of test_relink_host.py through the device path gives the statement's bits.  Skeleton.observe /
    update(10) on the relinked ids: body 1, which is seen for 6 frames between its two absences, has one table row with 10
    lengths or more on every bone; on the tracker's ids the fragment of those 6 frames has none.  Both are true of the
    statements (harness/skeleton.py on the two sets of ids) and of the device tables."""
    R, S = pkg('harness.relink'), pkg('harness.skeleton')
    poses, flags, n_persons, ids, who = rc.behaviour()
    arrays = (poses, flags, n_persons, ids)
    ref, _ = rc.statement(R, arrays, 'tri', rc.BEHAVE_OPTIONS)
    rl = relinker(eng, 'tri', rc.BEHAVE_OPTIONS, 4)
    try:
        got = feed(rl, arrays, (50, 70))
    finally:
        rl.close()
    rc.same(got, ref)
    assert ref['counters'].tolist() == [3, 6, 0]
    short = ids[46][who[46] == 1][0]                         # body 1 between its absences (frames 45 .. 50)
    assert (ids == short).sum() == 6
    tables = {}
    for name, use in (('tracker', ids), ('relinked', got['ids'])):
        st = S.new_state(16, S.BONES_18, 0.002)
        S.observe_sequence(st, poses, flags, n_persons, use, 'tri', (1 << rc.J) - 1)
        S.length_table(st, 10)
        sk = eng.skeleton('tri', bin_mm=2.0, tid_cap=16, pcap=4)
        try:
            sk.observe(dev(poses), dev(flags), dev(n_persons), dev(use))
            sk.update(10)
            tables[name] = sk.lengths()
        finally:
            sk.close()
        assert tables[name]['len'].tobytes() == st['len'].tobytes() and tables[name]['count'].tobytes() == st['count'].tobytes()
    assert not (tables['tracker']['len'][short] > 0).any() and (tables['tracker']['count'][short] == 6).all()
    one = got['ids'][46][who[46] == 1][0]
    assert (got['ids'][who == 1] == one).all() and (tables['relinked']['count'][one] >= 10).all() and (tables['relinked']['len'][one] > 0).all()
    assert ((tables['relinked']['len'] > 0).any(axis=1)).sum() == 3


def test_harness_relink_line(tmp_path, capsys, monkeypatch):
    """metrics_from_triangulation --relink 20 on the committed test file: match, triangulate, track, relink.  The rows that
    reach the relinker, run through harness/relink.py chunk by chunk, give its outputs bit for bit and the printed line;
    without the flag the output is what it is without this stage, line for line."""
    hd = os.path.join(GOLDEN, 'harness')
    with open(os.path.join(hd, 'harness_expected.json')) as fh:
        exp = json.load(fh)
    mdir = harness_model_files(str(tmp_path), exp['inputs'])
    m = importlib.import_module('3d_multi_pose_estimator_amd.harness.metrics_from_triangulation')
    R, P = pkg('harness.relink'), pkg('pipeline')
    argv = ['--testfiles', os.path.join(hd, exp['inputs']['testfile']), '--tmdir', hd, '--modelsdir', mdir,
            '--datastep', str(exp['inputs']['datastep'])]
    seen = []
    real_update = P.Relinker.update

    def recording_update(self, poses, flags, n_persons, ids):
        out = real_update(self, poses, flags, n_persons, ids)
        seen.append(([t.cpu().numpy() for t in (poses, flags, n_persons, ids)], {k: v.cpu().numpy() for k, v in out.items()}, dict(self.options)))
        return out
    monkeypatch.setattr(P.Relinker, 'update', recording_update)

    def lines(extra):
        capsys.readouterr()
        del seen[:]
        out = m.main(argv + extra)
        return out, [ln for ln in capsys.readouterr().out.splitlines() if not ln.startswith(('Mean time', 'Frames per second'))]
    plain, text = lines(['--track', '--batch', '7'])
    assert 'relink' not in plain and not seen and not any(ln.startswith('Relinked') for ln in text)
    for batch in ('7', '256'):
        out, with_flag = lines(['--relink', '20', '--relink-max-gap', '40', '--batch', batch])
        assert [ln for ln in with_flag if not ln.startswith(('Relinked', 'Tracks'))] == [ln for ln in text if not ln.startswith('Tracks')]
        assert with_flag[-1].startswith('Relinked (gate 20 mm, gap up to 40): ') and with_flag[-2].startswith('Tracks (gate 0.5 m, gap 2): ')
        assert len(seen) >= (2 if batch == '7' else 1)
        state, summary, ref = None, R.RelinkSummary(), None
        for frames, dev_out, options in seen:
            assert options['gate_m'] == 0.02 and options['min_gap'] == 4 and options['max_gap'] == 40 and options['tid_cap'] == 256
            ref, state = R.relink_sequence(*frames, 'tri', rc.BONES, options, state)
            rc.same(dev_out, ref, ('ids', 'link_cost', 'link_gap'), batch)
            summary.add(frames[3], ref)
        r = summary.result(ref)
        assert out['relink'] == r and r['births'] + r['links'] == r['tracks_before'] > 0 and r['tracks_after'] == r['births']
        assert with_flag[-1] == R.report_line(20.0, 40, r)
        assert out['tracks']['tracks'] == r['tracks_after'] and out['tracks']['late_births'] == plain['tracks']['late_births'] - r['links']
