"""mpe_consolidate_batch (csrc/consolidate.hip, Engine.consolidate) against its host statement harness/consolidate.py, bit
for bit, and the --merge / --found flags of the harness scripts end to end.  No engine of this file has weights loaded."""
import ctypes as C
import importlib

import numpy as np
import pytest

import consolidate_cases as cc
import geom_cases as gc
import regroup_cases as rc
from conftest import oracle, pkg

pytestmark = pytest.mark.gpu
HARNESS = '3d_multi_pose_estimator_amd.harness.'
KEYS = cc.KEYS
_made = {}


class Setup:
    """A case on the device, its rows and poses padded to the engine's row capacity."""

    def __init__(self, name, checked=True, **engine_kw):
        import torch
        first = cc.case(name)
        kw = dict(max_frames=max(17, first.pb.n_frames), max_persons_per_camera=max(4, first.most))
        kw.update(engine_kw)
        self.eng = eng = pkg('pipeline').Engine(first.params, first.calib, **kw)
        assert eng.gat_dims is None and eng.mlp_out is None
        self.case = case = cc.case(name, pcap=eng.pcap)
        self.db = eng.to_device(case.pb) if checked else case.pb.to(eng.device)      # (to_device refuses frames over the head cap)
        if name == 'explicit':
            self.db.struct.d_slot_cam = self.db.struct.d_slot_n = None
        self.rows, self.n_persons = torch.from_numpy(case.rows).cuda(), torch.from_numpy(case.n_persons).cuda()
        self.dev = {k: (torch.from_numpy(np.ascontiguousarray(p)).cuda(), torch.from_numpy(np.ascontiguousarray(f)).cuda(), m)
                    for k, (p, f, m) in case.kinds().items()}

    def device(self, kind, out=None, n_out=None, **kw):
        poses, flags, _ = self.dev[kind]
        return self.eng.consolidate(self.db, self.rows, self.n_persons, poses, flags, kind, out=out, n_out=n_out, **dict(self.case.opts, **kw))

    def statement(self, kind, **kw):
        kw.setdefault('fcap', self.case.opts.get('fcap', min(self.eng.hpf, 64)))
        return self.case.statement(kind, max_heads_per_frame=self.eng.hpf, **kw)


def setup(name):
    if name not in _made:
        _made[name] = Setup(name)
    return _made[name]


def teardown_module(module):
    for s in _made.values():
        s.eng.close()
    _made.clear()


def host_of(out):
    return {k: out[k].cpu().numpy() for k in KEYS}


def assert_same(got, want, what):
    for k in KEYS:
        g, w = got[k], want[k]
        assert g.shape == w.shape and g.dtype == w.dtype, (what, k, g.shape, w.shape, g.dtype, w.dtype)
        if not cc.same_bits(g, w):
            bad = np.argwhere(g != w)
            print(what, k, 'differing', len(bad), 'of', g.size, 'first', bad[:3].tolist(), g[tuple(bad[0])], w[tuple(bad[0])])
        assert cc.same_bits(g, w), (what, k)


@pytest.mark.parametrize('kind', ['triang', 'est'])
@pytest.mark.parametrize('name', cc.NAMES)
def test_bit_equal_to_host_statement(name, kind):
    """All nine outputs, every entry, under the three option sets; f64 poses with joint flags and f32 poses with person flags."""
    s = setup(name)
    if name in ('lost', 'lanes'):
        assert s.eng.pcap >= 24 and s.eng.pcap * s.eng.pcap > 256         # more (p, q) pairs than lanes
    for opts in cc.option_sets(s.case.params):
        got, want = host_of(s.device(kind, **opts)), s.statement(kind, **opts)
        print(name, kind, opts, 'scored', int((want['dist'] >= 0).sum()), int((want['pair'] >= 0).sum()), 'counts', want['counts'].sum(axis=0).tolist(),
              'status', want['status'].tolist())
        assert_same(got, want, (name, kind, opts))
    s.eng.sync_status()
    assert got['dist'].shape == (s.case.pb.n_frames, s.eng.pcap, s.eng.pcap)


@pytest.mark.parametrize('kind', ['triang', 'est'])
def test_in_place_and_frames_apart(kind):
    """out= / n_out= aliasing the inputs gives the bits of the out-of-place call; a batch in one call equals frame-by-frame calls."""
    for name in ('arplab', 'short'):
        s = setup(name)
        whole = host_of(s.device(kind))
        assert whole['change'].any() and (whole['n_persons'] != s.case.n_persons).any()
        poses, flags, _ = s.dev[kind]
        mine, n_mine = s.rows.clone(), s.n_persons.clone()
        alias = s.eng.consolidate(s.db, mine, n_mine, poses, flags, kind, out=mine, n_out=n_mine, **s.case.opts)
        assert alias['persons'].data_ptr() == mine.data_ptr() and alias['n_persons'].data_ptr() == n_mine.data_ptr()
        assert_same(host_of(alias), whole, 'in place')
        packing = pkg('packing')
        for f in range(s.case.pb.n_frames):
            db = s.eng.to_device(packing.pack_frames(s.case.processed[f:f + 1], s.case.params))
            one = s.eng.consolidate(db, s.rows[f:f + 1].contiguous(), s.n_persons[f:f + 1].contiguous(), poses[f:f + 1].contiguous(),
                                    flags[f:f + 1].contiguous(), kind, **s.case.opts)
            assert_same(host_of(one), {k: whole[k][f:f + 1] for k in KEYS}, ('frame', f))
        s.eng.sync_status()


def test_arguments():
    """What the entry point refuses, with a message; zero frames gives empty tensors."""
    L = pkg('lib')
    s = setup('split')
    for kw, word in (({'merge_m': 0.0}, 'merge_m'), ({'merge_m': float('nan')}, 'merge_m'), ({'found_m': 0.0}, 'found_m'),
                     ({'found_m': float('nan')}, 'found_m'), ({'clip_m': -1.0}, 'clip_m'), ({'clip_m': float('nan')}, 'clip_m'),
                     ({'min_joints': 0}, 'min_joints'), ({'min_joints': cc.J + 1}, 'min_joints'), ({'found_min_views': 1}, 'found_min_views'),
                     ({'fcap': 0}, 'fcap'), ({'fcap': 65}, 'fcap'), ({'merge': False, 'found': False}, 'flags')):
        with pytest.raises(L.MpeError) as err:
            s.device('triang', **kw)
        assert err.value.code == -1 and word in str(err.value), str(err.value)
    poses, flags, mask = s.dev['triang']

    def raw(**over):
        a = L.mpe_consolidate_args()
        a.n_frames, a.pcap, a.n_joints, a.pose_f64, a.joint_flags, a.joint_mask, a.threshold = s.db.n_frames, s.eng.pcap, s.eng.J, 1, 1, mask, 0.5
        a.min_joints, a.merge_m, a.found_m, a.clip_m, a.found_min_views, a.fcap, a.flags = 3, 0.1, 0.05, 0.0, 2, 20, 3
        a.d_persons, a.d_n_persons, a.d_poses, a.d_flags = s.rows.data_ptr(), s.n_persons.data_ptr(), poses.data_ptr(), flags.data_ptr()
        out = s.device('triang', fcap=20)
        a.d_persons_out, a.d_n_persons_out, a.d_change, a.d_n_views = (out[k].data_ptr() for k in ('persons', 'n_persons', 'change', 'n_views'))
        a.d_dist, a.d_pair, a.d_free, a.d_counts, a.d_status = (out[k].data_ptr() for k in ('dist', 'pair', 'free', 'counts', 'status'))
        for k, v in over.items():
            setattr(a, k, v)
        s.eng._chk(s.eng.lib.mpe_consolidate_batch(s.eng.ctx, s.eng._stream(), C.byref(s.db.struct), C.byref(a)))

    raw()
    for over, code, word in (({'n_frames': 2}, -1, 'frames'), ({'n_joints': 17}, -1, 'joints'), ({'flags': 4}, -1, 'flags'), ({'flags': 0}, -1, 'flags'),
                             ({'d_dist': None}, -1, 'NULL output'), ({'d_pair': None}, -1, 'NULL output'), ({'d_free': None}, -1, 'NULL output'),
                             ({'d_n_persons_out': None}, -1, 'NULL output'), ({'d_poses': None}, -1, 'NULL argument'),
                             ({'pcap': 129}, -2, 'pcap'), ({'pcap': 0}, -1, 'pcap 0 must be at least 1'), ({'fcap': 65}, -1, 'fcap 65'),
                             ({'pose_f64': 2}, -1, 'pose_f64 2 and joint_flags 1 must be 0 or 1'), ({'joint_flags': -1}, -1, 'joint_flags -1')):
        with pytest.raises(L.MpeError) as err:
            raw(**over)
        assert err.value.code == code and word in str(err.value), str(err.value)
    assert s.eng.lib.mpe_consolidate_batch(None, None, C.byref(s.db.struct), None) == -1
    with pytest.raises(ValueError):
        s.eng.consolidate(s.db, s.rows, s.n_persons, poses, flags, 'gt')
    with pytest.raises(ValueError):
        s.eng.consolidate(s.db, s.rows, s.n_persons, poses, flags, 'est')
    with pytest.raises(ValueError):
        s.eng.consolidate(s.db, s.rows, s.n_persons, poses, flags, 'triang', n_out=s.n_persons[:1])
    import torch
    empty = s.eng.to_device(pkg('packing').pack_frames([], s.case.params))
    z = s.eng.consolidate(empty, s.rows[:0].contiguous(), s.n_persons[:0].contiguous(), poses[:0].contiguous(), flags[:0].contiguous(), 'triang')
    assert tuple(z['persons'].shape) == (0, s.eng.pcap, s.eng.V) and all(z[k].numel() == 0 for k in KEYS) and z['pair'].dtype == torch.float64
    s.eng.sync_status()


@pytest.mark.parametrize('kind', ['triang', 'est'])
def test_frames_without_any_head(kind):
    """A batch of three frames and no head at all: nothing to merge from, nothing free; the outputs through the C entry point
    with every input the batch lacks absent."""
    import torch
    syn = pkg('synthetic')
    s = setup('degenerate')
    c, eng = s.case, s.eng
    names = list(c.params.camera_names)
    frames = [syn.make_frame(c.calib, f, syn.FrameSpec(persons=3, empty_cameras=names), seed=7)[0] for f in range(3)]
    pb = pkg('packing').pack_frames([oracle().processed_input(f) for f in frames], c.params)
    assert pb.n_frames == 3 and pb.n_heads == 0
    db = eng.to_device(pb)
    rows = np.full((3, eng.pcap, eng.V), -1, np.int32)
    n = np.array([3, 0, 2], np.int32)
    poses, flags, mask = (np.ascontiguousarray(a[:3]) if isinstance(a, np.ndarray) else a for a in c.kinds()[kind])
    flags = np.ones_like(flags)
    poses = poses.copy()
    poses[0, 0], poses[0, 2] = 1.0, -1.0
    poses[0, 1] = poses[0, 0] + np.asarray(cc.SHIFT, poses.dtype)         # two rows without heads, 27 mm apart: merged (nothing moves)
    want = pkg('harness.consolidate').consolidate(c.calib, pb, rows, n, poses, flags, mask, max_heads_per_frame=eng.hpf, fcap=min(eng.hpf, 64))
    assert want['counts'].tolist() == [[1, 0, 0, 0], [0, 0, 0, 0], [0, 0, 0, 0]] and (want['free'] == -1).all() and (want['pair'] == -1).all()
    dev = [torch.from_numpy(a).cuda() for a in (rows, n, poses, flags)]
    got = host_of(eng.consolidate(db, *dev, kind))
    assert_same(got, want, ('no heads', kind))
    assert not got['n_views'].any() and not got['change'].any() and not got['status'].any() and (got['persons'] == -1).all()
    named = rows.copy()
    named[2, 0, 1] = 0                                                    # a row that names a head of a frame without heads: a bad row
    got = host_of(eng.consolidate(db, torch.from_numpy(named).cuda(), *dev[1:], kind))
    want = pkg('harness.consolidate').consolidate(c.calib, pb, named, n, poses, flags, mask, max_heads_per_frame=eng.hpf, fcap=min(eng.hpf, 64))
    assert want['status'].tolist() == [0, 0, 1] and want['n_views'][2, 0] == 1
    assert_same(got, want, ('no heads, a bad row', kind))
    eng.sync_status()


def test_frames_over_the_head_cap_are_copied_through():
    """A context whose max_heads_per_frame the frames exceed: rows and counts copied through, the tables -1, the status bit in
    d_status and in mpe_sync_status."""
    L = pkg('lib')
    s = Setup('split', checked=False, max_heads_per_frame=19)
    try:
        assert s.eng.hpf == 19 and s.case.pb.max_heads_per_frame() == 20
        got, want = host_of(s.device('triang')), s.statement('triang')
        assert_same(got, want, 'over cap')
        assert (got['status'] == L.MPE_CONSOLIDATE_OVER_CAP).all() and np.array_equal(got['persons'], s.case.rows)
        assert (got['dist'] == -1).all() and (got['pair'] == -1).all() and not got['counts'].any() and np.array_equal(got['n_persons'], s.case.n_persons)
        with pytest.raises(L.MpeError) as err:
            s.eng.sync_status()
        assert err.value.code == -2
    finally:
        s.eng.close()


def partition_after(c, eng, db, persons, n_persons):
    """regroup, consolidate and the 3D stage again on device rows -> (consolidate's outputs, the poses they were fed, flags)."""
    poses, jv = eng.triangulate(db, persons, n_persons, all_joints=True)
    rg = eng.regroup(db, persons, n_persons, poses, jv, 'triang')
    poses, jv = eng.triangulate(db, rg['persons'], n_persons, all_joints=True)
    out = eng.consolidate(db, rg['persons'], n_persons, poses, jv, 'triang')
    again, _ = eng.triangulate(db, out['persons'], out['n_persons'], all_joints=True)
    assert tuple(again.shape) == tuple(poses.shape)
    return out, rg['persons'], poses, jv


def test_end_to_end_after_geometric_matching():
    """geom_match on the `messy` input of geom_cases, triangulate, regroup, triangulate, consolidate on the GPU's own poses: bit
    for bit the statement fed the same poses; neither the frames with the true partition nor the right entries fall.  Then the
    same with one person's row deleted per frame: the partition comes back wherever the host statement restores it."""
    import torch
    CS = pkg('harness.consolidate')
    c = gc.case('messy')
    eng = pkg('pipeline').Engine(c.params, c.calib, max_frames=17, max_persons_per_camera=max(4, c.most))
    try:
        db = eng.to_device(c.pb)
        _, persons, n_persons = eng.geom_match(db, want_scores=False)
        out, rows_d, poses, jv = partition_after(c, eng, db, persons, n_persons)
        eng.sync_status()
        rows, n = rows_d.cpu().numpy(), n_persons.cpu().numpy()
        want = CS.consolidate(c.calib, c.pb, rows, n, poses.cpu().numpy(), jv.cpu().numpy(), (1 << cc.J) - 1, max_heads_per_frame=eng.hpf,
                              fcap=min(eng.hpf, 64))
        got = host_of(out)
        assert_same(got, want, 'messy')
        before, after = rc.quality(c, rows, n), rc.quality(c, got['persons'], got['n_persons'])
        print('frames with the true partition:', before[0], '->', after[0], 'of', c.pb.n_frames, '; right entries:', before[1], '->', after[1],
              '; counts', got['counts'].sum(axis=0).tolist())
        assert after[0] >= before[0] and after[1] >= before[1]
        # one person's row deleted per frame (the last row is moved into its place, the count falls by one)
        matched = persons.cpu().numpy()
        cut, n_cut = cc.delete_rows(matched, n)
        d_cut, d_n = torch.from_numpy(cut).cuda(), torch.from_numpy(n_cut).cuda()
        out2, rows2_d, poses2, jv2 = partition_after(c, eng, db, d_cut, d_n)
        eng.sync_status()
        rows2 = rows2_d.cpu().numpy()
        want2 = CS.consolidate(c.calib, c.pb, rows2, n_cut, poses2.cpu().numpy(), jv2.cpu().numpy(), (1 << cc.J) - 1, max_heads_per_frame=eng.hpf,
                               fcap=min(eng.hpf, 64))
        got2 = host_of(out2)
        assert_same(got2, want2, 'messy, a row deleted')
        restored_on_cpu = cc.messy_restored()
        back = [rc.partition_of(got2['persons'][f], got2['n_persons'][f]) == rc.partition_of(matched[f], n[f]) for f in range(c.pb.n_frames)]
        print('partition back after the deletion:', back, 'on the CPU:', restored_on_cpu)
        assert all(b for b, r in zip(back, restored_on_cpu) if r)
    finally:
        eng.close()


def report_lines(text):
    return [ln for ln in text.splitlines() if not ln.startswith(('Mean time', 'Frames per second', 'Consolidated'))]


def test_cli_consolidated_line(tmp_path, capsys):
    """--matcher geometric --synthetic 32 --merge 0.1 --found 0.05: one further line; on that noise-free input nothing is merged
    or founded and the other lines are those of the run without the flags.  The flags go with --regroup, and the model script and
    calibrate take them as well."""
    tri = importlib.import_module(HARNESS + 'metrics_from_triangulation')
    mlp = importlib.import_module(HARNESS + 'metrics_from_model')
    base = ['--synthetic', '32', '--matcher', 'geometric', '--modelsdir', str(tmp_path), '--batch', '16']
    capsys.readouterr()
    plain = tri.main(base)
    text0 = capsys.readouterr().out
    got = tri.main(base + ['--merge', '0.1', '--found', '0.05'])
    text1 = capsys.readouterr().out
    line = [ln for ln in text1.splitlines() if ln.startswith('Consolidated')]
    assert len(line) == 1 and 'Consolidated' not in text0 and 'consolidate' not in plain and 'regroup' not in got
    assert line[0].startswith('Consolidated (merge 0.1 m, found 0.05 m): 0 rows merged, 0 founded from 0 skeletons, ')
    r = got['consolidate']
    assert set(r) == {'merged', 'founded', 'placed', 'free', 'copied'} and r['copied'] == 0
    assert r['merged'] == 0 and r['founded'] == 0 and r['placed'] == 0, r
    assert report_lines(text1) == report_lines(text0) and got['ap'] == plain['ap'] and got['mpjpe_mm'] == plain['mpjpe_mm']
    assert got['n_data'] == plain['n_data'] == 32
    both = tri.main(base + ['--regroup', '15', '--merge', '0.1', '--found', '0.05', '--found-min-views', '3', '--device-metrics'])
    text2 = capsys.readouterr().out
    assert 'regroup' in both and 'consolidate' in both and text2.count('Regrouped') == 1 and text2.count('Consolidated') == 1
    only = tri.main(base + ['--found', '0.05'])
    assert 'Consolidated (merge 0 m, found 0.05 m)' in capsys.readouterr().out and only['consolidate']['merged'] == 0
    out = mlp.main(['--synthetic', '16', '--random-weights', '--matcher', 'geometric', '--batch', '16', '--merge', '0.1', '--found', '0.05'])
    assert 'consolidate' in out and len([ln for ln in capsys.readouterr().out.splitlines() if ln.startswith('Consolidated')]) == 1
    cal = importlib.import_module(HARNESS + 'calibrate')
    cal.main(['--synthetic', '16', '--matcher', 'geometric', '--batch', '16', '--rounds', '1', '--passes', '1', '--merge', '0.1', '--found', '0.05'])
    assert len([ln for ln in capsys.readouterr().out.splitlines() if ln.startswith('Consolidated')]) == 2
