"""mpe_refine_timed_batch (csrc/refine_timed.hip, Engine.refine_timed) against its host statement harness/refine_timed.py,
bit for bit: both kinds of poses, both Huber settings, 5 and 23 cameras (eight and four (frame, person) pairs per workgroup),
row counts that leave the last workgroup part empty, every lag zero against Engine.refine, chunked calls, the refusals, the
launch count, and harness.lag --correct end to end."""
import ctypes as C

import numpy as np
import pytest

import refine_timed_cases as tc
from conftest import env, pkg

pytestmark = pytest.mark.gpu
_engines, _made = {}, {}
LAGS_MESSY = (0, 1.5, -0.25, 0.37, 2)                        # 0.37: an alpha whose products round


def engine(variant):
    if variant not in _engines:
        e = env(variant)
        _engines[variant] = pkg('pipeline').Engine(e.params, e.calib, max_frames=64, max_persons_per_camera=11)
    return _engines[variant]


class Setup:
    """A scene on the device: the batch, the persons and the table of either kind as tensors."""

    def __init__(self, scene):
        import torch
        self.scene = s = scene
        self.eng = eng = engine(s.variant)
        self.db = eng.to_device(s.pb)
        dev = lambda a: torch.from_numpy(np.ascontiguousarray(a)).cuda()      # noqa: E731
        self.persons, self.n_persons, self.ids = dev(s.persons), dev(s.n_persons), dev(s.ids)
        self.dev = {k: (dev(p), dev(f), m) for k, (p, f, m) in s.kinds.items()}

    def device(self, kind, lags, frames=None, **kw):
        """The scene, or its frames [a, b) as a batch of their own, against the whole table -> host arrays."""
        poses, flags, mask = self.dev[kind]
        a, b = (0, self.scene.pb.n_frames) if frames is None else frames
        db = self.db if frames is None else self.eng.to_device(self.scene.sub_batch(a, b))
        out = self.eng.refine_timed(db, a, self.persons[a:b].contiguous(), poses, flags, self.n_persons, self.ids, kind, lags, joint_mask=mask, **kw)
        return {k: out[k].cpu().numpy() for k in tc.KEYS}


def setup(key, maker):
    if key not in _made:
        _made[key] = Setup(maker())
    return _made[key]


def messy():
    return setup('messy', lambda: tc.messy('panoptic', 12, LAGS_MESSY))


def teardown_module(module):
    for eng in _engines.values():
        eng.close()
    _made.clear()
    _engines.clear()


def assert_same(got, want, what, keys=tc.KEYS):
    for k in keys:
        g, w = got[k], want[k]
        assert g.shape == w.shape and g.dtype == w.dtype, (what, k, g.shape, w.shape, g.dtype, w.dtype)
        if not tc.same_bits(g, w):
            bad = np.argwhere(g != w)
            print(what, k, 'differing', len(bad), 'first', bad[:3].tolist(), g[tuple(bad[0])], w[tuple(bad[0])])
        assert tc.same_bits(g, w), (what, k)


@pytest.mark.parametrize('huber', [0.0, 5.0])
@pytest.mark.parametrize('kind', ['triang', 'est'])
def test_bit_equal_to_host_statement(kind, huber):
    """lc.messy on PANOPTIC, three bodies in five rows (60 (frame, person) pairs: the last workgroup of eight is half
    empty), rows permuted, an id of -1, a duplicate id, n_persons out of range, a NaN neighbour, dropped flags: poses,
    status, cost0, cost1, iters, n_views and n_timed, every entry."""
    s = messy()
    got, want = s.device(kind, LAGS_MESSY, huber_px=huber), tc.statement(s.scene, kind, LAGS_MESSY, huber_px=huber)
    st = want['status']
    print(kind, huber, 'joints', st.size, 'solved', int((st & 1).astype(bool).sum()), 'moved', int((st & 2).astype(bool).sum()),
          'timed cameras', np.bincount(want['n_timed'].reshape(-1)).tolist())
    assert_same(got, want, (kind, huber))
    assert want['n_timed'].max() == 4 and (want['n_timed'][(st & 1) != 0] == 0).any() and (st & 2).any()
    assert got['poses'].dtype == (np.float64 if kind == 'triang' else np.float32)


@pytest.mark.parametrize('bodies', [10, 11])
def test_many_rows_on_23_cameras(bodies):
    """The 23-camera rig of the lag tests with ten and eleven rows and lags drawn from the multiples of 1/8 within +-2: 23
    cameras x 18 joints x 3 doubles are 9.9 KB of offsets per (frame, person), so the workgroup holds four of them, not
    eight, and 110 and 121 pairs leave its last one part empty."""
    lags = [int(k) / 8.0 for k in np.random.default_rng(5600).integers(-16, 17, 23)]
    s = setup(('rows', bodies), lambda: tc.Scene('ring23', 11, lags, n_bodies=bodies, seed=5400 + bodies, pcap=bodies, permute=True, weave=0.03))
    assert s.eng.V == 23 and (11 * bodies) % 4 != 0 and len(set(lags)) > 10 and 0.0 in lags
    got, want = s.device('triang', lags, huber_px=5.0), tc.statement(s.scene, 'triang', lags, huber_px=5.0)
    print('rows', bodies, 'timed cameras up to', int(want['n_timed'].max()), 'solved', int((want['status'] & 1).astype(bool).sum()))
    assert_same(got, want, ('rows', bodies))
    assert want['n_timed'].max() >= 15 and (want['status'] & 2).any()


def test_row_count_no_multiple_of_the_workgroup():
    """7 frames x 3 rows = 21 pairs for workgroups of eight, exact detections, the issue's lags."""
    s = setup('7x3', lambda: tc.Scene('panoptic', 7, tc.LAGS))
    assert s.scene.pcap == 3
    for kind in ('triang', 'est'):
        got, want = s.device(kind, tc.LAGS), tc.statement(s.scene, kind, tc.LAGS)
        assert_same(got, want, ('7x3', kind))
        assert want['n_timed'].max() == 4


@pytest.mark.parametrize('kind', ['triang', 'est'])
def test_all_lags_zero_is_engine_refine(kind):
    """Every lag zero: the seven shared outputs are Engine.refine's on the same frames, bit for bit, and nothing is timed
    (-0.0 is a zero, too)."""
    eng = engine('panoptic')
    s = setup('messy at the engine\'s pcap', lambda: tc.messy('panoptic', 12, LAGS_MESSY, pcap=eng.pcap))
    poses, flags, mask = s.dev[kind]
    for huber in (0.0, 5.0):
        got = s.device(kind, [0.0, -0.0, 0.0, 0.0, 0.0], huber_px=huber)
        plain = eng.refine(s.db, s.persons, s.n_persons, poses, flags, kind, joint_mask=mask, huber_px=huber)
        assert_same(got, {k: plain[k].cpu().numpy() for k in tc.SHARED}, (kind, huber), tc.SHARED)
        assert not got['n_timed'].any() and (got['status'] & 2).any()


def test_chunked_calls_equal_one_call():
    """12 frames as 5 + 7, each packed on its own against the whole table, and a call of zero frames."""
    s = messy()
    whole = s.device('triang', LAGS_MESSY, huber_px=2.0)
    for a, b in ((0, 5), (5, 12)):
        part = s.device('triang', LAGS_MESSY, frames=(a, b), huber_px=2.0)
        assert_same(part, {k: whole[k][a:b] for k in tc.KEYS}, ('chunk', a, b))
    poses, flags, mask = s.dev['triang']
    empty = s.eng.refine_timed(s.eng.to_device(s.eng.pack([])), 7, s.persons[:0].contiguous(), poses, flags, s.n_persons, s.ids, 'triang', LAGS_MESSY)
    assert tuple(empty['poses'].shape) == (0, s.scene.pcap, tc.J, 3) and all(empty[k].numel() == 0 for k in tc.KEYS)


def raw_args(s, kind='triang', lags=LAGS_MESSY, out=None):
    """The argument struct of a whole-scene call with tensors of its own (kept alive by the caller) -> (struct, tensors)."""
    import torch
    L = pkg('lib')
    poses, flags, mask = s.dev[kind]
    F, pcap = s.scene.pb.n_frames, s.scene.pcap
    shape = (F, pcap, tc.J)
    t = {'poses': torch.empty_like(poses) if out is None else out, 'cost0': torch.empty(shape, dtype=torch.float64, device='cuda'),
         'cost1': torch.empty(shape, dtype=torch.float64, device='cuda')}
    t.update({k: torch.empty(shape, dtype=torch.uint8, device='cuda') for k in ('status', 'iters', 'n_views', 'n_timed')})
    a = L.mpe_refine_timed_args()
    a.n_frames, a.pcap, a.n_joints, a.pose_f64, a.joint_flags = F, pcap, tc.J, int(kind == 'triang'), int(kind == 'triang')
    a.frame_start, a.n_table, a.joint_mask, a.threshold, a.max_iters, a.step_tol, a.huber_px = 0, F, mask, 0.5, 10, 1e-6, 0.0
    for c, x in enumerate(lags):
        a.lag[c] = x
    a.d_persons, a.d_poses, a.d_flags, a.d_n_persons, a.d_tid = (x.data_ptr() for x in (s.persons, poses, flags, s.n_persons, s.ids))
    a.d_poses_out, a.d_status, a.d_cost0, a.d_cost1 = (t[k].data_ptr() for k in ('poses', 'status', 'cost0', 'cost1'))
    a.d_iters, a.d_n_views, a.d_n_timed = (t[k].data_ptr() for k in ('iters', 'n_views', 'n_timed'))
    return a, t


def test_arguments():
    """An `out` that shares storage with the table raises, and the entry point refuses a d_poses_out inside the table's
    bytes; a lag of 9, a NaN lag; what mpe_refine_batch and mpe_lag_batch refuse on the shared arguments."""
    L = pkg('lib')
    s = messy()
    eng = s.eng
    poses, flags, mask = s.dev['triang']
    call = lambda **kw: eng.refine_timed(s.db, 0, s.persons, poses, flags, s.n_persons, s.ids, 'triang', **{'lags': LAGS_MESSY, **kw})   # noqa: E731
    with pytest.raises(ValueError, match='share storage'):
        call(out=poses)
    both = poses.new_empty((2,) + tuple(poses.shape))
    both[0].copy_(poses)
    with pytest.raises(ValueError, match='share storage'):
        eng.refine_timed(s.db, 0, s.persons, both[0], flags, s.n_persons, s.ids, 'triang', LAGS_MESSY, out=both[1])
    for kw, word in (({'lags': (0, 9, 0, 0, 0)}, 'lag'), ({'lags': (0, 0, float('nan'), 0, 0)}, 'lag'), ({'lags': (0, 0, 0, 0, -8.125)}, 'lag'),
                     ({'max_iters': 0}, 'max_iters'), ({'max_iters': 65}, 'max_iters'), ({'step_tol': -1e-9}, 'step_tol'), ({'huber_px': -1.0}, 'huber_px')):
        with pytest.raises(L.MpeError) as err:
            call(**kw)
        assert err.value.code == -1 and word in str(err.value), str(err.value)
    call(lags=(0, 8, -8, 0, 0))                              # the window's edge is allowed
    with pytest.raises(ValueError):
        call(lags=(0, 1, 2))
    with pytest.raises(ValueError):
        eng.refine_timed(s.db, 0, s.persons, *s.dev['est'][:2], s.n_persons, s.ids, 'triang', LAGS_MESSY)
    F = s.scene.pb.n_frames
    for change, word in ((dict(d_poses_out=poses.data_ptr() + 8), 'overlaps'), (dict(d_poses_out=poses.data_ptr() + poses.numel() * 8 - 8), 'overlaps'),
                         (dict(frame_start=-1), 'frame_start'), (dict(frame_start=1), 'table'), (dict(n_table=F - 1), 'table'),
                         (dict(n_frames=F - 1), 'frames'), (dict(n_joints=17), 'joints'), (dict(d_n_timed=None), 'NULL'), (dict(d_tid=None), 'NULL')):
        a, keep = raw_args(s)
        for k, v in change.items():
            setattr(a, k, v)
        with pytest.raises(L.MpeError) as err:
            eng._chk(eng.lib.mpe_refine_timed_batch(eng.ctx, eng._stream(), C.byref(s.db.struct), C.byref(a)))
        assert err.value.code == -1 and word in str(err.value), str(err.value)
    eng.sync_status()


def loaded_hip_runtime():
    """The HIP runtime this process already runs on (the one torch brought), as a ctypes handle."""
    with open('/proc/self/maps') as fh:
        paths = sorted({ln.split()[-1] for ln in fh if 'libamdhip64' in ln})
    assert len(paths) == 1, paths
    return C.CDLL(paths[0])


def test_one_launch():
    """The call neither synchronises nor allocates, so a stream under capture takes it; the captured graph has exactly one
    node, a kernel.  Nothing is replayed."""
    import torch
    s = messy()
    eng, hip = s.eng, loaded_hip_runtime()
    hip.hipStreamBeginCapture.argtypes = [C.c_void_p, C.c_int]
    hip.hipStreamEndCapture.argtypes = [C.c_void_p, C.POINTER(C.c_void_p)]
    hip.hipGraphGetNodes.argtypes = [C.c_void_p, C.POINTER(C.c_void_p), C.POINTER(C.c_size_t)]
    hip.hipGraphNodeGetType.argtypes = [C.c_void_p, C.POINTER(C.c_int)]
    hip.hipGraphDestroy.argtypes = [C.c_void_p]
    a, keep = raw_args(s)
    side = torch.cuda.Stream()
    torch.cuda.synchronize()
    graph, rc = C.c_void_p(), None
    assert hip.hipStreamBeginCapture(side.cuda_stream, 2) == 0                # relaxed: other streams of the process stay legal
    try:
        rc = eng.lib.mpe_refine_timed_batch(eng.ctx, C.c_void_p(side.cuda_stream), C.byref(s.db.struct), C.byref(a))
    finally:
        ended = hip.hipStreamEndCapture(side.cuda_stream, C.byref(graph))
    assert rc == 0 and ended == 0 and graph
    n = C.c_size_t()
    assert hip.hipGraphGetNodes(graph, None, C.byref(n)) == 0
    nodes = (C.c_void_p * max(n.value, 1))()
    assert hip.hipGraphGetNodes(graph, nodes, C.byref(n)) == 0
    kinds = []
    for i in range(n.value):
        t = C.c_int(-1)
        assert hip.hipGraphNodeGetType(nodes[i], C.byref(t)) == 0
        kinds.append(t.value)
    hip.hipGraphDestroy(graph)
    assert kinds == [0], kinds                               # hipGraphNodeTypeKernel


def test_script_corrects_subframe_lags(capsys, tmp_path):
    """harness.lag --synthetic 32 --lags 0,0.5,-0.25,1.25,-1.5 --correct 3 through the device: every estimate ends nearer
    the truth than before the correction and the cost at the best entry falls each round (directions only; DESIGN.md 7.16
    records the values).  The file it writes is what --lags of the metrics scripts takes: one further line, joints timed,
    and a cost that does not rise."""
    import json
    true = [0, 0.5, -0.25, 1.25, -1.5]
    path = str(tmp_path / 'lags.json')
    rep = pkg('harness.lag').main(['--synthetic', '32', '--lags', ','.join(str(x) for x in true), '--persons', '2', '--lag-seed', '5200',
                                   '--matcher', 'geometric', '--window', '3', '--sub', '4', '--rounds', '3', '--correct', '3', '--out', path])
    text = capsys.readouterr().out
    with capsys.disabled():
        print(text)
    with open(path) as fh:
        written = json.load(fh)['lags']
    assert list(written) == list(env('panoptic').params.used_cameras_skeleton_matching) and written[list(written)[0]] == 0.0
    syn = ['--synthetic', '16', '--random-weights', '--teacher-scores', '--batch', '16', '--noise-px', '2']
    for name in ('metrics_from_triangulation', 'metrics_from_model'):
        # the generator's frames are independent draws: a gate of 100 m links their persons into tracks all the same
        out = pkg('harness.' + name).main(syn + ['--track', '--track-gate', '100', '--refine', '8', '--lags', path])
        line = [ln for ln in capsys.readouterr().out.splitlines() if ln.startswith('Refined in time')]
        r = out['refine_timed']
        with capsys.disabled():
            print(name, line)
        assert len(line) == 1 and 'refine' not in out and r['cameras_lagged'] == 4 and r['joints_timed'] > 0 and r['mean_cost1'] <= r['mean_cost0']
    rounds = rep['correct']
    assert len(rounds) == 3 and all(r['joints_timed'] > 0 for r in rounds)
    shift = rep['total_shift']
    before = [shift[c] + rounds[0]['lag_before'][c] for c in range(5)]
    after = [shift[c] + rounds[-1]['lag_after'][c] for c in range(5)]
    with capsys.disabled():
        print('before', before, 'after', after)
    for c in range(1, 5):
        assert abs(after[c] - true[c]) < abs(before[c] - true[c]), (c, before[c], after[c])
    cost = [sum(rounds[0]['rms_before'][c] ** 2 for c in range(5))] + [sum(r['rms_after'][c] ** 2 for c in range(5)) for r in rounds]
    with capsys.disabled():
        print('cost at the best entries', cost)
    assert all(b < a for a, b in zip(cost, cost[1:]))
