"""mpe_refine_batch (csrc/refine.hip, Engine.refine) against its host statement harness/refine.py, bit for bit, and the
--refine flag of the three harness scripts end to end."""
import importlib
import sys

import numpy as np
import pytest

import refine_cases as rc
from conftest import env, pkg

pytestmark = pytest.mark.gpu
HARNESS = '3d_multi_pose_estimator_amd.harness.'
KEYS = ('poses', 'status', 'cost0', 'cost1', 'iters', 'n_views')
SYN = ['--synthetic', '16', '--random-weights', '--teacher-scores', '--batch', '16']
_made = {}


class Setup:
    """A case on the device: the engine, the batch, persons, and both kinds of starting poses (the triangulation is the
    device's own) as tensors and as the host arrays the statement takes."""

    def __init__(self, name):
        import torch
        e = env(rc.variant_of(name))
        case = rc.Case(name)
        most = max([1] + [f[c][0].count('{') for f in case.frames for c in f])
        self.eng = eng = pkg('pipeline').Engine(e.params, e.calib, max_frames=max(16, len(case.frames)), max_persons_per_camera=max(4, most),
                                                **rc.ENGINE.get(name, {}))
        self.case = case = rc.Case(name, pcap=eng.pcap)
        self.db = eng.to_device(eng.pack(case.processed))
        self.persons, self.n_persons = torch.from_numpy(case.persons).cuda(), torch.from_numpy(case.n_persons).cuda()
        tri, jv = eng.triangulate(self.db, self.persons, self.n_persons, all_joints=True, positive_ids_only=True)
        if name == 'hand made':
            tri[0, 2, 8] = torch.from_numpy(rc.behind_camera(e.calib, 2).astype(np.float64)).cuda()
        eng.sync_status()
        self.host = rc.kinds(case, (tri.cpu().numpy(), jv.cpu().numpy()))
        self.dev = {k: (torch.from_numpy(np.ascontiguousarray(p)).cuda(), torch.from_numpy(np.ascontiguousarray(f)).cuda(), m)
                    for k, (p, f, m) in self.host.items()}

    def device(self, kind, joint_mask=None, out=None, **kw):
        poses, flags, mask = self.dev[kind]
        return self.eng.refine(self.db, self.persons, self.n_persons, poses, flags, kind, joint_mask=joint_mask, out=out, **kw)

    def statement(self, kind, joint_mask=None, **kw):
        poses, flags, mask = self.host[kind]
        return pkg('harness.refine').refine(self.case.calib, self.db.host, self.case.persons, self.case.n_persons, poses, flags,
                                            mask if joint_mask is None else joint_mask, **kw)


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
        if not rc.same_bits(g, w):
            bad = np.argwhere(g != w)
            print(what, k, 'differing', len(bad), 'first', bad[:3].tolist(), g[tuple(bad[0])], w[tuple(bad[0])])
        assert rc.same_bits(g, w), (what, k)


@pytest.mark.parametrize('kind', ['triang', 'est'])
@pytest.mark.parametrize('name', rc.NAMES)
def test_bit_equal_to_host_statement(name, kind):
    """8: poses, status, cost0, cost1, iters and n_views, every entry, for huber_px in {0, 5} and step_tol in {0, 1e-6}."""
    s = setup(name)
    for huber in (0.0, 5.0):
        for tol in (0.0, 1e-6):
            got = host_of(s.device(kind, huber_px=huber, step_tol=tol))
            want = s.statement(kind, huber_px=huber, step_tol=tol)
            st = want['status']
            print(name, kind, 'huber', huber, 'step_tol', tol, 'joints', st.size, 'solved', int((st & 1).astype(bool).sum()),
                  'moved', int((st & 2).astype(bool).sum()), 'few views', int((st & 8).astype(bool).sum()), 'bad start', int((st & 16).astype(bool).sum()))
            assert_same(got, want, (name, kind, huber, tol))
            assert got['poses'].dtype == (np.float64 if kind == 'triang' else np.float32)
    if name in ('messy', '5x10', 'one frame'):
        assert (st & 2).any()
    if name == 'hand made':
        assert (st & 16).sum() == 16 and ((st & 8).any() or kind == 'triang') and (want['n_views'] == 2).any()
    if name in rc.RIGS:
        info = rc.check(s.case)
        print(name, info)
        nv = want['n_views'][..., 5]                                    # joint 5 is in both masks
        assert s.eng.V == info['V'] and s.eng.pcap == s.case.pcap == info.get('pcap', s.eng.pcap)
        rows = [0, 1, 2] if kind == 'est' else [0, 2]                   # a person in one camera has no triangulated joint
        assert nv[-1, rows].tolist() == [info['n_views'][-1][p] for p in rows] and (st & 2).any()
        if name == 'ring23' and kind == 'est':
            assert (st[2, 1] & 8).any() and not (st[:, [0, 2]] & 8).any()   # FEW_VIEWS on the device: the person camera 22 alone sees


@pytest.mark.parametrize('kind', ['triang', 'est'])
def test_in_place_frames_apart_and_one_joint(kind):
    """9: out= aliasing the input, the batch frame by frame, and a one-joint mask that leaves every other joint alone."""
    import torch
    s = setup('messy')
    whole = host_of(s.device(kind))
    poses, flags, _ = s.dev[kind]
    mine = poses.clone()
    alias = s.eng.refine(s.db, s.persons, s.n_persons, mine, flags, kind, out=mine)
    assert alias['poses'].data_ptr() == mine.data_ptr()
    assert_same(host_of(alias), whole, 'in place')
    for f in range(len(s.case.processed)):
        db = s.eng.to_device(s.eng.pack(s.case.processed[f:f + 1]))
        one = s.eng.refine(db, s.persons[f:f + 1].contiguous(), s.n_persons[f:f + 1].contiguous(), poses[f:f + 1].contiguous(),
                           flags[f:f + 1].contiguous(), kind)
        assert_same(host_of(one), {k: whole[k][f:f + 1] for k in KEYS}, ('frame', f))
    j3 = host_of(s.device(kind, joint_mask=1 << 3))
    assert_same(j3, s.statement(kind, joint_mask=1 << 3), 'joint 3')
    others = [j for j in range(rc.J) if j != 3]
    assert rc.same_bits(j3['poses'][:, :, others], s.host[kind][0][:, :, others]) and not j3['status'][:, :, others].any()
    assert np.all(j3['cost0'][:, :, others] == -1.0) and not j3['n_views'][:, :, others].any()
    if kind == 'triang':
        assert (j3['status'][:, :, 3] & 2).any()


def test_stream_order_refine_reproject_stats():
    """10: refine -> reproject -> residual_stats queued back to back give the statistics of the host chain."""
    R = pkg('harness.reprojection')
    s = setup('messy')
    poses, flags, mask = s.dev['triang']
    out = s.eng.refine(s.db, s.persons, s.n_persons, poses, flags, 'triang')
    res = s.eng.reproject(s.db, s.persons, s.n_persons, out['poses'], flags, 'triang')
    got = s.eng.residual_stats(res)
    want = s.statement('triang')
    hres = R.residuals(env().calib, s.db.host, s.case.persons, s.case.n_persons, want['poses'], s.host['triang'][1], mask)
    ref = R.stats([hres.reshape(-1, *hres.shape[-2:])])
    assert got['count'].tolist() == ref['count'].tolist() and got['count'].sum() > 0
    assert rc.same_bits(got['mid'], ref['mid']) and rc.same_bits(got['median'], ref['median'])
    assert np.allclose(got['sum'], ref['sum'], rtol=1e-12, atol=0)


def test_arguments():
    """11: what the entry point refuses, with a message; zero frames gives empty tensors."""
    MpeError = pkg('lib').MpeError
    s = setup('one frame')
    for kw, word in (({'max_iters': 0}, 'max_iters'), ({'max_iters': 65}, 'max_iters'), ({'step_tol': -1e-9}, 'step_tol'), ({'huber_px': -1.0}, 'huber_px')):
        with pytest.raises(MpeError) as err:
            s.device('triang', **kw)
        assert err.value.code == -1 and word in str(err.value), str(err.value)
    poses, flags, _ = s.dev['triang']
    with pytest.raises(MpeError) as err:
        import ctypes as C
        L = pkg('lib')
        a = L.mpe_refine_args()
        a.n_frames, a.pcap, a.n_joints, a.pose_f64, a.joint_flags, a.joint_mask, a.threshold = 2, s.eng.pcap, s.eng.J, 1, 1, 1, 0.5
        a.max_iters, a.step_tol, a.huber_px = 10, 0.0, 0.0
        s.eng._chk(s.eng.lib.mpe_refine_batch(s.eng.ctx, s.eng._stream(), C.byref(s.db.struct), C.byref(a)))
    assert err.value.code == -1 and 'frames' in str(err.value)
    with pytest.raises(ValueError):
        s.eng.refine(s.db, s.persons, s.n_persons, poses, flags, 'gt')
    with pytest.raises(ValueError):
        s.eng.refine(s.db, s.persons, s.n_persons, poses, flags, 'est')
    z = setup('zero frames')
    out = z.device('est')
    assert tuple(out['poses'].shape) == (0, z.eng.pcap, rc.J, 3) and all(out[k].numel() == 0 for k in KEYS)


def test_cli_refine_rows_and_line(capsys):
    """12 and 7: --refine adds the rows / the line and improves what it reports; without it the scripts do not touch the
    refinement at all (harness.refine made unimportable) and return what they return with it importable."""
    rep = importlib.import_module(HARNESS + 'reprojection_error')
    tri = importlib.import_module(HARNESS + 'metrics_from_triangulation')
    mlp = importlib.import_module(HARNESS + 'metrics_from_model')
    got = rep.main(SYN + ['--noise-px', '2', '--refine', '10'])
    rows = {kind: {key[1]: v for key, v in got.items() if isinstance(key, tuple) and key[0] == kind}
            for kind in ('triang', 'triang+refine', 'est', 'est+refine')}
    assert len(rows['triang']) == 5 and len(rows['triang+refine']) == 5
    assert {c: v[2] for c, v in rows['triang+refine'].items()} == {c: v[2] for c, v in rows['triang'].items()}
    assert {c: v[2] for c, v in rows['est+refine'].items()} == {c: v[2] for c, v in rows['est'].items()}
    sq = got['squared_sum']
    print(sq)
    assert sq['triang+refine'] < sq['triang']
    capsys.readouterr()
    out = tri.main(SYN + ['--noise-px', '2', '--refine', '10', '--refine-huber', '20'])
    line = [ln for ln in capsys.readouterr().out.splitlines() if ln.startswith('Refined')]
    print(line)
    r = out['refine']
    assert len(line) == 1 and r['solved'] > 0 and r['moved_share'] > 0 and r['mean_cost1'] < r['mean_cost0']
    assert set(mlp.main(SYN + ['--refine', '5'])['refine']) == {'solved', 'moved_share', 'mean_cost0', 'mean_cost1'}
    plain = {m: m.main(SYN + (['--device-metrics'] if m is not rep else [])) for m in (rep, tri, mlp)}
    name = '3d_multi_pose_estimator_amd.harness.refine'
    saved = sys.modules.pop(name, None)
    sys.modules[name] = None                     # import of the module now raises
    try:
        for m in (rep, tri, mlp):
            again = m.main(SYN + (['--device-metrics'] if m is not rep else []))
            assert 'refine' not in again and not any('refine' in str(k) for k in again)
            assert again.keys() == plain[m].keys()
            for k in again:
                if k in ('ap', 'mpjpe_mm', 'n_data') or isinstance(k, tuple):
                    assert again[k] == plain[m][k], (m.__name__, k)
    finally:
        del sys.modules[name]
        if saved is not None:
            sys.modules[name] = saved
