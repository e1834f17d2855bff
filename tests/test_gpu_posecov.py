"""mpe_posecov_batch (csrc/posecov.hip, Engine.pose_covariance) against its host statement harness/uncertainty.py, bit for
bit; the calibration of the covariance on the device's own refinement; and the --uncertainty flags of the two metrics scripts
end to end."""
import ctypes as C
import importlib
import re
import sys

import numpy as np
import pytest

import refine_cases as rc
from conftest import env, pkg

pytestmark = pytest.mark.gpu
HARNESS = '3d_multi_pose_estimator_amd.harness.'
KEYS = ('cov', 'sigma', 'status', 'n_views')
SYN = ['--synthetic', '16', '--random-weights', '--teacher-scores', '--batch', '16']
_made = {}


class Setup:
    """A case on the device: the engine, the batch, persons, and both kinds of poses (the triangulation is the device's
    own) as tensors and as the host arrays the statement takes."""

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

    def device(self, kind, sigma_px=1.0, joint_mask=None, poses=None, flags=None, **kw):
        p, f, mask = self.dev[kind]
        return self.eng.pose_covariance(self.db, self.persons, self.n_persons, p if poses is None else poses, f if flags is None else flags, kind,
                                        sigma_px, joint_mask=joint_mask, **kw)

    def statement(self, kind, sigma_px=1.0, joint_mask=None, poses=None, **kw):
        p, f, mask = self.host[kind]
        return pkg('harness.uncertainty').pose_covariance(self.case.calib, self.db.host, self.case.persons, self.case.n_persons,
                                                          p if poses is None else poses, f, mask if joint_mask is None else joint_mask, sigma_px, **kw)


def setup(name):
    if name not in _made:
        _made[name] = Setup(name)
    return _made[name]


def teardown_module(module):
    for s in _made.values():
        s.eng.close()
    _made.clear()


def host_of(out):
    return {k: v.cpu().numpy() for k, v in out.items()}


def assert_same(got, want, what, keys=KEYS):
    for k in keys:
        g, w = got[k], want[k]
        assert g.shape == w.shape and g.dtype == w.dtype, (what, k, g.shape, w.shape, g.dtype, w.dtype)
        if not rc.same_bits(g, w):
            bad = np.argwhere(g != w)
            print(what, k, 'differing', len(bad), 'first', bad[:3].tolist(), g[tuple(bad[0])], w[tuple(bad[0])])
        assert rc.same_bits(g, w), (what, k)


@pytest.mark.parametrize('kind', ['triang', 'est'])
@pytest.mark.parametrize('name', rc.NAMES)
def test_bit_equal_to_host_statement(name, kind):
    """7: cov, sigma, status and n_views, every entry, for huber_px in {0, 5}, sigma_px in {1.0, 2.5} and gate_m in {0, the
    case's median sigma}; the gated flags into a tensor of their own and over the input flags."""
    U = pkg('harness.uncertainty')
    s = setup(name)
    seen = 0
    for huber in (0.0, 5.0):
        for sigma_px in (1.0, 2.5):
            want = s.statement(kind, sigma_px, huber_px=huber)
            assert_same(host_of(s.device(kind, sigma_px, huber_px=huber)), want, (name, kind, huber, sigma_px))
            done = (want['status'] & U.COMPUTED) != 0
            st = want['status']
            print(name, kind, 'huber', huber, 'sigma_px', sigma_px, 'joints', st.size, 'computed', int(done.sum()), 'few views', int((st == U.FEW_VIEWS).sum()),
                  'bad pose', int((st == U.BAD_POSE).sum()), 'singular', int((st == U.SINGULAR).sum()))
            if not done.any():
                continue
            gate = float(np.median(want['sigma'][done]))
            tri = kind == 'triang'
            want = s.statement(kind, sigma_px, huber_px=huber, gate_m=gate, flags_out=tri)
            gated = (want['status'] & U.GATED) != 0
            assert 0 < gated.sum() < done.sum()
            seen += int(gated.sum())
            if not tri:
                assert_same(host_of(s.device(kind, sigma_px, huber_px=huber, gate_m=gate)), want, (name, kind, huber, sigma_px, 'gate'))
                continue
            flags = s.dev[kind][1]
            before = flags.clone()
            got = s.device(kind, sigma_px, huber_px=huber, gate_m=gate, flags_out=True)
            assert got['flags'].data_ptr() != flags.data_ptr() and bool((flags == before).all())
            assert_same(host_of(got), want, (name, kind, huber, sigma_px, 'gate, own flags'), KEYS + ('flags',))
            mine = flags.clone()
            got = s.device(kind, sigma_px, flags=mine, huber_px=huber, gate_m=gate, flags_out=mine)
            assert got['flags'].data_ptr() == mine.data_ptr()
            assert_same(host_of(got), want, (name, kind, huber, sigma_px, 'gate, flags in place'), KEYS + ('flags',))
            assert int((before != 0).sum()) - int((mine != 0).sum()) == gated.sum()
    if name != 'zero frames':
        assert seen > 0                                                   # GATED on the device
    if name == 'hand made':
        assert (st == U.BAD_POSE).sum() == 1 and st[0, 2, 8] == U.BAD_POSE and (want['n_views'] == 2).any()
        assert (st == U.FEW_VIEWS).any() or kind == 'triang'
    if name in rc.RIGS:
        info = rc.check(s.case)
        print(name, info)
        nv = want['n_views'][..., 5]                                    # joint 5 is in both masks
        assert s.eng.V == info['V'] and s.eng.pcap == s.case.pcap == info.get('pcap', s.eng.pcap)
        rows = [0, 1, 2] if kind == 'est' else [0, 2]                   # a person in one camera has no triangulated joint
        assert nv[-1, rows].tolist() == [info['n_views'][-1][p] for p in rows]
        if name == 'ring23':
            # person 2 is seen by cameras 19 and 22 alone, lanes that own no joint: computed from exactly those two
            assert (want['n_views'][:, 2][(st[:, 2] & U.COMPUTED) != 0] == 2).all() and ((st[:, 2] & U.COMPUTED) != 0).sum() >= 30
            assert (want['n_views'][:2, :2] == 23)[(st[:2, :2] & U.COMPUTED) != 0].all()
            if kind == 'est':
                assert (st[2, 1] == U.FEW_VIEWS).any() and not (st[:, [0, 2]] == U.FEW_VIEWS).any()


@pytest.mark.parametrize('kind', ['triang', 'est'])
def test_frames_apart_and_one_joint(kind):
    """8: the batch frame by frame gives the whole batch's bits, and a one-joint mask leaves every other joint at status 0,
    sigma -1 and cov 0."""
    s = setup('messy')
    whole = host_of(s.device(kind, 2.0, huber_px=5.0))
    assert_same(whole, s.statement(kind, 2.0, huber_px=5.0), 'whole')
    poses, flags, _ = s.dev[kind]
    for f in range(len(s.case.processed)):
        db = s.eng.to_device(s.eng.pack(s.case.processed[f:f + 1]))
        one = s.eng.pose_covariance(db, s.persons[f:f + 1].contiguous(), s.n_persons[f:f + 1].contiguous(), poses[f:f + 1].contiguous(),
                                    flags[f:f + 1].contiguous(), kind, 2.0, huber_px=5.0)
        assert_same(host_of(one), {k: whole[k][f:f + 1] for k in KEYS}, ('frame', f))
    j3 = host_of(s.device(kind, 2.0, joint_mask=1 << 3))
    assert_same(j3, s.statement(kind, 2.0, joint_mask=1 << 3), 'joint 3')
    others = [j for j in range(rc.J) if j != 3]
    assert not j3['status'][:, :, others].any() and np.all(j3['sigma'][:, :, others] == -1.0) and not j3['cov'][:, :, others].any()
    assert not j3['n_views'][:, :, others].any() and (j3['status'][:, :, 3] & 1).any()


@pytest.mark.parametrize('kind', ['triang', 'est'])
def test_calibration_on_the_device(kind):
    """9: Engine.refine (64 iterations, step_tol 1e-9) and Engine.pose_covariance on its output, queued on one stream with
    nothing in between: over the SOLVED and COMPUTED joints of 5x10 the mean Mahalanobis distance from the truth is 3 to
    five standard errors, 5 * sqrt(6 / n)."""
    U = pkg('harness.uncertainty')
    s = setup('5x10')
    poses, flags, _ = s.dev[kind]
    ref = s.eng.refine(s.db, s.persons, s.n_persons, poses, flags, kind, max_iters=64, step_tol=1e-9)
    out = s.eng.pose_covariance(s.db, s.persons, s.n_persons, ref['poses'], flags, kind, 1.0)
    ref, out = host_of(ref), host_of(out)
    assert_same(out, s.statement(kind, 1.0, poses=ref['poses']), 'after refine')
    use = ((ref['status'] & 1) != 0) & ((out['status'] & U.COMPUTED) != 0)
    err = (ref['poses'].astype(np.float64) - s.case.truth)[use]
    d2 = np.einsum('ni,ni->n', err, np.linalg.solve(U.full(out['cov'][use]), err[..., None])[..., 0])
    n = d2.size
    print(kind, 'n', n, 'mean d2 %.4f' % d2.mean(), 'bound %.4f' % (5 * np.sqrt(6 / n)))
    assert n > 1000 and np.array_equal(use, (ref['status'] & 1) != 0)
    assert abs(d2.mean() - 3.0) <= 5 * np.sqrt(6 / n)


def test_arguments():
    """10: what the entry point refuses, with a message; flags_out with 'est'; kind 'gt'; zero frames; a closed engine."""
    L = pkg('lib')
    MpeError = L.MpeError
    s = setup('one frame')
    nan, inf = float('nan'), float('inf')
    for sigma_px, kw, word in ((0.0, {}, 'sigma_px'), (-1.0, {}, 'sigma_px'), (inf, {}, 'sigma_px'), (nan, {}, 'sigma_px'), (1.0, {'gate_m': -1e-3}, 'gate_m'),
                               (1.0, {'gate_m': nan}, 'gate_m'), (1.0, {'huber_px': -1.0}, 'huber_px'), (1.0, {'huber_px': nan}, 'huber_px')):
        with pytest.raises(MpeError) as err:
            s.device('triang', sigma_px, **kw)
        assert err.value.code == -1 and word in str(err.value), str(err.value)
    poses, flags, _ = s.dev['est']
    good = s.device('est')

    def raw(**fields):
        a = L.mpe_posecov_args()
        a.n_frames, a.pcap, a.n_joints, a.pose_f64, a.joint_flags, a.joint_mask, a.threshold = 1, s.eng.pcap, s.eng.J, 0, 0, 1 << 5, 0.5
        a.huber_px, a.sigma_px, a.gate_m = 0.0, 1.0, 0.0
        a.d_persons, a.d_n_persons, a.d_poses, a.d_flags = s.persons.data_ptr(), s.n_persons.data_ptr(), poses.data_ptr(), flags.data_ptr()
        a.d_cov, a.d_sigma, a.d_status, a.d_n_views = (good[k].data_ptr() for k in KEYS)
        for k, v in fields.items():
            setattr(a, k, v)
        s.eng._chk(s.eng.lib.mpe_posecov_batch(s.eng.ctx, s.eng._stream(), C.byref(s.db.struct), C.byref(a)))
    raw()
    for fields, word in (({'n_frames': 2}, 'frames'), ({'n_joints': s.eng.J - 1}, 'joints'), ({'d_flags_out': good['status'].data_ptr()}, 'd_flags_out'),
                         ({'d_cov': None}, 'NULL')):
        with pytest.raises(MpeError) as err:
            raw(**fields)
        assert err.value.code == -1 and word in str(err.value), str(err.value)
    with pytest.raises(ValueError):
        s.device('est', gate_m=0.01, flags_out=True)
    with pytest.raises(ValueError):
        s.eng.pose_covariance(s.db, s.persons, s.n_persons, poses, flags, 'gt', 1.0)
    with pytest.raises(ValueError):
        s.eng.pose_covariance(s.db, s.persons, s.n_persons, poses, flags, 'triang', 1.0)
    tp, tf, _ = s.dev['triang']
    with pytest.raises(ValueError):
        s.device('triang', gate_m=0.01, flags_out=tf[..., 0].contiguous())
    z = setup('zero frames')
    out = z.device('triang', gate_m=0.01, flags_out=True)
    assert tuple(out['cov'].shape) == (0, z.eng.pcap, rc.J, 6) and all(out[k].numel() == 0 for k in KEYS + ('flags',))
    e = env()
    eng = pkg('pipeline').Engine(e.params, e.calib, max_frames=16, max_persons_per_camera=4)
    assert eng.pcap == s.eng.pcap
    eng.close()
    with pytest.raises(MpeError) as err:
        eng.pose_covariance(s.db, s.persons, s.n_persons, poses, flags, 'est', 1.0)
    assert err.value.code == -1


def uncertainty_lines(text):
    return [ln for ln in text.splitlines() if ln.startswith('Uncertainty')]


def test_cli_uncertainty_line_and_gate(capsys):
    """11: --uncertainty adds its line and its numbers; the gate at the median the ungated run prints drops joints; the
    model script refuses the gate; without the flag the scripts do not touch harness.uncertainty at all."""
    tri = importlib.import_module(HARNESS + 'metrics_from_triangulation')
    mlp = importlib.import_module(HARNESS + 'metrics_from_model')
    base = SYN + ['--noise-px', '2', '--refine', '10', '--uncertainty', '2']
    capsys.readouterr()
    plain = tri.main(base)
    lines = uncertainty_lines(capsys.readouterr().out)
    with capsys.disabled():
        print(lines)
    assert len(lines) == 1 and lines[0].startswith('Uncertainty (sigma 2 px): ')
    r = plain['uncertainty']
    median = re.search(r'sigma median ([0-9.]+) mm', lines[0]).group(1)
    assert abs(float(median) - r['median_mm']) < 1e-3 and r['computed'] > 0 and r['gated'] == 0 and r['median_mm'] <= r['p95_mm'] <= r['max_mm']
    bound = 5 / np.sqrt(2 * r['pooled_dof'])
    with capsys.disabled():
        print('pooled pixel sigma', r['pooled_sigma_px'], 'dof', r['pooled_dof'], 'bound', bound)
    assert 'pooled pixel sigma' in lines[0] and abs(r['pooled_sigma_px'] / 2.0 - 1.0) <= bound
    gated = tri.main(base + ['--uncertainty-gate', median])
    lines = uncertainty_lines(capsys.readouterr().out)
    with capsys.disabled():
        print(lines, 'joints flagged', r['joints_flagged'], '->', gated['uncertainty']['joints_flagged'])
    g = gated['uncertainty']
    assert len(lines) == 1 and 'gated' in lines[0] and g['gated'] > 0 and g['computed'] == r['computed']
    assert g['joints_flagged'] == r['joints_flagged'] - g['gated'] < r['joints_flagged']      # no more joints go on to be scored
    assert gated['ap'] != plain['ap'] or gated['mpjpe_mm'] != plain['mpjpe_mm']
    got = mlp.main(SYN + ['--uncertainty', '2'])
    lines = uncertainty_lines(capsys.readouterr().out)
    assert len(lines) == 1 and 'pooled' not in lines[0] and got['uncertainty']['computed'] > 0
    with pytest.raises(ValueError):
        mlp.main(SYN + ['--uncertainty', '2', '--uncertainty-gate', '5'])
    with pytest.raises(ValueError):
        tri.main(SYN + ['--uncertainty', '-1'])
    capsys.readouterr()
    with_refine = tri.main(SYN + ['--noise-px', '2', '--refine', '10'])
    for k in ('ap', 'mpjpe_mm', 'refine'):
        assert with_refine[k] == plain[k], k                             # measuring changes nothing that is scored
    plain = {m: m.main(SYN + ['--device-metrics']) for m in (tri, mlp)}
    name = '3d_multi_pose_estimator_amd.harness.uncertainty'
    saved = sys.modules.pop(name, None)
    sys.modules[name] = None                     # import of the module now raises
    try:
        for m in (tri, mlp):
            again = m.main(SYN + ['--device-metrics'])
            assert 'uncertainty' not in again and again.keys() == plain[m].keys()
            for k in again:
                if k in ('ap', 'mpjpe_mm', 'n_data'):
                    assert again[k] == plain[m][k], (m.__name__, k)
        assert not uncertainty_lines(capsys.readouterr().out)
    finally:
        del sys.modules[name]
        if saved is not None:
            sys.modules[name] = saved
