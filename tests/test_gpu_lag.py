"""mpe_lag_* (csrc/lag.hip, csrc/lag_pick.h, Engine.lag_estimator) against the host statement harness/lag.py: the sums and
counts of a pass bit for bit on every rig, both kinds of poses, several grids, at the table's edges and in any chunking;
the estimate bit for bit; the refusals; and the script end to end."""
import ctypes as C

import numpy as np
import pytest

import lag_cases as lc
from conftest import env, pkg

pytestmark = pytest.mark.gpu
_engines, _made = {}, {}
KEYS = ('cost', 'n_obs', 'n_skipped', 'n_support', 'n_unsupported')


def LG():
    return pkg('harness.lag')


def engine(variant):
    if variant not in _engines:
        e = env(variant)
        _engines[variant] = pkg('pipeline').Engine(e.params, e.calib, max_frames=64, max_persons_per_camera=11)
    return _engines[variant]


class Setup:
    """A scene on the device: the batch, the persons and the table of either kind as tensors; the estimators it made."""

    def __init__(self, scene):
        import torch
        self.scene = s = scene
        self.eng = eng = engine(s.variant)
        self.db = eng.to_device(s.pb)
        dev = lambda a: torch.from_numpy(np.ascontiguousarray(a)).cuda()      # noqa: E731
        self.persons, self.n_persons, self.ids = dev(s.persons), dev(s.n_persons), dev(s.ids)
        self.dev = {k: (dev(p), dev(f), m) for k, (p, f, m) in s.kinds.items()}
        self.ests = []

    def estimator(self, kind='triang', window=2, sub=4, huber_px=0.0, **kw):
        est = self.eng.lag_estimator(kind, window=window, sub=sub, huber_px=huber_px, pcap=self.scene.pcap, **kw)
        self.ests.append(est)
        return est

    def accumulate(self, est, kind='triang', frames=None):
        """The scene, or its frames [a, b) as a batch of their own, added to the estimator's pass against the whole table."""
        poses, flags, mask = self.dev[kind]
        if frames is None:
            return est.accumulate(self.db, 0, self.persons, poses, flags, self.n_persons, self.ids, joint_mask=mask)
        a, b = frames
        db = self.eng.to_device(self.scene.sub_batch(a, b))
        est.accumulate(db, a, self.persons[a:b].contiguous(), poses, flags, self.n_persons, self.ids, joint_mask=mask)


def setup(key, maker):
    if key not in _made:
        _made[key] = Setup(maker())
    return _made[key]


def messy(variant):
    lags = {'panoptic': (0, 1, -2, 0.5, 0.37), 'arplab': (0, 1, -1, 0.5, 0.25, -0.6), 'arprobot': (0, 1.25), 'ring23': [(i % 3 - 1) * 0.75 for i in range(23)]}
    frames = 22 if variant == 'ring23' else 14                # ring23 also takes W = 8: 17 frames and more for any support
    return setup(('messy', variant), lambda: lc.messy(variant, frames, lags[variant]))


def teardown_module(module):
    for s in _made.values():
        for est in s.ests:
            est.close()
    for eng in _engines.values():
        eng.close()
    _made.clear()
    _engines.clear()


def assert_same_sums(got, want, what):
    for k in KEYS:
        if not lc.same_bits(got[k], want[k]):
            bad = np.argwhere(np.asarray(got[k]) != np.asarray(want[k]))
            print(what, k, 'differing', len(bad), 'first', bad[:3].tolist(), got[k][tuple(bad[0])], want[k][tuple(bad[0])])
        assert lc.same_bits(got[k], want[k]), (what, k)


CASES = [('panoptic', 'triang', 0.0, 2, 4), ('panoptic', 'est', 5.0, 2, 4), ('panoptic', 'est', 0.0, 0, 1), ('panoptic', 'triang', 5.0, 1, 1),
         ('panoptic', 'triang', 0.0, 3, 3), ('panoptic', 'est', 5.0, 3, 3), ('arplab', 'triang', 5.0, 2, 4), ('arprobot', 'triang', 0.0, 2, 4),
         ('ring23', 'triang', 5.0, 8, 4), ('ring23', 'est', 0.0, 1, 1)]


@pytest.mark.parametrize('variant,kind,huber,window,sub', CASES)
def test_sums_bit_equal_to_host_statement(variant, kind, huber, window, sub):
    """lc.messy on every rig -- rows permuted from frame to frame, a track absent in the middle of windows, an id of -1, a
    duplicate id, n_persons negative and above pcap, joint flags dropped, a NaN coordinate in a neighbour frame only, a joint
    behind one camera at some entries only -- in one call from frame 0 to the table's end (the windows at either end
    reach outside), through LagEstimator.read, for both kinds of poses, both Huber settings and the grids (0, 1), (1, 1),
    (2, 4), (3, 3) (alpha = 1/3 and 2/3 are not exact: the three roundings matter) and, on 23 cameras, (8, 4): 23 * 65
    (camera, entry) pairs for 256 threads.  ARPLAB has six cameras, ARPLAB_ROBOT uses two of the six."""
    s = messy(variant)
    assert s.scene.pb.V == {'arplab': 6, 'arprobot': 2, 'ring23': 23}.get(variant, 5)
    est = s.estimator(kind, window, sub, huber)
    s.accumulate(est, kind)
    got, want = est.read(), s.scene.one_pass(window, sub, kind, huber)
    print(variant, kind, huber, window, sub, 'support', want['n_support'].tolist(), 'unsupported', want['n_unsupported'].tolist(),
          'skipped', want['n_skipped'].sum(axis=1).tolist())
    assert_same_sums(got, want, (variant, kind, huber, window, sub))
    assert got['cost'].shape == (s.scene.pb.V, 2 * window * sub + 1) and want['n_support'].max() > 20 and want['n_unsupported'].max() > 0
    if window in (1, 2, 3):
        c = 2 % s.scene.pb.V                                 # the joint behind this camera: skipped at some entries, summed at others
        assert 0 < want['n_skipped'][c].max() and (window == 1 or want['n_skipped'][c].min() == 0)     # W = 1: every entry meets it, in another frame
        assert np.array_equal(want['n_obs'][c] + want['n_skipped'][c], np.full(2 * window * sub + 1, want['n_support'][c]))
    est.reset()                                              # a reset, then the same pass: the first pass's bits again
    assert not est.read()['n_support'].any() and lc.same_bits(est.read()['cost'], np.zeros_like(got['cost']))
    s.accumulate(est, kind)
    assert_same_sums(est.read(), got, 'after reset')


def test_table_shorter_than_the_window():
    """n_table < 2W + 1: no window fits, so nothing is supported, every cost is 0.0 and every observation is counted as
    unsupported."""
    s = messy('panoptic')
    est = s.estimator('triang', 8, 1)
    s.accumulate(est)
    got, want = est.read(), s.scene.one_pass(8, 1)
    assert_same_sums(got, want, 'short table')
    assert not got['n_support'].any() and not got['n_obs'].any() and not got['n_skipped'].any() and got['n_unsupported'].min() > 300
    assert lc.same_bits(got['cost'], np.zeros((5, 17)))


@pytest.mark.parametrize('bodies', [10, 11])
def test_many_rows_on_23_cameras(bodies):
    """Ten and eleven rows at W = 4 on 23 cameras: the window's poses, (2W+1) * pcap * J * 3 doubles, stop fitting a
    workgroup's share of LDS about here, so a kernel that staged them would change its path between the two; this one reads
    the table from global memory and must give the statement's bits on either side."""
    s = setup(('rows', bodies), lambda: lc.Scene('ring23', 11, [(i % 3 - 1) * 1.25 for i in range(23)], n_bodies=bodies, seed=5400 + bodies,
                                                 pcap=bodies, permute=True, weave=0.03))
    est = s.estimator('triang', 4, 1, 5.0)
    s.accumulate(est)
    want = s.scene.one_pass(4, 1, huber_px=5.0)
    assert_same_sums(est.read(), want, ('rows', bodies))
    assert want['n_support'].min() > 100


def chunked():
    return setup('chunks', lambda: lc.Scene('panoptic', 40, (0, 1, -2, 0.5, 0.37), n_bodies=2, seed=5500, weave=0.05, permute=True))


def test_chunk_invariance_and_launch_count():
    """40 frames in one call and as 1 + 2 + 7 + 23 + 7 give the same bits (the statement's, too, chunked the same way); every
    non-empty call enqueues exactly two kernels and a call of zero frames none, leaving the state untouched."""
    s = chunked()
    whole, parts = s.estimator(huber_px=2.0), s.estimator(huber_px=2.0)
    s.accumulate(whole)
    assert whole.launches() == 2
    want, at = None, 0
    for n in (1, 2, 7, 23, 7):
        n0 = parts.launches()
        s.accumulate(parts, frames=(at, at + n))
        assert parts.launches() == n0 + 2
        want = s.scene.one_pass(2, 4, huber_px=2.0, frames=(at, at + n), sums=want)
        at += n
    assert at == 40
    got = whole.read()
    assert_same_sums(got, parts.read(), 'chunks')
    assert_same_sums(got, want, 'statement in chunks')
    assert_same_sums(got, s.scene.one_pass(2, 4, huber_px=2.0), 'statement')
    poses, flags, mask = s.dev['triang']
    empty = s.eng.to_device(s.eng.pack([]))
    n1 = whole.launches()
    whole.accumulate(empty, 7, s.persons[:0].contiguous(), poses, flags, s.n_persons, s.ids)
    assert whole.launches() == n1
    assert_same_sums(whole.read(), got, 'zero frames')


def test_estimate_equals_host_rule_and_finds_true_lags():
    """estimate() is lag_estimate_host on the sums read, bit for bit, at several min_obs (one of them above every count:
    MPE_LAG_FEW_OBS); on the straight-walk scene with lags on the grid the device finds the true indices at zero cost."""
    L = pkg('lib')
    for key, s, window, sub in (('chunks', chunked(), 2, 4), ('messy', messy('panoptic'), 3, 3)):
        est = s.estimator('triang', window, sub)
        s.accumulate(est)
        sums = est.read()
        for min_obs in (1, 50, 10 ** 7):
            got, want = est.estimate(min_obs), LG().lag_estimate_host(sums, window, sub, min_obs)
            for k in want:
                assert got[k].dtype == want[k].dtype and lc.same_bits(got[k], want[k]), (key, min_obs, k, got[k], want[k])
        assert np.all(got['status'] == L.MPE_LAG_FEW_OBS)
    s = setup('on grid', lambda: lc.Scene('panoptic', 16, (0, 1, -2, 0.5, 0.25), seed=5101))
    est = s.estimator('triang', 3, 4)
    s.accumulate(est)
    rep = est.estimate(50)
    assert rep['k_best'].tolist() == lc.true_k(s.scene, 4) and np.all(rep['cost_best'] == 0.0) and not rep['status'].any()
    assert lc.same_bits(rep['lag_grid'], np.array(s.scene.lags, np.float64))


def test_arguments_and_symbols():
    """MPE_ERR_INVALID for a frame count that is not the batch's, a joint count that is not the context's, a pcap that is
    not the state's, frame_start < 0, frames beyond the table, more frames than max_frames, a negative or NaN huber_px, a
    window or sub out of range at create, min_obs < 1; a closed estimator raises; the symbols resolve in the built library."""
    L = pkg('lib')
    s = chunked()
    eng = s.eng
    lib = C.CDLL(L.LIB_PATH)
    for sym in ('create', 'reset', 'destroy', 'batch', 'launches', 'read', 'estimate'):
        assert hasattr(lib, 'mpe_lag_' + sym)
    est = s.estimator()
    poses, flags, mask = s.dev['triang']

    def call(state=None, n_frames=40, n_joints=eng.J, pcap=s.scene.pcap, frame_start=0, n_table=40, huber=0.0):
        a = L.mpe_lag_args()
        a.n_frames, a.pcap, a.n_joints, a.pose_f64, a.joint_flags = n_frames, pcap, n_joints, 1, 1
        a.frame_start, a.n_table, a.joint_mask, a.threshold, a.huber_px = frame_start, n_table, mask, 0.5, huber
        a.d_persons, a.d_poses, a.d_flags, a.d_n_persons, a.d_tid = (t.data_ptr() for t in (s.persons, poses, flags, s.n_persons, s.ids))
        eng._chk(eng.lib.mpe_lag_batch(eng.ctx, eng._stream(), est.state if state is None else state, C.byref(s.db.struct), C.byref(a)))

    small = s.estimator(max_frames=39)
    for kw, word in (({'n_frames': 39}, 'frames'), ({'n_joints': 17}, 'joints'), ({'pcap': s.scene.pcap + 1}, 'pcap'), ({'frame_start': -1}, 'frame_start'),
                     ({'frame_start': 1}, 'table'), ({'n_table': 39}, 'table'), ({'state': small.state}, 'max_frames'),
                     ({'huber': float('nan')}, 'huber_px'), ({'huber': -1.0}, 'huber_px')):
        with pytest.raises(L.MpeError) as err:
            call(**kw)
        assert err.value.code == -1 and word in str(err.value), str(err.value)
    assert est.launches() == 0 and not est.read()['n_support'].any()
    call()
    assert est.launches() == 2
    for kw in ({'window': 9}, {'window': -1}, {'sub': 0}, {'sub': 9}):
        cfg = L.mpe_lag_config()
        cfg.pcap, cfg.n_joints, cfg.window, cfg.sub, cfg.pose_f64, cfg.joint_flags, cfg.max_frames = s.scene.pcap, eng.J, 2, 4, 1, 1, 64
        for k, v in kw.items():
            setattr(cfg, k, v)
        state = C.c_void_p()
        assert eng.lib.mpe_lag_create(eng.ctx, C.byref(cfg), C.byref(state)) == -1 and not state
        with pytest.raises(ValueError):
            eng.lag_estimator('triang', **kw)
    with pytest.raises(L.MpeError) as err:
        est.estimate(0)
    assert err.value.code == -1 and 'min_obs' in str(err.value)
    for bad in (lambda: eng.lag_estimator('gt'), lambda: eng.lag_estimator('triang', huber_px=-1.0), lambda: eng.lag_estimator('triang', max_frames=0)):
        with pytest.raises(ValueError):
            bad()
    with pytest.raises(ValueError):                          # a table of another kind
        est.accumulate(s.db, 0, s.persons, *s.dev['est'][:2], s.n_persons, s.ids)
    est.close()
    for closed in (est.read, est.estimate, est.launches, est.reset, lambda: s.accumulate(est)):
        with pytest.raises(RuntimeError):
            closed()


def test_script_on_synthetic_frames(capsys, monkeypatch):
    """The script on the scene of the host test's alternation (24 generated frames, lags 0, 2, -1, 0, 1; geometric matching,
    the device's triangulation and tracker): it ends with the true integer shifts, and prints the same lines when its
    passes go through the statement (--host-statement) as through the device."""
    a = lc.ALTERNATION
    argv = ['--synthetic', str(a['n_frames']), '--lags', ','.join(str(x) for x in a['lags']), '--persons', '2', '--lag-seed', str(a['seed']),
            '--weave', str(a['weave']), '--matcher', 'geometric', '--window', str(a['window']), '--sub', str(a['sub']), '--rounds', '4']
    rep = LG().main(argv)
    device = capsys.readouterr().out
    assert rep['total_shift'] == list(a['lags']) and not any(rep['rounds'][-1]['applied']) and len(rep['rounds']) <= 4
    host = LG().main(argv + ['--host-statement'])
    text = capsys.readouterr().out
    print(device)
    assert text == device and host['total_shift'] == rep['total_shift']
    lines = device.splitlines()
    assert lines[0].startswith('true lags') and lines[-1].startswith('integer shifts relative to')
    assert sum(ln.startswith('round 1 camera ') for ln in lines) == 5
