"""mpe_calib_* (csrc/calib.hip, csrc/calib_solve.h, Engine.calibrator) against the host statement harness/calibrate.py: the
sums of a pass bit for bit, on either side of the kernel's tiling border, in any chunking; the step's delta bit for bit
over a loop of passes; the refusals; and the script end to end."""
import ctypes as C
import os

import numpy as np
import pytest

import calib_cases as cc
from conftest import env, pkg

pytestmark = pytest.mark.gpu
_made = {}


def CB():
    return pkg('harness.calibrate')


class Setup:
    """A scene on the device: an engine of the scene's rig whose Pcap the scene is built for, the batch, persons and the
    scene's poses as tensors."""

    def __init__(self, variant, maker, ppc=2, **kw):
        import torch
        e = env(variant)
        self.eng = eng = pkg('pipeline').Engine(e.params, e.calib, max_frames=64, max_persons_per_camera=ppc)
        self.scene = s = maker(pcap=eng.pcap, **kw)
        self.db = eng.to_device(s.pb)
        self.persons, self.n_persons = torch.from_numpy(s.persons).cuda(), torch.from_numpy(s.n_persons).cuda()
        kinds = getattr(s, 'kinds', {'triang': (s.truth, s.flags, cc.ALL_JOINTS)})
        self.host = kinds
        self.dev = {k: (torch.from_numpy(np.ascontiguousarray(p)).cuda(), torch.from_numpy(np.ascontiguousarray(f)).cuda(), m)
                    for k, (p, f, m) in kinds.items()}
        self.cals = []

    def calibrator(self, kind='triang', **kw):
        kw.setdefault('min_obs', 6)
        cal = self.eng.calibrator(kind, **kw)
        self.cals.append(cal)
        return cal

    def accumulate(self, cal, kind='triang', frames=None):
        """The scene, or its frames [a, b) as a batch of their own, added to the calibrator's pass."""
        poses, flags, mask = self.dev[kind]
        if frames is None:
            return cal.accumulate(self.db, self.persons, self.n_persons, poses, flags, joint_mask=mask)
        a, b = frames
        db = self.eng.to_device(self.scene.sub_batch(a, b))
        cal.accumulate(db, self.persons[a:b].contiguous(), self.n_persons[a:b].contiguous(), poses[a:b].contiguous(),
                       flags[a:b].contiguous(), joint_mask=mask)

    def statement(self, E, kind='triang', huber_px=0.0, sums=None):
        poses, flags, mask = self.host[kind]
        return self.scene.one_pass(E, sums=sums, poses=poses, flags=flags, mask=mask, huber_px=huber_px)


def setup(key, *a, **kw):
    if key not in _made:
        _made[key] = Setup(*a, **kw)
    return _made[key]


def chunks():
    return setup('chunks', 'panoptic', lambda pcap: cc.Scene('panoptic', 16, 3, seed=4200, noise_px=1.5, pcap=pcap), ppc=3)


def teardown_module(module):
    for s in _made.values():
        for cal in s.cals:
            cal.close()
        s.eng.close()
    _made.clear()


def assert_same_sums(got, want, what):
    for k in ('acc', 'n_obs', 'n_skipped'):
        if not cc.same_bits(got[k], want[k]):
            bad = np.argwhere(np.asarray(got[k]) != np.asarray(want[k]))
            print(what, k, 'differing', len(bad), 'first', bad[:3].tolist(), got[k][tuple(bad[0])], want[k][tuple(bad[0])])
        assert cc.same_bits(got[k], want[k]), (what, k)


CASES = [('panoptic', kind, huber, moved) for kind in ('est', 'triang') for huber in (0.0, 5.0) for moved in (False, True)]
CASES.append(('arplab', 'triang', 5.0, True))
CASES.append(('arprobot', 'triang', 5.0, True))              # six cameras configured, calibration indices 4 and 5 used


@pytest.mark.parametrize('variant,kind,huber,moved', CASES)
def test_sums_bit_equal_to_host_statement(variant, kind, huber, moved):
    """8: 3 frames of the rig x 2 persons -- a person missing a camera, a joint absent, a confidence below the threshold and
    one at it, Pcap above the persons, a person / joint flag off -- through mpe_calib_read, for both kinds of poses, both
    Huber settings, the engine's own extrinsics and a moved set; ARPLAB has six cameras, ARPLAB_ROBOT uses two of the six."""
    s = setup(('small', variant), variant, lambda **kw: cc.small(variant, **kw), ppc=3 if variant == 'arprobot' else 2)   # two cameras: Pcap = ppc
    assert s.scene.pb.V == {'arplab': 6, 'arprobot': 2}.get(variant, 5) and s.eng.pcap > 2
    cal = s.calibrator(kind, huber_px=huber)
    E = CB().start_extrinsics(s.scene.calib)
    if moved:
        E = cc.perturbed_start(E, 0.7, 15.0, 21)
        cal.set_extrinsics(E)
    s.accumulate(cal, kind)
    got, want = cal.read(), s.statement(E, kind, huber)
    print(variant, kind, huber, moved, 'n_obs', want['n_obs'].tolist(), 'skipped', want['n_skipped'].tolist())
    assert_same_sums(got, want, (variant, kind, huber, moved))
    assert want['n_obs'].min() > 20 and len(set(want['n_obs'].tolist())) > 1
    acc, tri = cal.extrinsics()
    assert cc.same_bits(acc, E) and cc.same_bits(tri, E)
    idx = CB().engine_cameras(s.scene.calib)
    assert cc.same_bits(np.asarray(s.eng.calib.P, np.float64)[idx], CB().start_extrinsics(s.scene.calib))     # the engine's own: untouched
    if variant == 'arprobot':                                # the accepted extrinsics go back to the rows of their own cameras
        new, old = np.asarray(cal.calibration().P, np.float64), np.asarray(s.eng.calib.P, np.float64)
        assert idx == [4, 5] and cc.same_bits(new[idx], E) and cc.same_bits(new[:4], old[:4]) and not cc.same_bits(new[idx], old[idx])


def test_tiling_borders():
    """9: the records of a frame fit LDS up to 384 / V (person, joint) pairs -- 76 at five cameras, so four persons (72
    pairs) are one tile, five (90) are two with the border inside a person, and ten (180) are three; one batch holds
    all three, with a joint behind a moved camera (skipped and counted) in the second tile."""
    def maker(pcap):
        s = cc.Scene('panoptic', 4, [4, 5, 10, 1], seed=4400, noise_px=1.0, pcap=pcap)
        s.truth[1, 4, 9] = -s.E_true[2][:, :3].T @ s.E_true[2][:, 3] - s.E_true[2][2, :3]
        return s
    s = setup('tiles', 'panoptic', maker, ppc=10)
    assert s.eng.pcap >= 10
    for huber in (0.0, 5.0):
        cal = s.calibrator(huber_px=huber)
        E = cc.perturbed_start(s.scene.E_true, 0.4, 8.0, 33)
        cal.set_extrinsics(E)
        s.accumulate(cal)
        got, want = cal.read(), s.statement(E, huber_px=huber)
        assert_same_sums(got, want, ('tiles', huber))
        assert want['n_skipped'][2] >= 1 and want['n_obs'].min() > 300
    for f in range(4):                                       # each shape on its own
        cal.reset()
        E = CB().start_extrinsics(s.scene.calib)
        s.accumulate(cal, frames=(f, f + 1))
        assert_same_sums(cal.read(), s.scene.one_pass(E, frames=(f, f + 1), huber_px=5.0), ('frame', f))


def test_chunk_invariance_and_launch_count():
    """10: 16 frames in one call and as 5 + 10 + 1 give the same bits (the statement's, too); a call of zero frames leaves
    the state untouched; a 1-frame call enqueues as many kernels as a 64-frame call."""
    import torch
    s = chunks()
    E = cc.perturbed_start(s.scene.E_true, 0.3, 5.0, 3)
    whole, parts = s.calibrator(huber_px=2.0), s.calibrator(huber_px=2.0)
    whole.set_extrinsics(E)
    parts.set_extrinsics(E)
    s.accumulate(whole)
    n0 = parts.launches()
    for a, b in ((0, 5), (5, 15), (15, 16)):
        s.accumulate(parts, frames=(a, b))
    per_call = (parts.launches() - n0) // 3
    assert parts.launches() - n0 == 3 * per_call and whole.launches() == per_call
    got = whole.read()
    assert_same_sums(got, parts.read(), 'chunks')
    assert_same_sums(got, s.statement(E, huber_px=2.0), 'statement')
    # zero frames: nothing is enqueued, nothing changes
    poses, flags, mask = s.dev['triang']
    empty = s.eng.to_device(s.eng.pack([]))
    n1 = whole.launches()
    whole.accumulate(empty, s.persons[:0].contiguous(), s.n_persons[:0].contiguous(), poses[:0].contiguous(), flags[:0].contiguous())
    assert whole.launches() == n1
    assert_same_sums(whole.read(), got, 'zero frames')
    # 64 frames in one call
    big = setup('big', 'panoptic', lambda pcap: cc.Scene('panoptic', 64, 2, seed=4500, exact=False, pcap=pcap))
    cal = big.calibrator()
    big.accumulate(cal)
    assert cal.launches() == per_call == 2
    assert_same_sums(cal.read(), big.statement(CB().start_extrinsics(big.scene.calib)), '64 frames')
    torch.cuda.synchronize()


def test_loop_of_passes_against_the_host_step():
    """11: 8 frames of 5 x 2, every camera moved, 6 passes: after every device step the device's trial extrinsics go to
    the host statement; that pass's sums are bit-equal, and the host step on those sums gives the same delta bit for bit
    and the same trial within 1e-14."""
    s = setup('loop', 'panoptic', lambda pcap: cc.Scene('panoptic', 8, 2, seed=4600, noise_px=1.0, pcap=pcap))
    E0 = cc.perturbed_start(s.scene.E_true, 0.8, 15.0, 44)
    cal = s.calibrator()
    cal.set_extrinsics(E0)
    host = CB().HostCalibrator(E0)
    costs = []
    for it in range(6):
        trial = cal.extrinsics()[1]
        s.accumulate(cal)
        want = s.statement(trial)
        assert_same_sums(cal.read(), want, ('pass', it))
        rep = cal.step(1e-12, 1e-12)
        for c in range(5):                                   # the host takes the device's trial, bit for bit
            host.cams[c].Et = trial[c].copy()
        hrep = CB().calib_step_host(host, want, 1e-12, 1e-12)
        acc, new_trial = cal.extrinsics()
        for k in ('status', 'passes', 'n_obs', 'n_skipped'):
            assert np.array_equal(rep[k], hrep[k]), (it, k, rep[k], hrep[k])
        for k in ('cost_start', 'cost', 'lambda', 'last_rot', 'last_trans', 'delta'):
            assert cc.same_bits(rep[k], hrep[k]), (it, k, rep[k], hrep[k])
        for c in range(5):
            d = list(hrep['delta'][c])
            assert [x.hex() for x in rep['delta'][c]] == [float(x).hex() for x in d], (it, c)
            assert np.abs(new_trial[c] - host.cams[c].Et).max() <= 1e-14 and cc.same_bits(acc[c], host.cams[c].Ea)
        costs.append(rep['cost'].copy())
        assert cc.same_bits(cal.read()['acc'], np.zeros((5, 28))) and not cal.read()['n_obs'].any()            # zeroed by the step
    print('cost per camera, pass by pass', np.stack(costs).round(3).tolist())
    assert np.all(costs[-1] < costs[0]) and np.all(np.diff(np.stack(costs), axis=0) <= 0)


def test_arguments_and_symbols():
    """12: MPE_ERR_INVALID for a frame count that is not the batch's, a joint count that is not the context's, a NaN or
    negative huber_px, min_obs below 6; the new symbols resolve in the built library."""
    L = pkg('lib')
    s = chunks()
    lib = C.CDLL(L.LIB_PATH)
    for sym in ('create', 'destroy', 'reset', 'set_extrinsics', 'get_extrinsics', 'batch', 'read', 'step', 'launches'):
        assert hasattr(lib, 'mpe_calib_' + sym)
    cal = s.calibrator()
    poses, flags, mask = s.dev['triang']

    def call(n_frames=16, n_joints=s.eng.J, huber=0.0):
        a = L.mpe_calib_args()
        a.n_frames, a.pcap, a.n_joints, a.pose_f64, a.joint_flags, a.joint_mask, a.threshold = n_frames, s.eng.pcap, n_joints, 1, 1, mask, 0.5
        a.huber_px = huber
        a.d_persons, a.d_n_persons, a.d_poses, a.d_flags = s.persons.data_ptr(), s.n_persons.data_ptr(), poses.data_ptr(), flags.data_ptr()
        s.eng._chk(s.eng.lib.mpe_calib_batch(s.eng.ctx, s.eng._stream(), cal.state, C.byref(s.db.struct), C.byref(a)))

    for kw, word in (({'n_frames': 15}, 'frames'), ({'n_joints': 17}, 'joints'), ({'huber': float('nan')}, 'huber_px'), ({'huber': -1.0}, 'huber_px')):
        with pytest.raises(L.MpeError) as err:
            call(**kw)
        assert err.value.code == -1 and word in str(err.value), str(err.value)
    assert not cal.read()['n_obs'].any()
    call()
    few = s.calibrator(min_obs=5)
    s.accumulate(few)
    with pytest.raises(L.MpeError) as err:
        few.step()
    assert err.value.code == -1 and 'min_obs' in str(err.value)
    # a pass that does not see the first pass's data
    rep = cal.step()
    assert rep['n_obs'].min() > 0 and np.all(rep['status'] & L.MPE_CALIB_ACCEPTED)
    s.accumulate(cal, frames=(0, 5))
    with pytest.raises(L.MpeError) as err:
        cal.step()
    assert err.value.code == -1 and 'same data' in str(err.value)
    with pytest.raises(ValueError):
        s.eng.calibrator('gt')
    for hold in ((99,), ('no such camera',)):
        with pytest.raises(ValueError):
            s.eng.calibrator('triang', hold=hold)
    held = s.calibrator(hold=(s.scene.names[0],))
    s.accumulate(held)
    rep = held.step()
    assert rep['status'][0] == L.MPE_CALIB_HELD and not (rep['status'][1:] & L.MPE_CALIB_HELD).any()
    cal.close()
    with pytest.raises(RuntimeError):
        cal.read()


def test_script_on_synthetic_frames(tmp_path, capsys):
    """13: the script on 32 generated frames with one camera moved by 0.5 degrees and 10 mm, geometric matching, 3 rounds of
    up to 8 passes: for that camera the RMS reprojection error falls and so does its distance to the true extrinsics (no
    magnitude is fixed); --out reads back through load_transform_manager."""
    cal = pkg('calibration')
    out = str(tmp_path / 'tm_refined.json')
    rep = CB().main(['--synthetic', '32', '--matcher', 'geometric', '--perturb-deg', '0.5', '--perturb-mm', '10', '--rounds', '3',
                     '--passes', '8', '--out', out])
    text = capsys.readouterr().out
    print(text)
    c = len(rep['cameras']) - 1                              # the moved camera: the last
    assert rep['true_rot_deg_before'][c] > 0.49 and rep['true_trans_mm_before'][c] > 1.0
    assert all(rep['true_rot_deg_before'][k] < 1e-9 and rep['true_trans_mm_before'][k] == 0.0 for k in range(c))
    assert rep['rms_after'][c] < rep['rms_before'][c]
    assert rep['true_rot_deg_after'][c] < rep['true_rot_deg_before'][c] and rep['true_trans_mm_after'][c] < rep['true_trans_mm_before'][c]
    assert rep['rot_deg'][0] < 1e-9 and rep['trans_mm'][0] == 0.0 and rep['hold'] == [rep['cameras'][0]]
    assert sum(ln.startswith('camera ') for ln in text.splitlines()) == len(rep['cameras']) and os.path.exists(out)
    back = cal.Calibration(env().params, cal.load_transform_manager(out))
    assert cc.same_bits(back.P, rep['calibration'].P) and cc.same_bits(back.T_i, rep['calibration'].T_i)
