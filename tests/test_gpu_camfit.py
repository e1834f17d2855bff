"""mpe_camfit_* (csrc/camfit.hip, csrc/camfit_solve.h, Engine.camera_fitter) against the host statement harness/camfit.py:
the 105 sums of a pass bit for bit, its pose block against mpe_calib_batch, on either side of the kernel's tiling border,
in any chunking; the step bit for bit over a loop of passes; the refusals; and the script end to end."""
import ctypes as C
import os

import numpy as np
import pytest

import calib_cases as cc
import camfit_cases as fc
from conftest import env, pkg

pytestmark = pytest.mark.gpu
_made = {}
TILE_RECORDS = 180                                # csrc/camfit.hip CamfitSums::RECORDS: records per LDS tile; a tile holds 180 // V (p, j) pairs


def CF():
    return pkg('harness.camfit')


class Setup:
    """A scene on the device: an engine of the scene's rig whose Pcap the scene is built for, the batch, persons and the
    scene's poses as tensors."""

    def __init__(self, variant, maker, ppc=2, max_frames=64):
        import torch
        e = env(variant)
        self.eng = eng = pkg('pipeline').Engine(e.params, e.calib, max_frames=max_frames, max_persons_per_camera=ppc)
        self.scene = s = maker(pcap=eng.pcap)
        self.db = eng.to_device(s.pb)
        self.persons, self.n_persons = torch.from_numpy(s.persons).cuda(), torch.from_numpy(s.n_persons).cuda()
        kinds = getattr(s, 'kinds', {'triang': (s.truth, s.flags, cc.ALL_JOINTS)})
        self.host = kinds
        self.dev = {k: (torch.from_numpy(np.ascontiguousarray(p)).cuda(), torch.from_numpy(np.ascontiguousarray(f)).cuda(), m)
                    for k, (p, f, m) in kinds.items()}
        self.made = []

    def fitter(self, kind='triang', **kw):
        kw.setdefault('min_obs', 13)
        fit = self.eng.camera_fitter(kind, **kw)
        self.made.append(fit)
        return fit

    def calibrator(self, kind='triang', **kw):
        kw.setdefault('min_obs', 6)
        cal = self.eng.calibrator(kind, **kw)
        self.made.append(cal)
        return cal

    def accumulate(self, fit, kind='triang', frames=None):
        """The scene, or its frames [a, b) as a batch of their own, added to the pass."""
        poses, flags, mask = self.dev[kind]
        if frames is None:
            return fit.accumulate(self.db, self.persons, self.n_persons, poses, flags, joint_mask=mask)
        a, b = frames
        db = self.eng.to_device(self.scene.sub_batch(a, b))
        fit.accumulate(db, self.persons[a:b].contiguous(), self.n_persons[a:b].contiguous(), poses[a:b].contiguous(),
                       flags[a:b].contiguous(), joint_mask=mask)

    def statement(self, cams, kind='triang', huber_px=0.0, sums=None, frames=None):
        poses, flags, mask = self.host[kind]
        return fc.one_pass(self.scene, cams, sums=sums, frames=frames, poses=poses, flags=flags, mask=mask, huber_px=huber_px)


def setup(key, *a, **kw):
    if key not in _made:
        _made[key] = Setup(*a, **kw)
    return _made[key]


def teardown_module(module):
    for s in _made.values():
        for obj in s.made:
            obj.close()
        s.eng.close()
    _made.clear()


def assert_same_sums(got, want, what):
    for k in ('acc', 'n_obs', 'n_skipped'):
        if not fc.same_bits(got[k], want[k]):
            bad = np.argwhere(np.asarray(got[k]) != np.asarray(want[k]))
            print(what, k, 'differing', len(bad), 'first', bad[:3].tolist(), got[k][tuple(bad[0])], want[k][tuple(bad[0])])
        assert fc.same_bits(got[k], want[k]), (what, k)


def small(variant, pcap):
    """calib_cases.small with, in both kinds of poses, a joint behind a camera (frame 1: skipped and counted there) and one
    non-finite pose row (frame 2, person 1, joint 12 -- a used joint: skipped in every camera that selects it)."""
    s = cc.small(variant, pcap=pcap)
    c = min(2, s.pb.V - 1)
    P = s.E_true[c]
    behind = -P[:, :3].T @ P[:, 3] - P[2, :3]
    for kind, (poses, flags, mask) in s.kinds.items():
        poses[1, 1, 9] = behind
        poses[2, 1, 12] = np.nan
    return s


CASES = [('panoptic', kind, huber) for kind in ('est', 'triang') for huber in (0.0, 3.0)]
CASES.append(('arplab', 'triang', 3.0))
CASES.append(('arprobot', 'triang', 3.0))                    # six cameras configured, calibration indices 4 and 5 used
CASES.append(('ring23', 'triang', 3.0))                      # 23 cameras: 2415 chains, five per thread, seven pairs per tile


@pytest.mark.parametrize('variant,kind,huber', CASES)
def test_sums_bit_equal_to_host_statement(variant, kind, huber):
    """7: 3 frames of the rig x 2 persons (calib_cases.small: a person missing a camera, a joint absent, confidences at and
    below the threshold, flags off) with a joint behind a camera and a non-finite pose row, the trial set moved off in all
    thirteen unknowns, both kinds of poses, Huber 0 and 3 px, on the rigs test_gpu_calib.py takes and the 23-camera ring (the
    kernel with five chains per thread; the seven-chain one needs more than 24 cameras, which no fixture has): all 105 sums and both
    counts through mpe_camfit_read.  get_cameras returns what was set; the engine's calibration is untouched."""
    s = setup(('small', variant), variant, lambda pcap: small(variant, pcap), ppc=3 if variant == 'arprobot' else 2)
    assert s.scene.pb.V == {'arplab': 6, 'arprobot': 2, 'ring23': 23}.get(variant, 5) and s.eng.pcap > 2
    cams = fc.moved_set(s.scene, 21)
    fit = s.fitter(kind, huber_px=huber)
    fit.set_cameras(*cams)
    s.accumulate(fit, kind)
    got, want = fit.read(), s.statement(cams, kind, huber)
    print(variant, kind, huber, 'n_obs', want['n_obs'].tolist(), 'skipped', want['n_skipped'].tolist())
    assert_same_sums(got, want, (variant, kind, huber))
    assert want['n_obs'].min() > 20 and want['n_skipped'].sum() >= 2 and np.isfinite(want['acc']).all()
    acc, tri = fit.cameras()
    for a, t, w in zip(acc, tri, cams):
        assert fc.same_bits(a, w) and fc.same_bits(t, w)
    own = CF().start_cameras(s.scene.calib)
    fit.reset()
    for a, w in zip(fit.cameras()[0], own):
        assert fc.same_bits(a, w)
    if variant == 'arprobot':                                # the accepted set goes back to the rows of its own cameras
        fit.set_cameras(*cams)
        new, old = fit.calibration(), s.eng.calib
        idx = pkg('harness.reprojection').engine_cameras(old)
        assert idx == [4, 5] and fc.same_bits(np.asarray(new.P)[idx], cams[0]) and fc.same_bits(new.intrinsics()[idx], cams[1])
        assert fc.same_bits(np.asarray(new.dist)[idx], cams[2]) and fc.same_bits(new.K32[:4], old.K32[:4]) and fc.same_bits(new.dist[:4], old.dist[:4])


@pytest.mark.parametrize('kind,huber', [('triang', 0.0), ('est', 3.0)])
def test_pose_block_equals_mpe_calib_batch(kind, huber):
    """8: trial intrinsics the engine's, extrinsics moved: the 21 + 6 + 1 pose entries of the 105 sums are mpe_calib_batch's
    28 sums on the same batch, bit for bit, and the counts are equal."""
    s = setup(('small', 'panoptic'), 'panoptic', lambda pcap: small('panoptic', pcap))
    E, k, dist = fc.true_set(s.scene)
    E = cc.perturbed_start(E, 0.7, 15.0, 21)
    fit, cal = s.fitter(kind, huber_px=huber), s.calibrator(kind, huber_px=huber)
    fit.set_cameras(E, k, dist)
    cal.set_extrinsics(E)
    s.accumulate(fit, kind)
    s.accumulate(cal, kind)
    got, want = fit.read(), cal.read()
    assert fc.same_bits(got['acc'][:, CF().POSE_BLOCK], want['acc'])
    assert np.array_equal(got['n_obs'], want['n_obs']) and np.array_equal(got['n_skipped'], want['n_skipped']) and want['n_obs'].min() > 20


@pytest.mark.parametrize('variant,bodies', [('panoptic', [1, 2, 3, 5]), ('arplab', [1, 2, 4])])
def test_tiling_borders(variant, bodies):
    """9: a tile holds 180 // V (person, joint) pairs and a frame has 18 pairs per person, so pair counts move in steps of 18
    and "one pair below / above the tile" does not exist; the nearest frames there are are taken.  Five cameras: 36 pairs
    per tile -- one person (18, below), two (36, exactly the tile), three (54, above: the second tile holds one person)
    and five (90, beyond two tiles).  Six cameras: 30 pairs per tile, so the border falls inside a person -- one person
    (below), two (36: six pairs into the second tile) and four (72: three tiles).  One batch holds all the frames, with a
    joint behind a moved camera in a later tile; then each frame on its own.  Bits equal the host fold."""
    V = len(env(variant).params.used_cameras_skeleton_matching)
    tile = TILE_RECORDS // V
    pairs = [18 * b for b in bodies]
    assert min(pairs) < tile and max(pairs) > 2 * tile and (variant != 'panoptic' or tile in pairs) and any(tile < p <= 2 * tile for p in pairs)

    def maker(pcap):
        s = cc.Scene(variant, len(bodies), bodies, seed=4400, noise_px=1.0, pcap=pcap)
        P = s.E_true[2]
        s.truth[len(bodies) - 1, bodies[-1] - 1, 9] = -P[:, :3].T @ P[:, 3] - P[2, :3]
        return s
    s = setup(('tiles', variant), variant, maker, ppc=max(bodies))
    assert s.eng.pcap >= max(bodies)
    cams = fc.moved_set(s.scene, 33)
    for huber in (0.0, 3.0):
        fit = s.fitter(huber_px=huber)
        fit.set_cameras(*cams)
        s.accumulate(fit)
        want = s.statement(cams, huber_px=huber)
        assert_same_sums(fit.read(), want, ('tiles', variant, huber))
        assert want['n_skipped'][2] >= 1 and want['n_obs'].min() > 60
    for f in range(len(bodies)):                             # each shape on its own
        fit.set_cameras(*cams)
        s.accumulate(fit, frames=(f, f + 1))
        assert_same_sums(fit.read(), s.statement(cams, huber_px=3.0, frames=(f, f + 1)), ('frame', f))


def test_chunk_invariance_and_launch_count():
    """10: 7 frames as one call, as 3 + 4 and as seven calls give the same bits (the statement's, too); two launches per
    call whatever the frame count; a call of zero frames enqueues nothing and changes nothing."""
    s = setup('chunks', 'panoptic', lambda pcap: cc.Scene('panoptic', 7, 3, seed=4200, noise_px=1.5, pcap=pcap), ppc=3)
    cams = fc.moved_set(s.scene, 3)
    reads = []
    for cuts in ([(0, 7)], [(0, 3), (3, 7)], [(f, f + 1) for f in range(7)]):
        fit = s.fitter(huber_px=2.0)
        fit.set_cameras(*cams)
        n0 = fit.launches()
        for a, b in cuts:
            s.accumulate(fit, frames=None if (a, b) == (0, 7) else (a, b))
        assert fit.launches() - n0 == 2 * len(cuts)
        reads.append(fit.read())
    assert_same_sums(reads[0], reads[1], '3 + 4')
    assert_same_sums(reads[0], reads[2], 'seven calls')
    assert_same_sums(reads[0], s.statement(cams, huber_px=2.0), 'statement')
    poses, flags, mask = s.dev['triang']
    empty = s.eng.to_device(s.eng.pack([]))
    n1 = fit.launches()
    fit.accumulate(empty, s.persons[:0].contiguous(), s.n_persons[:0].contiguous(), poses[:0].contiguous(), flags[:0].contiguous())
    assert fit.launches() == n1
    assert_same_sums(fit.read(), reads[0], 'zero frames')


def test_loop_of_passes_against_the_host_step():
    """11: test_camfit_host's zero-residual loop through the device: 8 frames x 2 bodies, exact detections, the last camera
    0.5 degrees, 10 mm, +1 % focal, (+5, -5) px centre and (+0.02, -0.01, +0.005) lens terms off, all groups free.  The
    host statement runs beside the device from the same start; every pass's sums are bit-equal, and every step's report --
    status, passes, counts, costs, lambda, the four last_*, delta -- and the trial and accepted sets equal the host's bit
    for bit.  Both end CONVERGED in the same pass."""
    s = setup('loop', 'panoptic', lambda pcap: cc.Scene('panoptic', 8, 2, seed=4700, pcap=pcap))
    start = fc.moved_set(s.scene, 71, deg=0.5, mm=10.0, cameras=[s.scene.pb.V - 1])
    tols = (1e-9, 1e-9, 1e-3, 1e-7)
    fit = s.fitter()
    fit.set_cameras(*start)
    host = CF().HostCameraFitter(*start)
    for it in range(20):
        s.accumulate(fit)
        want = s.statement(host.trial())
        assert_same_sums(fit.read(), want, ('pass', it))
        rep, hrep = fit.step(*tols), CF().camfit_step_host(host, want, *tols)
        for k in ('status', 'passes', 'n_obs', 'n_skipped'):
            assert np.array_equal(rep[k], hrep[k]), (it, k, rep[k], hrep[k])
        for k in ('cost_start', 'cost', 'lambda', 'last_rot', 'last_trans', 'last_pix', 'last_lens', 'delta'):
            assert fc.same_bits(rep[k], hrep[k]), (it, k, rep[k], hrep[k])
        acc, tri = fit.cameras()
        for got, exp in zip(acc + tri, host.accepted() + host.trial()):
            assert fc.same_bits(got, exp), it
        assert rep['all_done'] == hrep['all_done']
        assert not fit.read()['n_obs'].any() and not fit.read()['acc'].any()          # zeroed by the step
        if rep['all_done']:
            break
    print('passes', it + 1, 'status', rep['status'].tolist(), 'cost', rep['cost'].tolist())
    assert rep['all_done'] and np.all(rep['status'] & CF().CONVERGED)
    truth = fc.true_set(s.scene)
    assert fc.same_bits(fit.cameras()[0][1], truth[1])       # fx, fy, cx, cy are the rig's float32 numbers again


def test_arguments_and_symbols():
    """12: NULL and zero arguments; a free_mask with unknown bits or none; a K with skew; min_obs below the free count; more
    frames than max_frames; passes that did not see the same data -- MPE_ERR_INVALID (capacity for the frames) and no
    crash; the new symbols resolve in the built library."""
    import torch
    L = pkg('lib')
    s = setup('chunks', 'panoptic', lambda pcap: cc.Scene('panoptic', 7, 3, seed=4200, noise_px=1.5, pcap=pcap), ppc=3)
    lib = C.CDLL(L.LIB_PATH)
    for sym in ('create', 'destroy', 'reset', 'set_cameras', 'get_cameras', 'batch', 'read', 'step', 'launches'):
        assert hasattr(lib, 'mpe_camfit_' + sym)
    eng, fit = s.eng, s.fitter()
    poses, flags, mask = s.dev['triang']
    # NULL pointers and a NULL state, with a live context
    null = C.c_void_p()
    assert eng.lib.mpe_camfit_create(eng.ctx, None) == -1 and eng.lib.mpe_camfit_destroy(eng.ctx, null) == -1
    assert eng.lib.mpe_camfit_reset(eng.ctx, None, null) == -1 and eng.lib.mpe_camfit_read(eng.ctx, None, null, None, None, None) == -1
    assert eng.lib.mpe_camfit_set_cameras(eng.ctx, None, fit.state, None, None, None) == -1
    assert eng.lib.mpe_camfit_get_cameras(eng.ctx, null, None, None, None, None, None, None) == -1
    assert eng.lib.mpe_camfit_get_cameras(eng.ctx, fit.state, None, None, None, None, None, None) == 0
    assert eng.lib.mpe_camfit_batch(eng.ctx, None, fit.state, C.byref(s.db.struct), None) == -1
    assert eng.lib.mpe_camfit_step(eng.ctx, None, fit.state, None, None) == -1 and eng.lib.mpe_camfit_launches(eng.ctx, fit.state, None) == -1

    def call(n_frames=7, n_joints=eng.J, huber=0.0):
        a = L.mpe_calib_args()
        a.n_frames, a.pcap, a.n_joints, a.pose_f64, a.joint_flags, a.joint_mask, a.threshold = n_frames, eng.pcap, n_joints, 1, 1, mask, 0.5
        a.huber_px = huber
        a.d_persons, a.d_n_persons, a.d_poses, a.d_flags = s.persons.data_ptr(), s.n_persons.data_ptr(), poses.data_ptr(), flags.data_ptr()
        eng._chk(eng.lib.mpe_camfit_batch(eng.ctx, eng._stream(), fit.state, C.byref(s.db.struct), C.byref(a)))

    for kw, word in (({'n_frames': 6}, 'frames'), ({'n_joints': 17}, 'joints'), ({'huber': float('nan')}, 'huber_px'), ({'huber': -1.0}, 'huber_px')):
        with pytest.raises(L.MpeError) as err:
            call(**kw)
        assert err.value.code == -1 and word in str(err.value), str(err.value)
    assert not fit.read()['n_obs'].any()

    def step(free_mask=63, min_obs=13):
        a, rep = L.mpe_camfit_step_args(), L.mpe_camfit_report()
        a.rot_tol, a.trans_tol, a.pix_tol, a.lens_tol, a.min_obs, a.hold_mask, a.free_mask = 1e-7, 1e-6, 1e-3, 1e-7, min_obs, 0, free_mask
        eng._chk(eng.lib.mpe_camfit_step(eng.ctx, eng._stream(), fit.state, C.byref(a), C.byref(rep)))
        return rep

    for kw, word in (({'free_mask': 64}, 'free_mask'), ({'free_mask': 0}, 'free_mask'), ({'free_mask': 63 | 128}, 'free_mask'),
                     ({'min_obs': 12}, 'min_obs'), ({'free_mask': 1, 'min_obs': 5}, 'min_obs'), ({'free_mask': 2 | 4, 'min_obs': 5}, 'min_obs')):
        with pytest.raises(L.MpeError) as err:
            step(**kw)
        assert err.value.code == -1 and word in str(err.value), str(err.value)
    step(free_mask=2 | 4, min_obs=6)                         # four free unknowns: 6 is enough
    fit.reset()
    # a pass that does not see the first pass's data
    call()
    rep = fit.step()
    assert rep['n_obs'].min() > 0 and np.all(rep['status'] & L.MPE_CALIB_ACCEPTED)
    s.accumulate(fit, frames=(0, 5))
    with pytest.raises(L.MpeError) as err:
        fit.step()
    assert err.value.code == -1 and 'same data' in str(err.value)
    # set_cameras: a value that is not finite, a focal length that is not positive, shapes
    E, k, dist = fc.true_set(s.scene)
    for bad in ((E * np.nan, k, dist), (E, -k, dist), (E, k, dist + np.inf)):
        with pytest.raises(L.MpeError) as err:
            fit.set_cameras(*bad)
        assert err.value.code == -1
    with pytest.raises(ValueError):
        fit.set_cameras(E[:2], k, dist)
    for kw in ({'kind': 'gt'}, {'free': ('focal', 'skew')}, {'free': ()}, {'hold': (99,)}, {'hold': ('no such camera',)}, {'huber_px': -1.0}):
        with pytest.raises(ValueError):
            eng.camera_fitter(**dict({'kind': 'triang'}, **kw))
    held = s.fitter(hold=(s.scene.names[0],), free='focal,centre')
    s.accumulate(held)
    rep = held.step()
    assert rep['status'][0] == L.MPE_CALIB_HELD and not (rep['status'][1:] & L.MPE_CALIB_HELD).any()
    assert not rep['delta'][:, :6].any() and not rep['delta'][:, 10:].any() and rep['delta'][1:, 6:10].all()
    # more frames than the engine's max_frames: refused before anything runs
    e = env()
    tiny = pkg('pipeline').Engine(e.params, e.calib, max_frames=4, max_persons_per_camera=3)
    try:
        f4 = tiny.camera_fitter('triang')
        with pytest.raises((L.MpeError, ValueError)):
            f4.accumulate(s.db, s.persons, s.n_persons, poses, flags, joint_mask=mask)
        f4.close()
    finally:
        tiny.close()
    # a K with skew: the state is refused at create
    skew = pkg('calibration').Calibration(e.params, e.calib.tm)
    skew.K32[0, 0, 1] = 0.5
    eng2 = pkg('pipeline').Engine(e.params, skew, max_frames=4, max_persons_per_camera=3)
    try:
        with pytest.raises(L.MpeError) as err:
            eng2.camera_fitter('triang')
        assert err.value.code == -1 and 'K of camera' in str(err.value)
        eng2.calibrator('triang').close()                    # the calibrator does not mind
    finally:
        eng2.close()
    fit.close()
    with pytest.raises(RuntimeError):
        fit.read()
    torch.cuda.synchronize()


def test_script_on_synthetic_frames(tmp_path, capsys):
    """13: the script on 32 generated frames with the last camera's focal length 1 % and its centre (+5, -5) px off,
    geometric matching, 3 rounds of up to 8 passes, focal and centre free: for that camera the RMS reprojection error falls
    and so do its focal and centre errors against the generator's truth (directions only).  What the held and the other
    free cameras do is printed, not asserted.  --out reads back through load_transform_manager and load_intrinsics, and
    an Engine built from it carries the fitted intrinsics."""
    cal = pkg('calibration')
    out = str(tmp_path / 'cams.json')
    rep = CF().main(['--synthetic', '32', '--matcher', 'geometric', '--perturb-focal', '1', '--perturb-centre', '5', '--free', 'focal,centre',
                     '--rounds', '3', '--passes', '8', '--out', out])
    text = capsys.readouterr().out
    print(text)
    c = len(rep['cameras']) - 1                              # the changed camera: the last
    before, after = rep['true_before'], rep['true_after']
    assert before[c][2] > 0.99 and before[c][3] > 7.0 and all(before[k][2] == 0.0 and before[k][3] == 0.0 for k in range(c))
    assert rep['rms_after'][c] < rep['rms_before'][c]
    assert after[c][2] < before[c][2] and after[c][3] < before[c][3]
    for k in range(c):
        print('camera', rep['cameras'][k], 'held' if rep['cameras'][k] in rep['hold'] else 'free', 'focal error %', after[k][2], 'centre error px',
              after[k][3], 'RMS', rep['rms_before'][k], '->', rep['rms_after'][k])
    assert rep['hold'] == [rep['cameras'][0]] and after[0][2] == 0.0 and after[0][3] == 0.0
    assert sum(ln.startswith('camera ') for ln in text.splitlines()) >= len(rep['cameras']) and 'gauge:' in text and os.path.exists(out)
    p = env().params
    back = cal.Calibration(p, cal.load_transform_manager(out), cal.load_intrinsics(out, p))
    for name in ('P', 'K32', 'Kinv32', 'dist'):
        assert fc.same_bits(getattr(back, name), getattr(rep['calibration'], name)), name
    eng = pkg('pipeline').Engine(p, back, max_frames=4, max_persons_per_camera=3)
    try:
        fit = eng.camera_fitter('triang')
        assert fc.same_bits(fit.cameras()[0][1], back.intrinsics()[pkg('harness.reprojection').engine_cameras(back)])
        fit.close()
    finally:
        eng.close()
