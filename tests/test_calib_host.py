"""CPU: harness/calibrate.py, the numpy statement of mpe_calib_batch / mpe_calib_step, and csrc/calib_solve.h -- that the
Jacobian is the derivative of the projection, that the solver solves (a stand-alone program under sanitizers, and the
numpy step bit for bit beside it), that the passes find the minimum (scipy's Levenberg-Marquardt as the yardstick), what a
rejected pass leaves alone, the small exact cases and chunk invariance."""
import os
import re
import shutil
import subprocess

import numpy as np
import pytest

import calib_cases as cc
from conftest import ROOT, env, pkg

_made = {}


def CB():
    return pkg('harness.calibrate')


def ring():
    """The ring rig (23 cameras), 32 frames x 4 bodies, detections exact."""
    if 'ring' not in _made:
        _made['ring'] = cc.Scene('ring23', 32, 4)
    return _made['ring']


def rig5(n_frames=16, n_bodies=3):
    key = ('rig5', n_frames, n_bodies)
    if key not in _made:
        _made[key] = cc.Scene('panoptic', n_frames, n_bodies, seed=4200)
    return _made[key]


def test_jacobian_is_the_derivative_of_the_projection():
    """1: Jx / Jy against central differences of the statement's own projection under exp(h e_k) / tau = h e_k, h = 1e-6,
    on 200 observations (5 cameras x 40 joints, extrinsics moved off the rig's): within 1e-6 of the row's largest entry
    (roundoff ~ eps |px| / h ~ 4e-7 on entries of a few hundred and more)."""
    s = rig5()
    _, kd, K = pkg('harness.refine').camera_constants64(s.calib)
    E = cc.perturbed_start(s.E_true, 2.0, 50.0, 77)
    X = s.truth[0, :3].reshape(-1, 3)[:40]
    h, n, worst = 1e-6, 0, 0.0
    for c in range(5):
        p = CB().project_camera(E[c], kd[c], K[c], X[:, 0], X[:, 1], X[:, 2], jacobian=True)
        assert np.all(p['pc'][2] > 0)
        rows = {'px': np.stack(p['Jx'], axis=1), 'py': np.stack(p['Jy'], axis=1)}
        num = {'px': np.zeros((len(X), 6)), 'py': np.zeros((len(X), 6))}
        for k in range(6):
            xi = np.zeros(6)
            xi[k] = h
            hi = CB().project_camera(CB().compose(E[c], xi), kd[c], K[c], X[:, 0], X[:, 1], X[:, 2])
            lo = CB().project_camera(CB().compose(E[c], -xi), kd[c], K[c], X[:, 0], X[:, 1], X[:, 2])
            for key in num:
                num[key][:, k] = (hi[key] - lo[key]) / (2 * h)
        for key in rows:
            scale = np.abs(rows[key]).max(axis=1, keepdims=True)
            rel = np.abs(rows[key] - num[key]) / scale
            worst = max(worst, float(rel.max()))
            n += len(X)
            assert scale.min() > 100 and rel.max() < 1e-6, (c, key, rel.max())
    print('observations', n // 2, 'worst relative difference', worst)
    assert n // 2 == 200


def test_solver_header_under_sanitizers_and_the_numpy_step_beside_it(tmp_path):
    """2: tests/native/calib_solve_test.cpp built with -fsanitize=address,undefined and run as a child process: its own
    checks (LDL^T on known systems, the pivot that is not > 0, the retry cap, Rodrigues at |w| = 0, 1e-12, 1e-3, 3,
    orthonormality), then the seeded systems of calib_cases: the numpy step gives the same delta and lambda bit for bit,
    E_t within 1e-14 (a few ulp of libm's sin / cos on entries <= 10)."""
    gxx = shutil.which('g++')
    if not gxx:
        pytest.skip('g++ not available')
    exe = str(tmp_path / 'calib_solve_test')
    subprocess.run([gxx, '-O1', '-g', '-Wall', '-Werror', '-ffp-contract=off', '-fsanitize=address,undefined', '-fno-sanitize-recover=all',
                    '-I', os.path.join(ROOT, '3d_multi_pose_estimator_amd', 'csrc'), os.path.join(ROOT, 'tests', 'native', 'calib_solve_test.cpp'),
                    '-o', exe], check=True, capture_output=True, timeout=300)
    systems = cc.systems()
    path = tmp_path / 'systems.txt'
    with open(path, 'w') as fh:
        for A, g, lam, Ea in systems:
            fh.write(' '.join(float(x).hex() for x in list(A) + list(g) + [lam] + list(Ea)) + '\n')
    r = subprocess.run([exe, str(path)], capture_output=True, text=True, timeout=120)
    assert r.returncode == 0, r.stdout + r.stderr
    m = re.search(r'tested (\d+) bad (\d+)', r.stdout)
    assert m and int(m.group(1)) > 400 and int(m.group(2)) == 0, r.stdout
    lines = [ln.split() for ln in r.stdout.splitlines() if ln.startswith('sys ')]
    assert len(lines) == len(systems)
    n_stalled = n_retried = 0
    for ln, (A, g, lam, Ea) in zip(lines, systems):
        stalled, lam_c = int(ln[2]), float.fromhex(ln[3])
        delta_c = [float.fromhex(x) for x in ln[4:10]]
        Et_c = np.array([float.fromhex(x) for x in ln[10:22]])
        delta, lam_h, Et, st = cc.host_trial(A, g, lam, Ea)
        assert st == bool(stalled) and lam_h == lam_c, (ln[1], st, stalled, lam_h, lam_c)
        n_stalled += st
        n_retried += lam_h != lam
        if not st:
            assert [x.hex() for x in delta] == [x.hex() for x in delta_c], ln[1]
            assert np.abs(Et).max() <= 10 and np.abs(Et - Et_c).max() <= 1e-14, (ln[1], np.abs(Et - Et_c).max())
        else:
            assert np.array_equal(Et, Ea) and np.array_equal(Et_c, Ea)
    print('systems', len(systems), 'stalled', n_stalled, 'retried', n_retried)
    assert n_stalled >= 1 and n_retried > n_stalled


def _distances(E, truth):
    d = [CB().extrinsics_distance(E[c], truth[c]) for c in range(len(E))]
    return max(x[0] for x in d), max(x[1] for x in d)


def test_known_answer_zero_residual_against_scipy():
    """3: ring rig, 32 frames x 4 bodies, detections exact; every camera starts 1 degree and 20 mm off.  Passes until every
    camera is CONVERGED (cap 30; tolerances 1e-9 rad / 1e-9 m).  Our distance to the truth <= 10 x max(scipy's, 1e-12) in
    rotation angle and in translation norm, scipy.optimize.least_squares(method='lm', ftol = xtol = gtol = 1e-15) per
    camera on the same residuals from the same start.
    Measured: 6 passes; ours 1.3e-14 rad / 1.3e-14 m, scipy 1.2e-16 rad / 4.6e-16 m (worst camera each)."""
    s = ring()
    E0 = cc.perturbed_start(s.E_true, 1.0, 20.0, 900)
    state, reports = cc.run_host(s, E0, 30, 1e-9, 1e-9)
    last = reports[-1]
    assert last['all_done'] and np.all(last['status'] & CB().CONVERGED), last['status']
    ours = _distances(state.accepted(), s.E_true)
    fits = [cc.scipy_fit(s, c, E0[c])[0] for c in range(s.pb.V)]
    theirs = _distances(fits, s.E_true)
    print('passes', len(reports), 'ours rad / m', ours, 'scipy rad / m', theirs)
    assert ours[0] <= 10 * max(theirs[0], 1e-12) and ours[1] <= 10 * max(theirs[1], 1e-12)
    assert np.array_equal(state.accepted(), state.trial())


def test_noisy_cost_against_scipy_and_costs_never_rise():
    """4: the same scene with 2 px of seeded noise, both solvers asked for 1e-12 steps: our final cost per camera <=
    scipy's x (1 + 1e-6) (the cost is flat to second order at the minimum), and the accepted costs never increase.
    Measured over 30 passes: ours / scipy between 1 - 3.0e-13 and 1 - 3.1e-15 over the 23 cameras."""
    s = ring()
    noisy = cc.copy.copy(s)
    noisy.pb = s.with_detections(2.0, 31)
    E0 = cc.perturbed_start(s.E_true, 1.0, 20.0, 900)
    state, reports = cc.run_host(noisy, E0, 30, 1e-12, 1e-12)
    costs = np.stack([r['cost'] for r in reports])
    assert np.all(np.diff(costs, axis=0) <= 0)
    theirs = np.array([cc.scipy_fit(noisy, c, E0[c])[1] for c in range(s.pb.V)])
    ratio = costs[-1] / theirs
    print('passes', len(reports), 'cost ratio ours / scipy: max', ratio.max(), 'min', ratio.min(), 'cost per observation', (costs[-1] / reports[-1]['n_obs']).mean())
    assert np.all(costs[-1] <= theirs * (1 + 1e-6))
    assert np.all(costs[-1] < 0.1 * costs[0])             # the noise floor, 2 x 2^2 px^2 per observation, against a start 20 x above it


REJECTED_START = (25.0, 600.0, 5)       # degrees, millimetres, seed: found by the search the docstring below describes


def test_rejected_pass_grows_lambda_and_leaves_the_accepted_state():
    """5: a start at which the statement's first trial is rejected at least once (searched on the CPU over 10 / 25 / 40 degrees with
    300 / 600 / 1000 mm and seeds 0..19 for the first start with a rejection in pass 2 whose passes all see the same
    observations, then pinned: 25 degrees, 600 mm, seed 5, camera 0): lambda grows by ten, the accepted
    extrinsics, sums and cost are those of before, and the run still ends below the start cost."""
    s = rig5(8, 3)
    deg, mm, seed = REJECTED_START
    E0 = cc.perturbed_start(s.E_true, deg, mm, seed)
    state = CB().HostCalibrator(E0)
    rep = CB().calib_step_host(state, s.one_pass(state.trial()), 1e-9, 1e-9)
    assert np.all(rep['status'] & CB().ACCEPTED)
    before = [(c.Ea.copy(), c.Aa.copy(), c.lam) for c in state.cams]
    rep2 = CB().calib_step_host(state, s.one_pass(state.trial()), 1e-9, 1e-9)
    rejected = np.flatnonzero(rep2['status'] & CB().REJECTED)
    print('rejected cameras', rejected.tolist(), 'lambda', rep2['lambda'].tolist())
    assert len(rejected) >= 1
    for c in rejected:
        Ea, Aa, lam = before[c]
        cam = state.cams[c]
        assert cam.lam == lam * 10.0 and np.array_equal(cam.Ea, Ea) and np.array_equal(cam.Aa, Aa)
        assert rep2['cost'][c] == rep['cost'][c] and not np.array_equal(cam.Et, Ea)
    for _ in range(28):
        last = CB().calib_step_host(state, s.one_pass(state.trial()), 1e-9, 1e-9)
    assert np.all(last['cost'] < last['cost_start'])


def test_small_exact_cases():
    """6: a HELD camera, FEW_OBS, a joint behind the trial camera, Huber on a hand-made outlier, n_obs that changes."""
    s = rig5(8, 3)
    E0 = cc.perturbed_start(s.E_true, 0.5, 10.0, 12)
    # HELD: sums and cost reported, the trial never moves
    state, reports = cc.run_host(s, E0, 3, 1e-9, 1e-9, hold=(1,), until_done=False)
    for r in reports:
        assert r['status'][1] == CB().HELD and r['cost'][1] == reports[0]['cost'][1] > 0
    assert np.array_equal(state.trial()[1], E0[1]) and not np.array_equal(state.trial()[0], E0[0])
    # FEW_OBS: min_obs one above the observations of the camera that has the fewest
    n = reports[0]['n_obs']
    few = int(np.argmin(n))
    state, reports = cc.run_host(s, E0, 2, 1e-9, 1e-9, min_obs=int(n[few]) + 1, until_done=False)
    held = reports[-1]['status'] & CB().HELD != 0
    assert held[few] and reports[-1]['status'][few] & CB().FEW_OBS and np.array_equal(held, n <= n[few])
    assert np.array_equal(state.trial()[few], E0[few])
    with pytest.raises(ValueError):
        CB().HostCalibrator(E0, min_obs=5)
    # a joint behind camera 2: skipped and counted there, and the sums are those of the pass without it
    behind = s.truth.copy()
    P = s.E_true[2]
    behind[0, 1, 8] = -P[:, :3].T @ P[:, 3] - P[2, :3]
    base = s.one_pass(s.E_true)
    got = s.one_pass(s.E_true, poses=behind)
    off = s.flags.copy()
    off[0, 1, 8] = 0
    assert got['n_skipped'][2] == 1 and got['n_obs'][2] == base['n_obs'][2] - 1 and base['n_skipped'].sum() == 0
    assert cc.same_bits(got['acc'][2], s.one_pass(s.E_true, poses=behind, flags=off)['acc'][2])
    nan = s.truth.copy()
    nan[0, 1, 8, 1] = np.nan
    got = s.one_pass(s.E_true, poses=nan)
    assert np.all(got['n_skipped'] == 1) and np.isfinite(got['acc']).all()
    # Huber: one detection 100 px off; its rho is 2 h e - h^2 and its weight h / e
    pb = cc.copy.copy(s.pb)
    pb.xy = np.array(s.pb.xy, np.float64, copy=True).reshape(-1, cc.J, 2)
    head = int(s.pb.frame_head_off[0]) + int(s.persons[0, 0, 0])
    pb.xy[head, 3, 0] += 100.0
    pb.xy = pb.xy.reshape(np.asarray(s.pb.xy).shape)
    plain, hub = s.one_pass(s.E_true, pb=pb), s.one_pass(s.E_true, pb=pb, huber_px=5.0)
    e = 100.0
    assert abs(plain['acc'][0, 27] - e * e) < 1e-6 and abs(hub['acc'][0, 27] - (2 * 5.0 * e - 25.0)) < 1e-6
    assert np.allclose(hub['acc'][0, 21:27], plain['acc'][0, 21:27] * (5.0 / e), rtol=1e-6, atol=0)
    assert cc.same_bits(plain['acc'][1:], hub['acc'][1:])
    with pytest.raises(ValueError):
        s.one_pass(s.E_true, huber_px=float('nan'))
    # n_obs that changes between passes
    state = CB().HostCalibrator(E0)
    CB().calib_step_host(state, s.one_pass(state.trial()), 1e-9, 1e-9)
    kept = [c.Et.copy() for c in state.cams]
    with pytest.raises(ValueError, match='did not see the same data'):
        CB().calib_step_host(state, s.one_pass(state.trial(), flags=off), 1e-9, 1e-9)
    assert all(np.array_equal(c.Et, k) and c.passes == 1 for c, k in zip(state.cams, kept))


def test_chunk_invariance():
    """7: 16 frames in one call and as three calls of 5 + 10 + 1 give the same bits, for both Huber settings."""
    s = rig5(16, 3)
    noisy = cc.copy.copy(s)
    noisy.pb = s.with_detections(1.5, 8)
    E = cc.perturbed_start(s.E_true, 0.3, 5.0, 3)
    for huber in (0.0, 2.0):
        whole = noisy.one_pass(E, huber_px=huber)
        parts = None
        for a, b in ((0, 5), (5, 15), (15, 16)):
            parts = noisy.one_pass(E, sums=parts, frames=(a, b), huber_px=huber)
        assert cc.same_bits(whole['acc'], parts['acc']) and np.array_equal(whole['n_obs'], parts['n_obs'])
        assert whole['n_obs'].sum() > 3000 and np.array_equal(whole['n_skipped'], parts['n_skipped'])


def test_with_extrinsics_and_declarations(tmp_path):
    """Calibration.with_extrinsics rebuilds every derived array and leaves the original alone; the transform file the script
    writes reads back to the same bits; lib.py declares the entry points and the structs follow include/mpe.h."""
    calib = env().calib
    E = cc.perturbed_start(np.asarray(calib.P), 1.0, 20.0, 5)
    before = np.array(calib.P, copy=True)
    new = calib.with_extrinsics(E)
    assert np.array_equal(calib.P, before) and new is not calib
    assert np.array_equal(new.P, E) and np.array_equal(new.T_d[:, :3], E) and np.all(new.T_d[:, 3] == [0, 0, 0, 1])
    for i in range(calib.n_cameras):
        assert np.array_equal(new.T_i[i], np.linalg.inv(new.T_d[i])) and np.array_equal(new.T_i32[i], new.T_i[i].astype(np.float32))
        assert np.allclose(new.centre32[i, :3], -E[i][:, :3].T @ E[i][:, 3], atol=1e-5)
    assert np.array_equal(new.K32, calib.K32) and np.array_equal(new.dist, calib.dist) and np.array_equal(new.Kinv32, calib.Kinv32)
    with pytest.raises(ValueError):
        calib.with_extrinsics(E[:2])
    path = str(tmp_path / 'tm_out.json')
    with open(path, 'w') as fh:
        cc.json.dump(CB().transform_manager_json(new), fh)
    back = pkg('calibration').Calibration(calib.params, pkg('calibration').load_transform_manager(path))
    assert cc.same_bits(back.P, new.P) and cc.same_bits(back.T_i, new.T_i)
    L = pkg('lib')
    with open(os.path.join(ROOT, 'include', 'mpe.h')) as fh:
        header = fh.read()
    for sym in ('create', 'destroy', 'reset', 'set_extrinsics', 'get_extrinsics', 'batch', 'read', 'step', 'launches'):
        assert 'mpe_calib_' + sym in L.SYMBOLS and 'int mpe_calib_%s(' % sym in header
    for name, struct in (('mpe_calib_args', L.mpe_calib_args), ('mpe_calib_step_args', L.mpe_calib_step_args),
                         ('mpe_calib_cam_report', L.mpe_calib_cam_report)):
        body = re.search(r'typedef struct \{([^}]*)\} %s;' % name, header).group(1)
        body = re.sub(r'/\*.*?\*/', '', body, flags=re.S)
        fields = [re.sub(r'\[\d+\]', '', f).strip().lstrip('*') for decl in body.split(';') if decl.strip() for f in re.sub(
            r'\b(const|int32_t|uint32_t|int64_t|uint8_t|double|float|void)\b', '', decl).split(',')]
        assert fields == [f.rstrip('_') for f, _ in struct._fields_], (name, fields)
    args = CB().build_own_parser().parse_args(['--synthetic', '4', '--rounds', '2', '--passes', '3', '--hold'])
    assert args.rounds == 2 and args.passes == 3 and args.hold == [] and args.calib_huber == 0.0
