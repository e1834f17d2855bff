"""CPU: harness/camfit.py, the numpy statement of mpe_camfit_batch / mpe_camfit_step, and csrc/camfit_solve.h -- that the
thirteen Jacobian columns are the derivatives of the projection, that with only the pose free the statement is
harness/calibrate.py bit for bit, that the passes find the minimum (scipy's Levenberg-Marquardt as the yardstick), that
the reduced solve solves, and a stand-alone program under sanitizers that holds the header to the statement."""
import os
import re
import shutil
import subprocess

import numpy as np
import pytest

import camfit_cases as fc
from conftest import ROOT, env, pkg

_made = {}
POSE_TOLS = (1e-9, 1e-9, 1e-3, 1e-7)            # rot, trans (as test_calib_host's), pix, lens (the defaults)


def CF():
    return pkg('harness.camfit')


def CB():
    return pkg('harness.calibrate')


def zero_scene():
    """Test 3's scene: 8 frames x 2 bodies, exact detections."""
    if 'zero' not in _made:
        _made['zero'] = fc.Scene('panoptic', 8, 2, seed=4700)
    return _made['zero']


def zero_start(s):
    """... and its start: the last camera 0.5 degrees and 10 mm off, focal +1 %, centre (+5, -5) px, kd (+0.02, -0.01, +0.005)."""
    return fc.moved_set(s, 71, deg=0.5, mm=10.0, cameras=[s.pb.V - 1])


def zero_run(log=None):
    key = 'zero_run'
    if key not in _made or log is not None:
        s = zero_scene()
        _made[key] = fc.run_host(s, zero_start(s), 20, POSE_TOLS, log=log)
    return _made[key]


@pytest.mark.parametrize('variant', ['panoptic', 'arplab'])
def test_jacobian_is_the_derivative_of_the_projection(variant):
    """1: all thirteen columns against central differences of the statement's projection, 200 seeded points per rig spread
    over its cameras, the set moved off the rig's (so that the lens terms are not zero on ARPLAB).  Steps: 1e-6 on the
    pose, 1e-3 px on fx fy cx cy, 1e-2 on the lens terms; within 1e-6 of the row's largest entry for the pose columns
    (as test_calib_host), and within 1e-7 relative (+ 1e-9 absolute) for the seven new columns: the projection is linear
    in each of these unknowns, so the central difference is exact up to its roundoff eps |px| / h <= 2e-13 / 1e-3."""
    s = fc.Scene(variant, 4, 3, seed=4800)
    E, k, dist = fc.moved_set(s, 5, deg=2.0, mm=50.0)
    V = s.pb.V
    rng = np.random.default_rng(9)
    X = s.truth[:, :3].reshape(-1, 3)
    X = X[rng.choice(len(X), 200, replace=False)]
    steps = [1e-6] * 6 + [1e-3] * 4 + [1e-2] * 3
    n, worst_pose, worst_new = 0, 0.0, 0.0
    for c in range(V):
        pts = X[c::V]
        p = CF().project_camera(E[c], k[c], dist[c], pts[:, 0], pts[:, 1], pts[:, 2], jacobian=True)
        assert np.all(p['pc'][2] > 0) and len(p['Jx']) == 13 and len(p['Jy']) == 13
        rows = {'px': np.stack(p['Jx'], axis=1), 'py': np.stack(p['Jy'], axis=1)}
        num = {'px': np.zeros((len(pts), 13)), 'py': np.zeros((len(pts), 13))}
        for u in range(13):
            ends = []
            for sign in (1.0, -1.0):
                x = np.zeros(13)
                x[u] = sign * steps[u]
                Eu = CB().compose(E[c], x[:6]) if u < 6 else E[c]
                ku = k[c].astype(np.float64) + x[6:10]
                du = dist[c].copy()
                du[fc.KD] = du[fc.KD] + x[10:13]
                K = np.array([[ku[0], 0.0, ku[2]], [0.0, ku[1], ku[3]], [0.0, 0.0, 1.0]])
                ends.append(CB().project_camera(Eu, du[fc.KD], K, pts[:, 0], pts[:, 1], pts[:, 2]))
            for key in num:
                num[key][:, u] = (ends[0][key] - ends[1][key]) / (2 * steps[u])
        for key in rows:
            scale = np.abs(rows[key][:, :6]).max(axis=1, keepdims=True)
            rel = np.abs(rows[key][:, :6] - num[key][:, :6]) / scale
            worst_pose = max(worst_pose, float(rel.max()))
            assert rel.max() < 1e-6, (c, key, rel.max())
            err = np.abs(rows[key][:, 6:] - num[key][:, 6:]) / (np.abs(rows[key][:, 6:]) + 1e-2)
            worst_new = max(worst_new, float(err.max()))
            assert np.all(np.abs(rows[key][:, 6:] - num[key][:, 6:]) <= 1e-7 * np.abs(rows[key][:, 6:]) + 1e-9), (c, key, err.max())
        n += len(pts)
    print(variant, 'points', n, 'worst pose column', worst_pose, 'worst new column', worst_new)
    assert n == 200


def test_pose_only_is_the_calibrator_bit_for_bit():
    """2: free = POSE, trial intrinsics the rig's: the pose block of camfit_pass_host (21 + 6 + 1 of the 105) is
    calib_pass_host's bit for bit, at the rig's extrinsics and at a moved set, with and without Huber; three steps give
    calib_step_host's deltas, lambdas, statuses and trial extrinsics bit for bit."""
    import calib_cases as cc
    s = fc.Scene('panoptic', 8, 2, seed=4600, noise_px=1.0)
    E0, k, dist = fc.true_set(s)
    block = CF().POSE_BLOCK
    assert len(block) == 28 and len(set(block)) == 28
    moved = cc.perturbed_start(E0, 0.8, 15.0, 44)
    for E in (E0, moved):
        for huber in (0.0, 3.0):
            got, want = fc.one_pass(s, (E, k, dist), huber_px=huber), s.one_pass(E, huber_px=huber)
            assert fc.same_bits(got['acc'][:, block], want['acc']), huber
            assert np.array_equal(got['n_obs'], want['n_obs']) and np.array_equal(got['n_skipped'], want['n_skipped'])
    ours = CF().HostCameraFitter(moved, k, dist, free=CF().POSE, min_obs=6)
    theirs = CB().HostCalibrator(moved)
    for it in range(3):
        Et = ours.trial()[0]
        assert fc.same_bits(Et, theirs.trial()), it
        rep = CF().camfit_step_host(ours, fc.one_pass(s, ours.trial()), 1e-12, 1e-12)
        ref = CB().calib_step_host(theirs, s.one_pass(Et), 1e-12, 1e-12)
        for key in ('status', 'passes', 'n_obs', 'cost_start', 'cost', 'lambda', 'last_rot', 'last_trans'):
            assert fc.same_bits(rep[key], ref[key]), (it, key)
        assert fc.same_bits(rep['delta'][:, :6], ref['delta']) and not rep['delta'][:, 6:].any()
        assert fc.same_bits(ours.trial()[0], theirs.trial()) and fc.same_bits(ours.accepted()[0], theirs.accepted())
        assert fc.same_bits(ours.trial()[1], k) and fc.same_bits(ours.trial()[2], dist)
    assert np.all(rep['cost'] < rep['cost_start'])


def test_zero_residual_convergence_against_scipy():
    """3: 8 frames x 2 bodies, detections exact (made with the rig's own K32: the truth is representable); the last camera
    starts 0.5 degrees and 10 mm off, focal +1 %, centre (+5, -5) px, kd (+0.02, -0.01, +0.005); all groups free, no
    camera held.  Every camera ends CONVERGED within 20 passes.  Distance to the truth, per unknown group, against
    scipy.optimize.least_squares(method='lm') on the same residuals from the same start: ours <= max(10 x scipy's, the
    floor), the floor one float32 spacing for fx, fy, cx, cy and 1e-12 (test_calib_host's floor under scipy) for the rest.
    Measured: see the printed line; DESIGN.md 7.17 quotes it."""
    s = zero_scene()
    c = s.pb.V - 1
    start = zero_start(s)
    state, reports = zero_run()
    last = reports[-1]
    print('passes', len(reports), 'status', last['status'].tolist(), 'cost', last['cost'].tolist())
    assert len(reports) <= 20 and last['all_done'] and np.all(last['status'] & CF().CONVERGED), last['status']
    truth = fc.true_set(s)
    ours = fc.camera_distance(state.accepted(), truth, c)
    (E, kk, dd), cost = fc.scipy_fit(s, c, start)
    fit = (np.repeat(E[None], s.pb.V, 0), np.repeat(kk[None], s.pb.V, 0), np.repeat(dd[None], s.pb.V, 0))
    truth64 = (truth[0], truth[1].astype(np.float64), truth[2])
    theirs = fc.camera_distance(fit, truth64, c)
    print('ours', ours, 'scipy', theirs, 'scipy cost', cost)
    for i, name in enumerate(('fx', 'fy', 'cx', 'cy')):
        assert ours[name] <= max(10 * theirs[name], float(np.spacing(truth[1][c][i]))), name
    for name in ('rot', 'trans', 'kd0', 'kd1', 'kd2'):
        assert ours[name] <= max(10 * theirs[name], 1e-12), name
    for other in range(c):                                   # the cameras that started at the truth stayed there
        assert fc.same_bits(state.accepted()[1][other], truth[1][other]) and last['cost'][other] == 0.0


def test_noisy_cost_against_scipy():
    """4: 32 frames x 4 bodies, 1 px of seeded noise, every camera moved off in all thirteen unknowns, up to 30 passes.  The
    final cost per camera against scipy's: ours <= scipy's + sum |A_kl| d_k d_l over the four K entries, d = half a
    float32 spacing of each, + 1e-9 x scipy's.  The reason: the cost is flat to second order at the minimum; our fx, fy,
    cx, cy live on the float32 grid, at most d from the continuous minimiser, and with the other unknowns held there the
    cost rises by at most that quadratic form -- refitting them can only lower it; 1e-9 covers both solvers' stopping.
    Measured: see the printed line; DESIGN.md 7.17 quotes it."""
    s = fc.Scene('panoptic', 32, 4, seed=4900, noise_px=1.0)
    start = fc.moved_set(s, 17, deg=0.5, mm=10.0)
    state, reports = fc.run_host(s, start, 30, POSE_TOLS)
    costs = np.stack([r['cost'] for r in reports])
    assert np.all(np.diff(costs, axis=0) <= 0)
    ratios, margins = [], []
    for c in range(s.pb.V):
        _, theirs = fc.scipy_fit(s, c, start)
        A = state.cams[c].Aa
        d = [0.5 * float(np.spacing(state.cams[c].a.k[i])) for i in range(4)]
        margin = sum(abs(float(A[CF().TRI.index((min(6 + a, 6 + b), max(6 + a, 6 + b)))])) * d[a] * d[b] for a in range(4) for b in range(4))
        ratios.append(costs[-1][c] / theirs - 1.0)
        margins.append(margin / theirs)
        assert costs[-1][c] <= theirs + margin + 1e-9 * theirs, (c, costs[-1][c], theirs, margin)
    print('passes', len(reports), 'ours / scipy - 1 per camera', ratios, 'rounding margin / scipy per camera', margins,
          'status', reports[-1]['status'].tolist())
    assert np.all(costs[-1] < 0.1 * costs[0])


def test_solve_with_held_groups():
    """5: the reduced solve equals numpy's dense solve of the reduced system to 1e-12 relative on 200 seeded SPD systems,
    for several masks; a held unknown's delta is 0; a pivot that is not > 0 returns None."""
    cf = CF()
    masks = [cf.ALL, cf.POSE, cf.FOCAL | cf.CENTRE, cf.POSE | cf.FOCAL | cf.K1, cf.K1 | cf.K2 | cf.K3, cf.CENTRE]
    worst = 0.0
    for i, (A, g, dense) in enumerate(fc.spd_systems()):
        mask = masks[i % len(masks)]
        idx = cf.free_unknowns(mask)
        lam = [0.0, 1e-3, 10.0][i % 3]
        delta = cf.solve(A, g, lam, mask)
        assert delta is not None
        M = dense[np.ix_(idx, idx)].copy()
        M[np.diag_indices(len(idx))] *= 1.0 + lam
        want = np.linalg.solve(M, -g[idx])
        rel = np.abs(np.array(delta)[idx] - want).max() / np.abs(want).max()
        worst = max(worst, float(rel))
        assert rel <= 1e-12, (i, mask, rel)
        assert all(delta[u] == 0.0 for u in range(13) if u not in idx)
    print('worst relative difference', worst)
    A, g, dense = fc.spd_systems(1)[0]
    bad = A.copy()
    bad[cf.TRI.index((6, 7))] = 1.02 * np.sqrt(dense[6, 6] * dense[7, 7])          # fx, fy: not positive definite
    assert cf.solve(bad, g, 0.0, cf.FOCAL) is None and cf.solve(bad, g, 0.0, cf.ALL) is None
    assert cf.solve(bad, g, 0.0, cf.POSE) is not None                                 # the held rows are left out
    assert cf.solve(np.zeros(91), g, 1e-3, cf.ALL) is None
    assert [cf.free_unknowns(m) for m in (cf.POSE, cf.FOCAL | cf.K3)] == [[0, 1, 2, 3, 4, 5], [6, 7, 12]]
    with pytest.raises(ValueError):
        cf.free_mask(['focal', 'skew'])
    with pytest.raises(ValueError):
        cf.HostCameraFitter(*fc.true_set(zero_scene()), min_obs=12)


def test_solver_header_under_sanitizers_equals_the_statement(tmp_path):
    """6: tests/native/camfit_solve_test.cpp built with -fsanitize=address,undefined and run as a child process (nothing
    preloaded, nothing loaded into python): it replays, per camera, the passes of tests 2 and 3 -- the sums the statement
    saw, written as hex floats -- through camfit_cam_step and prints status, passes, lambda, delta, the trial and the
    accepted set and the four last_* after every step; all equal the statement's, bit for bit."""
    gxx = shutil.which('g++')
    if not gxx:
        pytest.skip('g++ not available')
    exe = str(tmp_path / 'camfit_solve_test')
    subprocess.run([gxx, '-O1', '-g', '-Wall', '-Werror', '-ffp-contract=off', '-fsanitize=address,undefined', '-fno-sanitize-recover=all',
                    '-I', os.path.join(ROOT, '3d_multi_pose_estimator_amd', 'csrc'), os.path.join(ROOT, 'tests', 'native', 'camfit_solve_test.cpp'),
                    '-o', exe], check=True, capture_output=True, timeout=300)
    import calib_cases as cc
    runs = []
    s2 = fc.Scene('panoptic', 8, 2, seed=4600, noise_px=1.0)
    E0, k, dist = fc.true_set(s2)
    log = []
    start2 = (cc.perturbed_start(E0, 0.8, 15.0, 44), k, dist)
    fc.run_host(s2, start2, 3, (1e-12, 1e-12, 1e-3, 1e-7), free=CF().POSE, min_obs=6, until_done=False, log=log)
    runs.append((start2, CF().POSE, 6, (1e-12, 1e-12, 1e-3, 1e-7), log))
    log3 = []
    zero_run(log=log3)
    runs.append((zero_start(zero_scene()), CF().ALL, 13, POSE_TOLS, log3))
    path = tmp_path / 'cases.txt'
    want = []
    with open(path, 'w') as fh:
        for start, mask, min_obs, tols, log in runs:
            for c in range(len(start[0])):
                nums = list(start[0][c].reshape(12)) + [float(x) for x in start[1][c]] + list(start[2][c]) + list(tols)
                fh.write('cam %d %d %d %s\n' % (mask, min_obs, len(log), ' '.join(float(x).hex() for x in nums)))
                for sums, snaps in log:
                    fh.write('pass %d %s\n' % (int(sums['n_obs'][c]), ' '.join(float(x).hex() for x in sums['acc'][c])))
                    want.append(snaps[c])
    r = subprocess.run([exe, str(path)], capture_output=True, text=True, timeout=120)
    assert r.returncode == 0, r.stdout + r.stderr
    m = re.search(r'self-checks (\d+) bad (\d+)', r.stdout)
    assert m and int(m.group(1)) >= 10 and int(m.group(2)) == 0, r.stdout
    lines = [ln.split()[1:] for ln in r.stdout.splitlines() if ln.startswith('step ')]
    assert len(lines) == len(want) > 30
    for i, (got, exp) in enumerate(zip(lines, want)):
        got = got[:2] + [float.fromhex(x).hex() for x in got[2:]]          # printf's %a drops trailing zeros; the value and its sign stay
        assert got == exp, (i, [(j, a, b) for j, (a, b) in enumerate(zip(got, exp)) if a != b][:4])


def test_calibration_intrinsics_and_declarations(tmp_path):
    """Calibration.with_intrinsics rebuilds K32 / Kinv32 / dist and leaves the original and params alone; intrinsics=None
    gives today's bits; with_extrinsics keeps fitted intrinsics; the "intrinsics" list of the script's file reads back to
    the same bits and load_transform_manager ignores it; lib.py's structs follow include/mpe.h."""
    import json

    import torch
    cal = pkg('calibration')
    calib = env().calib
    plain = cal.Calibration(calib.params, calib.tm)
    again = cal.Calibration(calib.params, calib.tm, intrinsics=None)
    for name in ('K32', 'Kinv32', 'dist', 'P', 'T_i32', 'centre32'):
        assert fc.same_bits(getattr(plain, name), getattr(again, name))
    k = calib.intrinsics()
    assert k.dtype == np.float32 and fc.same_bits(k[:, 0], calib.K32[:, 0, 0]) and fc.same_bits(k[:, 3], calib.K32[:, 1, 2])
    k2 = (k.astype(np.float64) * 1.01 + 0.3).astype(np.float32)
    d2 = np.array(calib.dist) + 0.01
    before = (np.array(calib.K32, copy=True), np.array(calib.dist, copy=True), list(calib.params.fx))
    new = calib.with_intrinsics(k2, d2)
    assert new is not calib and new.params is calib.params and list(calib.params.fx) == before[2]
    assert fc.same_bits(calib.K32, before[0]) and fc.same_bits(calib.dist, before[1])
    assert fc.same_bits(new.intrinsics(), k2) and fc.same_bits(new.dist, d2) and fc.same_bits(new.P, calib.P)
    for i in range(calib.n_cameras):
        assert fc.same_bits(new.Kinv32[i], torch.inverse(torch.from_numpy(new.K32[i])).numpy())
        assert new.K32[i][0, 1] == 0 and new.K32[i][2, 2] == 1
    moved = new.with_extrinsics(np.asarray(calib.P) + 0.0)
    assert fc.same_bits(moved.K32, new.K32) and fc.same_bits(moved.dist, new.dist)
    with pytest.raises(ValueError):
        calib.with_intrinsics(k2[:2], d2)
    with pytest.raises(ValueError):
        calib.with_intrinsics(-k2, d2)
    path = str(tmp_path / 'cams.json')
    with open(path, 'w') as fh:
        json.dump(CF().cameras_json(new), fh)
    tm = cal.load_transform_manager(path)
    back = cal.Calibration(calib.params, tm, cal.load_intrinsics(path, calib.params))
    for name in ('K32', 'Kinv32', 'dist', 'P', 'T_i'):
        assert fc.same_bits(getattr(back, name), getattr(new, name)), name
    assert cal.load_intrinsics(cal.default_transform_path(calib.params), calib.params) is None
    L = pkg('lib')
    with open(os.path.join(ROOT, 'include', 'mpe.h')) as fh:
        header = fh.read()
    for sym in ('create', 'destroy', 'reset', 'set_cameras', 'get_cameras', 'batch', 'read', 'step', 'launches'):
        assert 'mpe_camfit_' + sym in L.SYMBOLS and 'int mpe_camfit_%s(' % sym in header
    for name, struct in (('mpe_camfit_step_args', L.mpe_camfit_step_args), ('mpe_camfit_cam_report', L.mpe_camfit_cam_report)):
        body = re.search(r'typedef struct \{([^}]*)\} %s;' % name, header).group(1)
        body = re.sub(r'/\*.*?\*/', '', body, flags=re.S)
        fields = [re.sub(r'\[\d+\]', '', f).strip().lstrip('*') for decl in body.split(';') if decl.strip() for f in re.sub(
            r'\b(const|int32_t|uint32_t|int64_t|uint8_t|double|float|void)\b', '', decl).split(',')]
        assert fields == [f.rstrip('_') for f, _ in struct._fields_], (name, fields)
    assert L.MPE_CAMFIT_SUMS == CF().SUMS == 105 and '#define MPE_CAMFIT_SUMS 105' in header
    args = CF().build_own_parser().parse_args(['--synthetic', '4', '--free', 'focal,k1', '--perturb-focal', '1'])
    assert args.free == 'focal,k1' and args.perturb_focal == 1.0 and args.pix_tol == 1e-3 and args.lens_tol == 1e-7
