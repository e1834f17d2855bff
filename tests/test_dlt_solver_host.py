"""CPU: csrc/dlt_solve.h, the one two-view DLT solver of every kernel, built for the host with -fsanitize=address,undefined
(tests/native/dlt_solve_host.cpp, run as a child process) against numpy.linalg.svd of the same systems (dlt_cases.py has the
systems and the bounds).  Two builds: the host's own 1 / sqrt and 1 / x as the rsq / rcp estimates, and the estimates rounded to
24 bits (coarser than the hardware's), which is what the Newton steps of the rotation are there for."""
import json
import os
import re
import shutil
import subprocess
from fractions import Fraction

import numpy as np
import pytest

import dlt_cases as dc
from conftest import ROOT

BUILDS = {'exact': [], 'coarse': ['-DMPE_DLT_COARSE_ESTIMATES']}
_exe = {}


@pytest.fixture(scope='module')
def build_dir(tmp_path_factory):
    return tmp_path_factory.mktemp('dlt_solve_host')


def exe(build_dir, build):
    if build not in _exe:
        cxx = shutil.which('g++') or shutil.which('c++') or shutil.which('clang++')
        assert cxx, 'no host C++ compiler'
        out = str(build_dir / ('dlt_solve_host_' + build))
        subprocess.run([cxx, '-O1', '-g', '-std=c++17', '-Wall', '-Werror', '-fsanitize=address,undefined', '-fno-sanitize-recover=all'] + BUILDS[build] +
                       ['-I', os.path.join(ROOT, '3d_multi_pose_estimator_amd', 'csrc'), os.path.join(ROOT, 'tests', 'native', 'dlt_solve_host.cpp'), '-o', out],
                       check=True, capture_output=True, timeout=300)
        _exe[build] = out
    return _exe[build]


def run(build_dir, build, mode, data, width):
    src, dst = str(build_dir / 'in.f64'), str(build_dir / 'out.f64')
    np.ascontiguousarray(data, np.float64).tofile(src)
    r = subprocess.run([exe(build_dir, build), mode, src, dst], capture_output=True, text=True, timeout=120)
    assert r.returncode == 0, r.stdout + r.stderr
    m = re.search(r'done (\d+) most sweeps (\d+) cap (\d+)', r.stdout)
    assert m and int(m.group(1)) == len(data) and int(m.group(3)) == 12, r.stdout
    return np.fromfile(dst, np.float64).reshape(len(data), width), int(m.group(2))


@pytest.mark.parametrize('build', list(BUILDS))
@pytest.mark.parametrize('variant', ['panoptic', 'arplab'])
def test_solver_against_lapack(build_dir, variant, build):
    """Matched pairs to 1e-10 m, well-posed mismatched pairs to 1e-10 m x max(1, |X|) (at least 80 % of them), every mismatched pair the
    right vector by its residual; no system needs the cap of 12 sweeps."""
    s = dc.systems(variant)
    out, most = run(build_dir, build, 'solve', s.host_input(), 4)
    print('%s %s: mean sweeps %.2f, most %d' % (build, variant, out[:, 3].mean(), most))
    assert most < 12
    dc.check(s, out[:, :3], 'host/' + build)


@pytest.mark.parametrize('build', list(BUILDS))
def test_degenerate_systems_finish_within_the_cap(build_dir, build):
    """Both views from the same camera: the same point twice (rank 2), two different points (rank 3, the null vector is the camera
    centre), and the all-zero system.  The program finishes, clean under the sanitizers, and no solve passes the cap."""
    s = dc.systems('panoptic')
    inp = s.host_input()[:64].copy()
    inp[:, 12:24] = inp[:, :12]                       # second view: the first camera again
    inp[:32, 26:28] = inp[:32, 24:26]                 # ... looking at the same point
    inp = np.concatenate([inp, np.zeros((1, 28))])
    out, most = run(build_dir, build, 'solve', inp, 4)
    print('degenerate: sweeps', out[:, 3].astype(int).tolist())
    assert most <= 12 and (out[:, 3] >= 0).all() and (out[:, 3] <= 12).all()
    centre = -np.linalg.solve(s.P1[32:64, :, :3], s.P1[32:64, :, 3:4])[..., 0]
    assert np.abs(out[32:64, :3] - centre).max() < 1e-9


@pytest.mark.parametrize('build', list(BUILDS))
def test_rotation_is_orthonormal_to_a_few_ulp(build_dir, build):
    """dlt_rotation on squared norms over twelve decades and inner products from 1e-15 to 1 of their limit: |c^2 + s^2 - 1| (in exact
    arithmetic on the returned doubles) within 16 x 2^-53 -- c is 1 / sqrt(1 + t^2) through three roundings and s = c t a fourth, each
    half an ulp of a number near 1 -- and the rotated inner product small against the norms: t need not be correctly rounded, but the
    pair must come out orthogonal to 1e-12 of its norms, so that the next visit's rotation is the last."""
    rng = np.random.default_rng(7)
    n = 4000
    al, be = 10.0 ** rng.uniform(-6, 6, n), 10.0 ** rng.uniform(-6, 6, n)
    be[:400] = al[:400]                               # d = 0
    be[400:800] = al[400:800] * (1 + 1e-15 * rng.integers(-8, 9, 400))
    rho = 10.0 ** rng.uniform(-15, 0, n) * rng.choice([-1.0, 1.0], n)
    ga = rho * np.sqrt(al * be)
    out, _ = run(build_dir, build, 'rot', np.stack([al, be, ga], axis=1), 2)
    c, s = out[:, 0], out[:, 1]
    assert np.isfinite(out).all() and (c > 0).all()
    orth = max(abs(float(Fraction(ci) ** 2 + Fraction(si) ** 2 - 1)) for ci, si in zip(c.tolist(), s.tolist()))
    # <a_p', a_q'> = c s (al - be) + (c^2 - s^2) ga, against |a_p'||a_q'| <= (al + be) / 2
    left = max(abs(float(Fraction(ci) * Fraction(si) * (Fraction(a) - Fraction(b)) + (Fraction(ci) ** 2 - Fraction(si) ** 2) * Fraction(g))) / (a + b)
               for ci, si, a, b, g in zip(c.tolist(), s.tolist(), al.tolist(), be.tolist(), ga.tolist()))
    print('%s: max |c^2 + s^2 - 1| %.3g (%.1f x 2^-53), max rotated inner product / (al + be) %.3g' % (build, orth, orth * 2.0 ** 53, left))
    assert orth <= 16 * 2.0 ** -53
    assert left <= 1e-12


def test_window_edge_f64_and_float_windows_disagree():
    """Why mpe_config.median_window is a double.  The frame of window_edge_case.py through the oracle's triangulation (numpy's SVD):
    a bisection on the displacement t finds the point at which one moved pair sits less than 5e-10 m OUTSIDE the 5 cm window.  The
    reference's comparison (`dist_to_median < 0.05`, doubles) drops that pair; the same comparison against float(0.05) =
    0.05000000074505806, which is what a float field hands the kernel, keeps it, and the joint moves by
    more than 7 mm."""
    import window_edge_case as we
    from conftest import env, oracle, pkg
    onp, syn, calib = oracle(), pkg('synthetic'), env('panoptic').calib
    params = calib.params
    axis = params.axes_3D['Y'][0]
    cams = list(params.camera_names)
    assert we.JOINT in params.used_joints and len(cams) == 5

    def skeletons(t):
        fr, _ = we.frame(calib, syn, t)
        return {c: json.loads(fr[c][0])[0] for c in cams}

    def pair_points(t):
        """The oracle's pair loop for the one joint (oracle_np.triangulate_person)."""
        sk = skeletons(t)
        und = [onp.undistort_points(np.array(sk[c][str(we.JOINT)][1:3]), calib.K32[calib.index(c)], calib.dist[calib.index(c)])[0] for c in cams]
        return np.array([onp.dlt_pair(calib.P[calib.index(cams[a])], calib.P[calib.index(cams[b])], und[a], und[b])
                         for a in range(5) for b in range(a + 1, 5)])

    t_out, t_in, k, steps = we.bisect(lambda t: we.window_distances(pair_points(t), axis))
    d_out, d_in = we.window_distances(pair_points(t_out), axis)[k], we.window_distances(pair_points(t_in), axis)[k]
    print('t outside %.12f px (distance - 0.05 = %.3g m), t inside %.12f px (%.3g m), pair %d, %d steps' % (t_out, d_out - 0.05, t_in, d_in - 0.05, k, steps))
    assert we.WINDOW <= d_out < we.WINDOW + we.BAND and we.WINDOW - we.BAND < d_in < we.WINDOW
    pts = pair_points(t_out)
    want, kept = we.filtered_mean(pts, axis, we.WINDOW)
    # the oracle itself (the reference's rule restated) is the f64 window: same bits as numpy's mean over the kept pairs up to its summation order
    ref = onp.triangulate_person(skeletons(t_out), calib, all_joints=True)[we.JOINT]
    assert np.abs(ref - want).max() < 1e-15
    as_float, kept_float = we.filtered_mean(pts, axis, we.WINDOW_AS_FLOAT)
    assert kept_float == kept + 1, (kept, kept_float)
    moved = np.linalg.norm(as_float - want)
    print('f64 window keeps %d of 10 pairs, the float window %d; the joint moves by %.1f mm' % (kept, kept_float, 1e3 * moved))
    # the kept pairs are the six that never moved (all at the median), the seventh is 5 cm from it along Y: 0.05 / 7 m along Y alone
    assert kept == 6 and moved > 0.05 / 7 * 0.99
    # inside the window the two agree
    pts = pair_points(t_in)
    a, ka = we.filtered_mean(pts, axis, we.WINDOW)
    b, kb = we.filtered_mean(pts, axis, we.WINDOW_AS_FLOAT)
    assert ka == kb == kept + 1 and np.array_equal(a, b)
