"""CPU: csrc/project64.h, the one camera model and 3-unknown LM step of the geometry kernels, built for the host with
-ffp-contract=off -fsanitize=address,undefined (tests/native/camera64_test.cpp, run as a child process) against the numpy
statement harness/refine.py: project64 with its Jacobian, _rho, huber_weight and lm_step3.  Every finite output has the
statement's bits; what is not finite is not finite in the same places."""
import os
import shutil
import subprocess

import numpy as np
import pytest

import refine_cases as rc
from conftest import ROOT, env, pkg

HUBERS = (0.0, 5.0)


@pytest.fixture(scope='module')
def exe(tmp_path_factory):
    cxx = shutil.which('g++') or shutil.which('c++') or shutil.which('clang++')
    assert cxx, 'no host C++ compiler'
    out = str(tmp_path_factory.mktemp('camera64') / 'camera64_test')
    subprocess.run([cxx, '-O1', '-std=c++17', '-Wall', '-Werror', '-ffp-contract=off', '-fsanitize=address,undefined', '-fno-sanitize-recover=all',
                    '-I', os.path.join(ROOT, '3d_multi_pose_estimator_amd', 'csrc'), os.path.join(ROOT, 'tests', 'native', 'camera64_test.cpp'), '-o', out],
                   check=True, capture_output=True, timeout=300)
    return out


def same_where_finite(got, want, what):
    got, want = np.asarray(got, np.float64), np.asarray(want, np.float64)
    assert got.shape == want.shape, what
    fin = np.isfinite(want)
    assert np.array_equal(fin, np.isfinite(got)), (what, 'finite in other places')
    assert np.array_equal(got[fin].view(np.int64), want[fin].view(np.int64)), (what, int((got[fin].view(np.int64) != want[fin].view(np.int64)).sum()))
    return int(fin.sum()), int((~fin).sum())


def on_plane(Tc):
    """A point whose pc2 is exactly 0.0 in the header's order of operations.  On the world axis k with the largest
    |T[2][k]| the product p = T[2][k] * x lands within a few ulps of -T[2][3]; the difference d = -T[2][3] - p is exact
    (Sterbenz), and a second axis carries it: T[2][j] * y = d to a rounding far below half an ulp of p, so p + that rounds to
    -T[2][3]."""
    k = int(np.argmax(np.abs(Tc[2, :3])))
    j = (k + 1) % 3
    X = np.zeros(3)
    X[k] = -Tc[2, 3] / Tc[2, k]
    X[j] = (-Tc[2, 3] - Tc[2, k] * X[k]) / Tc[2, j]
    assert ((Tc[2, 0] * X[0] + Tc[2, 1] * X[1]) + Tc[2, 2] * X[2]) + Tc[2, 3] == 0.0
    return X


def scene(variant, case):
    """-> (T [V,3,4], dist [V,5], K32 [V,3,3], points [n,3]): the rig's cameras by engine slot, a few hundred joints of the
    case's bodies, and per camera the points that break the lines: behind it, on its plane, far off its axis; a NaN."""
    R = pkg('harness.reprojection')
    T, dist, K32 = R.engine_calibration(env(variant).calib)
    bodies = np.concatenate([np.asarray(b, np.float64).reshape(-1, 3) for b in rc.raw(case)[2]])[:360]
    hard = [[np.nan, 0.1, 2.0], [0.3, np.inf, 1.0]]
    for Tc in T:
        Rm, t = Tc[:, :3], Tc[:, 3]
        centre = -Rm.T @ t
        hard.append(centre - 2.0 * Rm[2] + 0.1 * Rm[0])                   # pc2 = -2
        hard.append(centre)                                                # the centre, to rounding: tiny pc
        hard.append(on_plane(Tc))                                          # pc2 == 0: x / 0
        for far in (3.0, 30.0, 3000.0):
            hard.append(centre + 1.0 * Rm[2] + far * Rm[0] - far * Rm[1])  # r = 2 far^2: the lens polynomial's far end
    return T, dist, K32, np.concatenate([bodies, np.array(hard)])


def systems(T, kd, K, pts, rng):
    """LM systems over the scene's cameras: (X, lambda, huber, [(camera, ox, oy)], [(m, q)])."""
    R = pkg('harness.refine')
    V = len(T)
    out = []
    for i in range(0, 120):
        X = pts[i]
        cams = [c for c in range(V) if (i + c) % 3 != 0 or V < 4][:8]
        obs = []
        for c in cams:
            p = R.project64(T[c], kd[c], K[c], X[0], X[1], X[2])
            noise = rng.normal(0.0, [0.5, 3.0, 40.0][i % 3], 2)
            obs.append((c, float(p['px']) + noise[0], float(p['py']) + noise[1]))
        bones = [(rng.normal(0.0, 300.0, 3), float(rng.normal(0.0, 5.0))) for _ in range(i % 3)]
        out.append((X, [1e-3, 1e-12, 10.0][i % 3], HUBERS[i % 2], obs, bones))
    # singular: the same camera twice and nothing else, undamped -- A has rank 2, and the last pivot is what rounding leaves
    # of 0.  Per camera the first point at which the statement's pivot is not positive (rounding leaves a positive one at
    # about every other point; those solve, to a huge step, on both sides, and the next one is taken)
    for c in range(V):
        for X in pts[:60]:
            p = R.project64(T[c], kd[c], K[c], X[0], X[1], X[2])
            twice = (X, 0.0, 0.0, [(c, float(p['px']) + 1.0, float(p['py']) - 2.0)] * 2, [])
            if statement_step(R, T, kd, K, twice)[3] == 0.0:
                break
        else:
            raise AssertionError('camera %d: every rank-2 system has a positive last pivot' % c)
        out.append(twice)
    # and systems whose point is one of the hard ones, and an empty one
    for X in pts[-6:]:
        out.append((X, 1e-3, 5.0, [(0, 100.0, 200.0), (V - 1, 300.0, 100.0)], []))
    out.append((pts[0], 1e-3, 0.0, [], []))
    return out


def statement_step(R, T, kd, K, system):
    X, lam, huber, obs, bones = system
    A = {kl: np.zeros(()) for kl in R.PAIRS}
    g = [np.zeros(()) for _ in range(3)]
    with np.errstate(all='ignore'):
        for c, ox, oy in obs:
            p = R.project64(T[c], kd[c], K[c], X[0], X[1], X[2], jacobian=True)
            rx, ry = p['px'] - ox, p['py'] - oy
            w = R.huber_weight(np.sqrt(rx * rx + ry * ry), huber)
            for (k, l) in A:
                A[k, l] = A[k, l] + w * (p['jx'][k] * p['jx'][l] + p['jy'][k] * p['jy'][l])
            for k in range(3):
                g[k] = g[k] + w * (p['jx'][k] * rx + p['jy'][k] * ry)
        for m, q in bones:
            for (k, l) in A:
                A[k, l] = A[k, l] + m[k] * m[l]
            for k in range(3):
                g[k] = g[k] + m[k] * q
        delta, ok = R.lm_step3(A, g, np.float64(lam))
    return np.concatenate([delta, [1.0 if ok else 0.0]])


@pytest.mark.parametrize('variant,case', [('panoptic', '5x10'), ('arplab', 'one frame'), ('arprobot', 'arprobot')])
def test_header_has_the_statements_bits(exe, tmp_path, variant, case):
    """The cameras of data/tm_panoptic.json and data/tm_arp.json (all of ARPLAB's, then the robot preset's two slots)."""
    R = pkg('harness.refine')
    T, dist, K32, pts = scene(variant, case if variant != 'arplab' else '5x10')
    V, kd, K = len(T), np.ascontiguousarray(dist[:, [0, 1, 4]]), K32.astype(np.float64)
    rng = np.random.default_rng(64)
    es = np.concatenate([[0.0, 5.0, np.nextafter(5.0, 6.0), np.nextafter(5.0, 0.0), np.inf, np.nan], 10.0 ** rng.uniform(-6, 4, 200)])
    sys_ = systems(T, kd, K, pts, rng)
    words = [float(V), float(len(pts)), float(len(es)), float(len(HUBERS)), float(len(sys_))]
    for c in range(V):
        words += T[c].reshape(-1).tolist() + dist[c].tolist() + K[c].reshape(-1).tolist()
    words += pts.reshape(-1).tolist() + es.tolist() + list(HUBERS)
    for X, lam, huber, obs, bones in sys_:
        words += list(X) + [lam, huber, float(len(obs)), float(len(bones))]
        for o in obs:
            words += [float(o[0]), o[1], o[2]]
        for m, q in bones:
            words += list(m) + [q]
    src, dst = str(tmp_path / 'in.f64'), str(tmp_path / 'out.f64')
    np.asarray(words, np.float64).tofile(src)
    r = subprocess.run([exe, src, dst], capture_output=True, text=True, timeout=120)
    assert r.returncode == 0, r.stdout + r.stderr
    got = np.fromfile(dst, np.float64)
    n_proj, n_rho = V * len(pts) * 9, len(HUBERS) * len(es) * 2
    assert got.size == n_proj + n_rho + 4 * len(sys_)

    want, lens = np.empty((V, len(pts), 9)), np.empty((V, len(pts)))
    for c in range(V):
        p = R.project64(T[c], kd[c], K[c], pts[:, 0], pts[:, 1], pts[:, 2], jacobian=True)
        want[c] = np.stack([p['px'], p['py'], p['pc2']] + p['jx'] + p['jy'], axis=1)
        lens[c] = p['f']
    fin, rest = same_where_finite(got[:n_proj].reshape(want.shape), want, 'projection and Jacobian')
    behind, plane = (want[..., 2] < 0).sum(), (want[..., 2] == 0).sum()
    assert behind >= V and plane >= V and np.isnan(want[..., 2]).sum() >= V and rest > 0
    print('lens polynomial f: least %g, %d negative' % (np.nanmin(lens), (lens < 0).sum()))
    assert (lens < 0).any() or not kd.any()                             # far off the axis f has changed sign (tm_arp has no distortion)
    print('%s: %d cameras, %d points, %d finite words, %d not finite; %d behind, %d on the plane' % (variant, V, len(pts), fin, rest, behind, plane))

    want = np.stack([np.stack([R._rho(es, h), R.huber_weight(es, h)], axis=1) for h in HUBERS])
    same_where_finite(got[n_proj:n_proj + n_rho].reshape(want.shape), want, 'rho and the weight')

    want = np.stack([statement_step(R, T, kd, K, s) for s in sys_])
    step = got[n_proj + n_rho:].reshape(-1, 4)
    same_where_finite(step, want, 'the LM step')
    ok = want[:, 3] == 1.0
    assert ok[:120].sum() >= 100, ok[:120].sum()                       # the ordinary systems solve
    assert not ok[120:120 + V].any()                                     # the same camera twice: singular, on both sides
    assert not ok[-1] and not ok[-7:-1].all()                           # no observation at all; points that project to nothing
