"""Inputs for the camera-fit tests (test_camfit_host.py: harness/camfit.py and csrc/camfit_solve.h on their own;
test_gpu_camfit.py: mpe_camfit_* against them).  The scenes are calib_cases.Scene's; a trial set is (E [V,3,4] f64,
k [V,4] f32: fx fy cx cy, dist [V,5] f64).  Everything is seeded.  Not a test module."""
import numpy as np

import calib_cases as cc
from calib_cases import Scene, same_bits  # noqa: F401  (the tests take them from here)
from conftest import pkg

ALL_JOINTS = cc.ALL_JOINTS
KD = [0, 1, 4]                                   # the radial terms among dist's five numbers


def CF():
    return pkg('harness.camfit')


def CB():
    return pkg('harness.calibrate')


def true_set(scene):
    """The rig's own cameras as a trial set."""
    return CF().start_cameras(scene.calib)


def moved_set(scene, seed, deg=0.4, mm=8.0, focal=1.01, centre=(5.0, -5.0), kd=(0.02, -0.01, 0.005), cameras=None):
    """The rig's set moved off in all thirteen unknowns (every camera, or `cameras`)."""
    E, k, dist = true_set(scene)
    moved = cc.perturbed_start(E, deg, mm, seed)
    for c in (range(len(E)) if cameras is None else cameras):
        E[c] = moved[c]
        k[c, :2] = (k[c, :2].astype(np.float64) * focal).astype(np.float32)
        k[c, 2:] = (k[c, 2:].astype(np.float64) + np.array(centre)).astype(np.float32)
        dist[c, KD] = dist[c, KD] + np.array(kd)
    return E, k, dist


def one_pass(scene, cams, **kw):
    """camfit_pass_host over the scene, or over the frames [a, b) of it packed on their own (Scene.one_pass's arguments)."""
    return scene.one_pass(cams, pass_host=CF().camfit_pass_host, **kw)


def run_host(scene, start, passes, tols, free=63, hold=(), min_obs=13, huber_px=0.0, until_done=True, log=None, **pass_kw):
    """Passes and steps of the statement -> (HostCameraFitter, the reports in order).  log: a list that receives, per
    pass, (the sums, a snapshot of every camera after the step) for the stand-alone program to replay."""
    state = CF().HostCameraFitter(*start, free=free, hold=hold, min_obs=min_obs)
    reports = []
    for _ in range(passes):
        sums = one_pass(scene, state.trial(), huber_px=huber_px, **pass_kw)
        reports.append(CF().camfit_step_host(state, sums, *tols))
        if log is not None:
            log.append(({k: np.array(v, copy=True) for k, v in sums.items()}, [snapshot(c) for c in state.cams]))
        if until_done and reports[-1]['all_done']:
            break
    return state, reports


def snapshot(cam):
    """What the stand-alone program prints after a step, as hex strings."""
    nums = [cam.lam] + list(cam.delta) + list(cam.t.E.reshape(12)) + [float(x) for x in cam.t.k] + list(cam.t.dist) + \
        list(cam.a.E.reshape(12)) + [float(x) for x in cam.a.k] + list(cam.a.dist) + [cam.last_rot, cam.last_trans, cam.last_pix, cam.last_lens]
    return [str(int(cam.status)), str(int(cam.passes))] + [float(x).hex() for x in nums]


def camera_distance(cams, truth, c):
    """-> the distances of camera c of a set to the truth: {'rot' rad, 'trans' m, 'fx', 'fy', 'cx', 'cy' px, 'kd0', 'kd1', 'kd2'}."""
    (E, k, dist), (Et, kt, dt) = cams, truth
    rot, trans = CB().extrinsics_distance(E[c], Et[c])
    out = {'rot': rot, 'trans': trans}
    for i, name in enumerate(('fx', 'fy', 'cx', 'cy')):
        out[name] = abs(float(k[c][i]) - float(kt[c][i]))
    for i, name in zip(KD, ('kd0', 'kd1', 'kd2')):
        out[name] = abs(float(dist[c][i]) - float(dt[c][i]))
    return out


def camera_residuals(scene, c, start):
    """-> fn(x): the residual vector (rx and ry of every observation of camera c) with the camera at the start set moved by
    the thirteen-vector x (pose by compose, the rest added in float64: scipy's K is not rounded to float32), and
    unpack(x) -> (E [3,4], k [4] f64, dist [5]): what scipy's optimiser is given, on the same observations from the same
    start."""
    sel, xy = pkg('harness.reprojection').selection(scene.pb, scene.persons, scene.n_persons, scene.flags, ALL_JOINTS)
    pick = sel[:, :, c]
    X = scene.truth[pick]
    obs = xy[:, :, c][pick]
    E0, k0, d0 = start[0][c], start[1][c].astype(np.float64), start[2][c]

    def unpack(x):
        k = k0 + x[6:10]
        dist = d0.copy()
        dist[KD] = dist[KD] + x[10:13]
        return CB().compose(E0, x[:6]), k, dist

    def fn(x):
        E, k, dist = unpack(x)
        K = np.array([[k[0], 0.0, k[2]], [0.0, k[1], k[3]], [0.0, 0.0, 1.0]])
        p = CB().project_camera(E, dist[KD], K, X[:, 0], X[:, 1], X[:, 2])
        return np.concatenate([p['px'] - obs[:, 0], p['py'] - obs[:, 1]])
    return fn, unpack


def scipy_fit(scene, c, start):
    """scipy's Levenberg-Marquardt on the thirteen unknowns of camera c from the start set -> ((E, k f64, dist), cost)."""
    from scipy.optimize import least_squares
    fn, unpack = camera_residuals(scene, c, start)
    scale = np.array([1e-3] * 3 + [1e-2] * 3 + [1.0] * 4 + [1e-2, 1e-2, 1e-2])
    sol = least_squares(fn, np.zeros(13), method='lm', x_scale=scale, ftol=1e-15, xtol=1e-15, gtol=1e-15, max_nfev=4000)
    return unpack(sol.x), float(np.sum(sol.fun ** 2))


def spd_systems(n=200, seed=616):
    """Seeded 13 x 13 symmetric positive definite systems with the scales of a camera's normal equations -> (A [91], g [13],
    the dense matrix)."""
    rng = np.random.default_rng(seed)
    scale = np.array([3000.] * 3 + [400.] * 3 + [0.3, 0.3, 1.0, 1.0, 40.0, 8.0, 2.0])
    out = []
    for _ in range(n):
        Jm = rng.normal(size=(60, 13)) * scale
        A, g = Jm.T @ Jm, Jm.T @ (rng.normal(size=60) * 3.0)
        out.append((np.array([A[k, l] for k, l in CF().TRI]), g, A))
    return out
