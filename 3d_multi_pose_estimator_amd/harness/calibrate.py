"""numpy statement of what mpe_calib_batch and mpe_calib_step compute (csrc/calib.hip, csrc/calib_solve.h): the camera
extrinsics refined from a recording's own poses, the 3D joints held fixed -- and the script that alternates this with the
matching / triangulation / refinement stages, which is a bundle adjustment of the rig.  The GPU tests hold the kernel's sums
to `calib_pass_host` bit for bit and the step's delta to `calib_step_host` bit for bit.  include/mpe.h words the rule; the
lines below are its lines.

All arithmetic is float64, every operation rounded on its own (numpy fuses nothing; the solver runs on Python floats, which
are IEEE doubles), in the header's order.  The observations of a camera are the entries harness/reprojection.py counts.

As a script:

    python -m 3d_multi_pose_estimator_amd.harness.calibrate --testfiles F.json --tmdir DIR --matcher geometric \
        --rounds R --passes N [--calib-huber PX] [--hold NAME ...] [--regroup PX] [--merge M] [--found M] [--refine ITERS] [--out tm.json]

A round matches, triangulates, (with --regroup) regroups and (with --refine) refines every batch with the current engine,
keeps batches and poses on the device, runs up to N passes and steps over them, and builds a new engine from the
calibrator's extrinsics.  One camera is held by default (the first): the alternation leaves the global similarity of the
rig free, and a held camera pins most of it.
--synthetic N --perturb-deg D --perturb-mm M runs on generated frames from a calibration with one camera moved, and also
prints every camera's distance to the true extrinsics.
"""
import json
import math

import numpy as np

from . import reprojection as R
from .refine import camera_constants64, huber_weight, jacobian_tail, project64, radial_slope, _rho

HELD, FEW_OBS, CONVERGED, STALLED, ACCEPTED, REJECTED = 1, 2, 4, 8, 16, 32
MAX_RETRIES = 8


class Family:
    """What a family of csrc/normal_sums.h states: N unknowns per camera, hence the layout of a camera's sums (q = 0 ..
    G0-1 the upper triangle of A row by row, TRI[q] = (k, l); G0 .. COST-1 g; COST the cost: SUMS = N(N+1)/2 + N + 1 in
    all) and project(*the camera's entries of a trial set, X0, X1, X2, jacobian=True) -> project_camera's dict with Jx / Jy
    as lists of N arrays.  This module's is FAMILY (6 unknowns), harness/camfit.py's has 13."""

    def __init__(self, N, project):
        self.N, self.project = N, project
        self.TRI = [(k, l) for k in range(N) for l in range(k, N)]
        self.G0, self.COST, self.SUMS = len(self.TRI), len(self.TRI) + N, len(self.TRI) + N + 1


def project_camera(T, kd, K, X0, X1, X2, jacobian=False):
    """One camera (T [3,4] the trial extrinsics, kd [3], K [3,3], float64), points X0 / X1 / X2 [...] float64 -> a dict
    with px, py, pc (three arrays) and, with jacobian, Jx / Jy: lists of six arrays, the derivatives of px / py by the
    perturbation xi = (w, tau) of the camera.  The header's lines."""
    with np.errstate(all='ignore'):
        out = project64(T, kd, K, X0, X1, X2)
        if jacobian:
            pc, h0, h1 = out['pc'], out['h0'], out['h1']
            fd = radial_slope(kd, out['r'])
            zero = np.zeros_like(h0)
            a = [1.0 / pc[2], zero, (-h0) / pc[2]]
            b = [zero, 1.0 / pc[2], (-h1) / pc[2]]
            rows = [jacobian_tail(out, K, fd, a[k], b[k]) for k in range(3)]
            cx, cy = [x for x, _ in rows], [y for _, y in rows]
            out['Jx'] = [cx[2] * pc[1] - cx[1] * pc[2], cx[0] * pc[2] - cx[2] * pc[0], cx[1] * pc[0] - cx[0] * pc[1], cx[0], cx[1], cx[2]]
            out['Jy'] = [cy[2] * pc[1] - cy[1] * pc[2], cy[0] * pc[2] - cy[2] * pc[0], cy[1] * pc[0] - cy[0] * pc[1], cy[0], cy[1], cy[2]]
    return out


FAMILY = Family(6, project_camera)             # a trial set is (E [V,3,4], kd [V,3], K [V,3,3]) by camera slot; only E moves
SUMS, TRI = FAMILY.SUMS, FAMILY.TRI            # 28; q = 0..20 -> (k, l)

engine_cameras = R.engine_cameras             # the one mapping (harness/reprojection.py), under the name this module's callers use


def start_extrinsics(calib):
    """cfg.P of an Engine built from `calib`: [V,3,4] float64."""
    return R.engine_calibration(calib)[0]


def new_sums(V, n_sums=SUMS):
    return {'acc': np.zeros((V, n_sums)), 'n_obs': np.zeros(V, np.int64), 'n_skipped': np.zeros(V, np.int64)}


def observation_terms(fam, cams, pb, persons, n_persons, poses, flags, joint_mask, threshold=0.5, huber_px=0.0):
    """fam: the Family; cams: the trial set, arrays over the camera slots.  -> (summed [F,Pcap,V,J] bool, skipped
    [F,Pcap,V,J] bool, terms [F,Pcap,V,J,fam.SUMS] float64: what every observation adds to its camera's sums; unspecified
    where summed is False)."""
    if not huber_px >= 0.0:
        raise ValueError('huber_px >= 0')
    huber = float(huber_px)
    poses = np.asarray(poses)
    if poses.dtype not in (np.float32, np.float64):
        raise ValueError('poses must be float32 or float64')
    sel, xy = R.selection(pb, persons, n_persons, flags, joint_mask, threshold)
    F, Pcap, V, J = sel.shape
    X = poses.astype(np.float64)
    terms = np.zeros((F, Pcap, V, J, fam.SUMS))
    summed = np.zeros(sel.shape, bool)
    finite = np.isfinite(X).all(axis=-1)                                          # [F,Pcap,J]
    with np.errstate(all='ignore'):
        for c in range(V):
            p = fam.project(*(x[c] for x in cams), X[..., 0], X[..., 1], X[..., 2], jacobian=True)
            ok = sel[:, :, c] & finite & (p['pc'][2] > 0.0) & np.isfinite(p['px']) & np.isfinite(p['py'])
            summed[:, :, c] = ok
            rx = p['px'] - xy[:, :, c, :, 0]
            ry = p['py'] - xy[:, :, c, :, 1]
            e = np.sqrt(rx * rx + ry * ry)
            w, rho = huber_weight(e, huber), _rho(e, huber)
            Jx, Jy = p['Jx'], p['Jy']
            for q, (k, l) in enumerate(fam.TRI):
                terms[:, :, c, :, q] = w * (Jx[k] * Jx[l] + Jy[k] * Jy[l])
            for k in range(fam.N):
                terms[:, :, c, :, fam.G0 + k] = w * (Jx[k] * rx + Jy[k] * ry)
            terms[:, :, c, :, fam.COST] = rho
    return summed, sel & ~summed, terms


def pass_host(fam, cams, pb, persons, n_persons, poses, flags, joint_mask, threshold=0.5, huber_px=0.0, sums=None):
    """One mpe_calib_batch / mpe_camfit_batch call on the host (normal_batch of csrc/api.hip): the observations of the
    batch under the trial set `cams`, added to `sums` (new_sums(V, fam.SUMS) at the start of a pass), which is returned."""
    persons = np.asarray(persons)
    F, Pcap, V = persons.shape
    sums = new_sums(V, fam.SUMS) if sums is None else sums
    if F == 0:
        return sums
    summed, skipped, terms = observation_terms(fam, cams, pb, persons, n_persons, poses, flags, joint_mask, threshold, huber_px)
    J = summed.shape[-1]
    S = np.zeros((F, V, fam.SUMS))                                                # the frame partials: left folds over p, then j
    for p in range(Pcap):
        for j in range(J):
            S = np.where(summed[:, p, :, j, None], S + terms[:, p, :, j, :], S)
    acc = sums['acc']
    for f in range(F):                                                            # every frame, in order
        acc = acc + S[f]
    sums['acc'] = acc
    sums['n_obs'] = sums['n_obs'] + summed.sum(axis=(0, 1, 3))
    sums['n_skipped'] = sums['n_skipped'] + skipped.sum(axis=(0, 1, 3))
    return sums


def calib_pass_host(calib, E, pb, persons, n_persons, poses, flags, joint_mask, threshold=0.5, huber_px=0.0, sums=None):
    """One mpe_calib_batch call on the host.  E [V,3,4]: the trial extrinsics; pb, persons, n_persons, poses, flags,
    joint_mask, threshold: as reprojection.residuals takes them.  sums: what earlier calls of the pass left (new_sums(V)
    at the start of a pass); it is updated and returned: {'acc' [V,28], 'n_obs' [V], 'n_skipped' [V]}."""
    _, kd, K = camera_constants64(calib)                                          # by camera slot, as E is
    return pass_host(FAMILY, (np.asarray(E, np.float64), kd, K), pb, persons, n_persons, poses, flags, joint_mask, threshold, huber_px, sums)


# ---- the step: csrc/calib_solve.h, statement for statement, on Python floats -------------------------------------------

def ldlt(A, g, N, idx, lam):
    """calib_ldlt.  A: the stored upper triangle of order N row by row, g: N, idx: the unknowns solved for, ascending, lam
    -> y (list of len(idx) floats) or None when a pivot is not > 0 or a y is not finite."""
    n = len(idx)
    M = [[0.0] * n for _ in range(n)]
    for k in range(n):
        for l in range(k, n):
            M[k][l] = M[l][k] = float(A[idx[k] * N - idx[k] * (idx[k] - 1) // 2 + (idx[l] - idx[k])])       # calib_tri_of
    for k in range(n):
        M[k][k] = M[k][k] + lam * M[k][k]
    L = [[0.0] * n for _ in range(n)]
    D = [0.0] * n
    for j in range(n):
        v = [L[j][k] * D[k] for k in range(j)]
        d = M[j][j]
        for k in range(j):
            d = d - L[j][k] * v[k]
        if not d > 0.0:
            return None
        D[j] = d
        for i in range(j + 1, n):
            t = M[i][j]
            for k in range(j):
                t = t - L[i][k] * v[k]
            L[i][j] = t / d
    z = [0.0] * n
    for i in range(n):
        t = -float(g[idx[i]])
        for k in range(i):
            t = t - L[i][k] * z[k]
        z[i] = t
    y = [0.0] * n
    for i in range(n - 1, -1, -1):
        t = z[i] / D[i]
        for k in range(i + 1, n):
            t = t - L[k][i] * y[k]
        y[i] = t
    return y if all(math.isfinite(x) for x in y) else None


def solve6(A, g, lam):
    """A: the 21 entries of the upper triangle row by row, g: 6, lam -> delta (list of 6 floats) or None when a pivot is
    not > 0 or a delta is not finite (calib_solve6)."""
    return ldlt(A, g, 6, range(6), lam)


def norm3(w):
    return math.sqrt((w[0] * w[0] + w[1] * w[1]) + w[2] * w[2])


def max_abs(x):
    m = 0.0
    for v in x:
        m = max(m, abs(float(v)))
    return m


def rodrigues(w):
    """exp of the rotation vector w -> 3 x 3 nested lists (calib_exp)."""
    t = norm3(w)
    if t < 1e-8:
        a = 1.0 - (t * t) / 6.0
        b = 0.5 - (t * t) / 24.0
    else:
        s = math.sin(t / 2.0)
        a = math.sin(t) / t
        b = (2.0 * (s * s)) / (t * t)
    W = [0.0, -w[2], w[1], w[2], 0.0, -w[0], -w[1], w[0], 0.0]
    s0, s1, s2 = w[0] * w[0], w[1] * w[1], w[2] * w[2]
    W2 = [-(s1 + s2), w[0] * w[1], w[0] * w[2], w[0] * w[1], -(s0 + s2), w[1] * w[2], w[0] * w[2], w[1] * w[2], -(s0 + s1)]
    return [[((1.0 if i == j else 0.0) + a * W[3 * i + j]) + b * W2[3 * i + j] for j in range(3)] for i in range(3)]


def compose(Ea, xi):
    """[exp(w) R_a | exp(w) t_a + tau] -> [3,4] float64 (calib_compose)."""
    X = rodrigues([float(x) for x in xi[:3]])
    Ea = np.asarray(Ea, np.float64).reshape(3, 4)
    Et = np.zeros((3, 4))
    for i in range(3):
        for j in range(4):
            Et[i, j] = (X[i][0] * float(Ea[0, j]) + X[i][1] * float(Ea[1, j])) + X[i][2] * float(Ea[2, j])
        Et[i, 3] = float(Et[i, 3]) + float(xi[3 + i])
    return Et


LM_REFUSED, LM_STOPPED, LM_HELD, LM_FIRST, LM_ACCEPTED, LM_REJECTED = -1, 0, 1, 2, 3, 4


class LMState:
    """calib_lm, with the sums at the accepted set and the last perturbation: what a camera carries from step to step
    whatever its unknowns are.  The camera classes add their sets."""

    def __init__(self, fam):
        self.Aa = np.zeros(fam.SUMS)
        self.delta = [0.0] * fam.N
        self.lam = 1e-3
        self.cost_start = self.last_rot = self.last_trans = 0.0
        self.n_obs = 0
        self.status = self.passes = 0

    def refuses(self, n_obs):
        """n_obs is not the first pass's."""
        return self.passes > 0 and int(n_obs) != self.n_obs

    def lm_step(self, sums, n_obs, held, min_obs):
        """calib_lm_step: the bookkeeping of one step; `sums` (the cost last) and n_obs are what the pass at the trial
        left.  -> what the caller does with its sets:
          LM_REFUSED   n_obs is not the first pass's: nothing is changed
          LM_STOPPED   the camera had converged or stalled: nothing more is changed
          LM_HELD      held, or fewer than min_obs observations: trial = accepted (Aa = sums, reported, never solved)
          LM_FIRST     the first pass: accepted = trial, Aa = sums, lambda kept; build a trial
          LM_ACCEPTED  the cost fell: accepted = trial, Aa = sums, lambda / 10 (at least 1e-12); test convergence, else build a trial
          LM_REJECTED  the cost did not fall (an equal or NaN cost included): lambda * 10; build a trial"""
        if self.refuses(n_obs):
            return LM_REFUSED
        C = float(sums[-1])
        first = self.passes == 0
        self.passes += 1
        self.status &= ~(ACCEPTED | REJECTED | HELD | FEW_OBS)
        if first:
            self.n_obs, self.cost_start = int(n_obs), C
        if held or self.n_obs < min_obs:
            self.status |= HELD | (FEW_OBS if self.n_obs < min_obs else 0)
            self.Aa = np.array(sums, np.float64)
            return LM_HELD
        if self.status & (CONVERGED | STALLED):
            return LM_STOPPED
        if not first and not C < float(self.Aa[-1]):
            self.status |= REJECTED
            self.lam = self.lam * 10.0
            return LM_REJECTED
        self.Aa = np.array(sums, np.float64)
        self.status |= ACCEPTED
        if first:
            return LM_FIRST
        self.lam = max(self.lam / 10.0, 1e-12)
        return LM_ACCEPTED

    @property
    def done(self):
        return bool(self.status & (HELD | CONVERGED | STALLED))


class CameraState(LMState):
    """calib_cam: a camera's accepted and trial extrinsics."""

    def __init__(self, E):
        super().__init__(FAMILY)
        self.Ea = np.array(E, np.float64).reshape(3, 4)
        self.Et = self.Ea.copy()

    def trial(self):
        for attempt in range(MAX_RETRIES + 1):
            d = solve6(self.Aa[:21], self.Aa[21:27], self.lam)
            if d is not None:
                self.delta = d
                self.Et = compose(self.Ea, d)
                self.last_rot, self.last_trans = norm3(d[:3]), norm3(d[3:])
                return
            if attempt < MAX_RETRIES:
                self.lam = self.lam * 10.0
        self.status |= STALLED
        self.Et = self.Ea.copy()

    def step(self, sums, n_obs, held, min_obs, rot_tol, trans_tol):
        """calib_cam_step."""
        what = self.lm_step(sums, n_obs, held, min_obs)
        if what in (LM_REFUSED, LM_STOPPED):
            return
        if what == LM_HELD:
            self.Et = self.Ea.copy()
            return
        if what != LM_REJECTED:
            self.Ea = self.Et.copy()
        if what == LM_ACCEPTED and norm3(self.delta[:3]) < rot_tol and max_abs(self.delta[3:]) < trans_tol:
            self.status |= CONVERGED
            return
        self.trial()


class HostCalibrator:
    """The state of mpe_calib_*: a CameraState per camera.  trial() is what the next pass is taken at."""

    def __init__(self, E, hold=(), min_obs=6):
        if min_obs < 6:
            raise ValueError('min_obs >= 6')
        self.cams = [CameraState(e) for e in np.asarray(E, np.float64).reshape(-1, 3, 4)]
        self.hold, self.min_obs = set(int(c) for c in hold), int(min_obs)

    def trial(self):
        return np.stack([c.Et for c in self.cams])

    def accepted(self):
        return np.stack([c.Ea for c in self.cams])


def calib_step_host(state, sums, rot_tol, trans_tol):
    """mpe_calib_step on the host: `state` a HostCalibrator, `sums` what the pass at state.trial() left (calib_pass_host).
    -> the report: {'status', 'passes', 'n_obs', 'n_skipped', 'cost_start', 'cost', 'lambda', 'last_rot', 'last_trans'}
    as arrays over the cameras, 'delta' [V,6] (the perturbation of the last trial built) and 'all_done'."""
    return step_host(state, sums, rot_tol, trans_tol)


def step_host(state, sums, *rule, more=()):
    """normal_step of csrc/api.hip on the host: every camera of `state` (.cams, .hold, .min_obs) takes its step under
    `rule`, the arguments its step() takes after min_obs.  The passes that did not see the same data are refused before
    any camera has changed.  -> the report; `more` names what a family reports beside last_rot and last_trans."""
    n_obs = np.asarray(sums['n_obs'])
    for c, cam in enumerate(state.cams):
        if cam.refuses(n_obs[c]):
            raise ValueError('the passes did not see the same data (camera %d: %d observations, %d in the first pass)'
                             % (c, int(n_obs[c]), cam.n_obs))
    for c, cam in enumerate(state.cams):
        cam.step(sums['acc'][c], n_obs[c], c in state.hold, state.min_obs, *rule)
    cams = state.cams
    rep = {'status': np.array([c.status for c in cams], np.int32), 'passes': np.array([c.passes for c in cams], np.int32),
           'n_obs': n_obs.astype(np.int64), 'n_skipped': np.asarray(sums['n_skipped']).astype(np.int64),
           'cost_start': np.array([c.cost_start for c in cams]), 'cost': np.array([float(c.Aa[-1]) for c in cams]),
           'lambda': np.array([c.lam for c in cams])}
    for key in ('last_rot', 'last_trans') + tuple(more):
        rep[key] = np.array([getattr(c, key) for c in cams])
    rep.update(delta=np.array([c.delta for c in cams], np.float64), all_done=all(c.done for c in cams))
    return rep


# ---- bookkeeping of the script ----------------------------------------------------------------------------------------

def rotation_angle(Ra, Rb):
    """The angle of Ra Rb^T, radians."""
    M = np.asarray(Ra, np.float64) @ np.asarray(Rb, np.float64).T
    skew = 0.5 * np.array([M[2, 1] - M[1, 2], M[0, 2] - M[2, 0], M[1, 0] - M[0, 1]])
    return float(math.atan2(np.linalg.norm(skew), 0.5 * (np.trace(M) - 1.0)))


def extrinsics_distance(Ea, Eb):
    """-> (rotation angle in radians, norm of the translation difference in metres) between two 3 x 4 extrinsics."""
    Ea, Eb = np.asarray(Ea, np.float64).reshape(3, 4), np.asarray(Eb, np.float64).reshape(3, 4)
    return rotation_angle(Ea[:, :3], Eb[:, :3]), float(np.linalg.norm(Ea[:, 3] - Eb[:, 3]))


def perturbed(E, deg, mm, seed):
    """E [3,4] rotated by `deg` degrees about a seeded axis and shifted by `mm` millimetres in a seeded direction."""
    rng = np.random.default_rng(seed)
    axis, shift = rng.normal(size=3), rng.normal(size=3)
    axis, shift = axis / np.linalg.norm(axis), shift / np.linalg.norm(shift)
    return compose(E, list(axis * math.radians(deg)) + list(shift * (mm / 1000.0)))


def transform_manager_json(calib):
    """The document calibration.load_transform_manager reads: root -> camera of every camera of `calib`, hex floats."""
    return {'transforms': [{'from': 'root', 'to': cam, 'matrix': [[float(x).hex() for x in row] for row in calib.T_d[i]]}
                           for i, cam in enumerate(calib.names)]}


def build_own_parser():
    from .common import build_parser
    p = build_parser('Refine the camera extrinsics from the poses of a recording (alternating bundle adjustment)')
    p.add_argument('--rounds', type=int, default=3, help='match / triangulate / calibrate alternations')
    p.add_argument('--passes', type=int, default=8, help='passes and steps over the recording per round, at most')
    p.add_argument('--calib-huber', type=float, default=0.0, metavar='PX', help='Huber threshold of the calibration cost in pixels (0: plain least squares)')
    p.add_argument('--hold', type=str, nargs='*', default=None, metavar='NAME',
                   help='cameras that keep their extrinsics (default: the first camera; --hold with no name holds none)')
    p.add_argument('--min-obs', type=int, default=50, help='a camera with fewer observations is held')
    p.add_argument('--rot-tol', type=float, default=1e-7, metavar='RAD', help='a camera stops when its accepted step is below this rotation ...')
    p.add_argument('--trans-tol', type=float, default=1e-6, metavar='M', help='... and this translation')
    p.add_argument('--out', type=str, default=None, metavar='tm.json', help='write the refined calibration (the format --tmdir files are read in)')
    p.add_argument('--perturb-deg', type=float, default=0.0, help='--synthetic: the start has one camera rotated by this much')
    p.add_argument('--perturb-mm', type=float, default=0.0, help='--synthetic: ... and shifted by this much')
    p.add_argument('--perturb-camera', type=str, default=None, metavar='NAME', help='--synthetic: the camera that is moved (default: the last)')
    return p


def rig_calibration(args):
    """The calibration the run starts from: the rig's transform file under --tmdir when there is one (the name of
    parameters.transformations_path, .pickle or .json), else the one the package resolves."""
    import os

    from ..calibration import Calibration, load_transform_manager
    from ..parameters import parameters
    stem = os.path.splitext(os.path.basename(parameters.transformations_path or 'tm_panoptic.pickle'))[0]
    for ext in ('.pickle', '.json'):
        path = os.path.join(args.tmdir[0], stem + ext)
        if not args.synthetic and os.path.exists(path):
            return Calibration(parameters, load_transform_manager(path))
    return Calibration(parameters)


def rms_per_camera(eng, batches):
    """sqrt(mean squared residual) per camera over the kept batches (Engine.reproject rounds to float32, as the reference's
    script does) -> ([V] pixels, [V] counts)."""
    V = eng.V
    sq, n = np.zeros(V), np.zeros(V, np.int64)
    for db, persons, n_persons, poses, flags in batches:
        res = eng.reproject(db, persons, n_persons, poses, flags, 'triang')
        keep = res >= 0
        sq += (res.clamp(min=0.0) ** 2 * keep).sum(dim=(0, 1, 3)).cpu().numpy()
        n += keep.sum(dim=(0, 1, 3)).cpu().numpy()
    with np.errstate(all='ignore'):
        return np.sqrt(sq / n), n


def stages(eng, args, work):
    """Match, triangulate, (--regroup) regroup, (--merge, --found) consolidate and (--refine) refine every batch of `work`
    with `eng`; batches and poses stay on the device."""
    from .common import match_stage, repair_stage, report_consolidate, report_regroup, teacher_scores
    kept, regrouped, consolidated = [], [], []
    for at in range(0, len(work), args.batch):
        chunk = work[at:at + args.batch]
        frames = [{c: [f[c][0], f[c][1]] for c in f if json.loads(f[c][0])} for f, _, _ in chunk]
        db = eng.to_device(eng.pack(frames))
        if args.teacher_scores and chunk[0][2] is not None:
            persons, n_persons = eng.cluster(db, teacher_scores(db, [w[2] for w in chunk]))
        else:
            persons, n_persons = match_stage(eng, args, db)
        poses, flags = eng.triangulate(db, persons, n_persons, all_joints=True)
        persons, n_persons, poses, flags = repair_stage(eng, args, db, persons, n_persons, poses, flags, 'triang', regrouped, consolidated,
                                                        lambda rows, n: eng.triangulate(db, rows, n, all_joints=True))
        if args.refine:
            eng.refine(db, persons, n_persons, poses, flags, 'triang', max_iters=args.refine, huber_px=args.refine_huber, out=poses)
        kept.append((db, persons, n_persons, poses, flags))
    eng.sync_status()
    if args.regroup:
        report_regroup(args, regrouped)
    if args.merge or args.found:
        report_consolidate(args, consolidated)
    return kept


def script_work(args, true_calib, names):
    """What both scripts start from -> (work: collect_work's items, hold: the names of the held cameras)."""
    from .common import collect_work, held_cameras, load_frames
    if args.synthetic:
        work = collect_work(args, true_calib)           # synthetic frames are projected with the true calibration
    else:
        work = [(frame, None, None) for frame in load_frames(args)]      # the frame stride of the metrics scripts; no ground truth is read
    return work, held_cameras(args.hold, names)


def alternate(args, work, calib, make_fitter, tols, report):
    """The alternation: per round an engine from `calib`, the stages, up to --passes passes and steps of the object
    make_fitter(eng) gives (a Calibrator or a CameraFitter; `tols`: what its step() takes) over the kept batches, and the
    next `calib` from it; every round adds its entry to report['rounds'].  Then what the last `calib` gives on poses matched
    and triangulated with it.  -> (calib, RMS per camera before the first round, after the last, the observation counts)."""
    from ..lib import MpeError
    from ..parameters import parameters
    from ..pipeline import Engine
    from .common import max_skeletons_per_camera
    ppc = max(4, args.persons + 1, max_skeletons_per_camera(work))
    first_rms = None
    for rnd in range(max(1, args.rounds)):
        eng = Engine(parameters, calib, max_frames=args.batch, max_persons_per_camera=ppc)
        batches = stages(eng, args, work)
        before, _ = rms_per_camera(eng, batches)
        first_rms = before if first_rms is None else first_rms
        fit = make_fitter(eng)
        rep, passes = None, 0
        for _ in range(max(1, args.passes)):
            for b in batches:
                fit.accumulate(*b)
            try:
                rep = fit.step(*tols)
            except MpeError as err:                      # a trial that loses an observation (a joint behind the camera): keep what is accepted
                print('round %d stops after %d passes: %s' % (rnd + 1, passes, err))
                break
            passes += 1
            if rep['all_done']:
                break
        calib = fit.calibration()
        fit.close()
        eng.close()
        if rep is not None:
            report['rounds'].append({'passes': passes, 'rms_before': before.tolist(), 'cost_start': rep['cost_start'].tolist(),
                                     'cost': rep['cost'].tolist(), 'status': rep['status'].tolist(), 'n_obs': rep['n_obs'].tolist()})
            print('round %d: %d passes, cost %.6g -> %.6g px^2' % (rnd + 1, passes, float(np.sum(rep['cost_start'])), float(np.sum(rep['cost']))))
    eng = Engine(parameters, calib, max_frames=args.batch, max_persons_per_camera=ppc)
    last_rms, counts = rms_per_camera(eng, stages(eng, args, work))
    eng.close()
    return calib, first_rms, last_rms, counts


def run(args):
    from ..parameters import parameters
    true_calib = rig_calibration(args)
    names = list(parameters.used_cameras_skeleton_matching)
    calib = true_calib
    if args.synthetic and (args.perturb_deg or args.perturb_mm):
        moved = args.perturb_camera or names[-1]
        E = np.array(true_calib.P, np.float64)
        E[true_calib.index(moved)] = perturbed(E[true_calib.index(moved)], args.perturb_deg, args.perturb_mm, seed=2718)
        calib = true_calib.with_extrinsics(E)
    work, hold = script_work(args, true_calib, names)
    start = start_extrinsics(calib)
    report = {'cameras': names, 'hold': hold, 'rounds': []}
    calib, first_rms, last_rms, counts = alternate(
        args, work, calib, lambda eng: eng.calibrator('triang', huber_px=args.calib_huber, min_obs=args.min_obs, hold=hold),
        (args.rot_tol, args.trans_tol), report)
    final = start_extrinsics(calib)
    truth = start_extrinsics(true_calib)
    report.update(rms_before=first_rms.tolist(), rms_after=last_rms.tolist(), n_obs=counts.tolist(), rot_deg=[], trans_mm=[])
    if args.synthetic:
        report.update(true_rot_deg_before=[], true_trans_mm_before=[], true_rot_deg_after=[], true_trans_mm_after=[])
    for c, name in enumerate(names):
        rot, tr = extrinsics_distance(final[c], start[c])
        report['rot_deg'].append(math.degrees(rot))
        report['trans_mm'].append(tr * 1000.0)
        line = 'camera %s: %d observations, RMS %.4f -> %.4f px, rotated %.5f deg, moved %.4f mm%s' % (
            name, counts[c], first_rms[c], last_rms[c], math.degrees(rot), tr * 1000.0, ' (held)' if name in hold else '')
        if args.synthetic:
            r0, t0 = extrinsics_distance(start[c], truth[c])
            r1, t1 = extrinsics_distance(final[c], truth[c])
            for k, v in (('true_rot_deg_before', math.degrees(r0)), ('true_trans_mm_before', t0 * 1000.0),
                         ('true_rot_deg_after', math.degrees(r1)), ('true_trans_mm_after', t1 * 1000.0)):
                report[k].append(v)
            line += '; to the true extrinsics %.5f deg %.4f mm -> %.5f deg %.4f mm' % (math.degrees(r0), t0 * 1000.0, math.degrees(r1), t1 * 1000.0)
        print(line)
    if args.out:
        with open(args.out, 'w') as fh:
            json.dump(transform_manager_json(calib), fh, indent=1)
        print('wrote', args.out)
    report['calibration'] = calib
    return report


def main(argv=None):
    return run(build_own_parser().parse_args(argv))


if __name__ == '__main__':
    main()
