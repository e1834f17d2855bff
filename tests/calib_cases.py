"""Inputs for the calibration tests (test_calib_host.py: harness/calibrate.py and csrc/calib_solve.h on their own;
test_gpu_calib.py: mpe_calib_* against them).  Scenes are bodies of the frame generator projected into a rig; persons come
from the generator's pairing, so neither file needs a matcher.  Everything is seeded.  Not a test module."""
import copy
import json
import math

import numpy as np

from conftest import env, oracle, pkg
from refine_cases import same_bits  # noqa: F401  (the tests take it from here)

J = 18
ALL_JOINTS = (1 << J) - 1


def CB():
    return pkg('harness.calibrate')


def bodies_of(calib, n_frames, n_bodies, seed=4100):
    syn = pkg('synthetic')
    counts = n_bodies if isinstance(n_bodies, (list, tuple)) else [n_bodies] * n_frames
    return [syn.make_frame(calib, i, syn.FrameSpec(persons=n), seed=seed)[1]['persons'] for i, n in enumerate(counts)]


class Scene:
    """One batch of a rig (`variant`: a fixture variant of conftest.env) with its persons and the true bodies as float64
    poses with joint flags.  exact: the detections are harness.calibrate.project_camera of the bodies under the rig's own
    extrinsics, to the last bit (zero residual at the truth); noise_px: seeded normal noise on top.  damage(frames,
    owners): edits the wire frames before they are packed."""

    def __init__(self, variant, n_frames, n_bodies, seed=4100, exact=True, noise_px=0.0, pcap=None, damage=None):
        syn, onp = pkg('synthetic'), oracle()
        self.variant, self.env = variant, env(variant)
        self.calib = calib = self.env.calib
        self.names = list(calib.params.used_cameras_skeleton_matching)
        self.bodies = bodies_of(calib, n_frames, n_bodies, seed)
        made = [syn.frame_from_bodies(calib, i, b) for i, b in enumerate(self.bodies)]
        self.frames, self.owners = [m[0] for m in made], [m[1] for m in made]
        if damage is not None:
            damage(self.frames, self.owners)
        self.processed = [onp.processed_input(f) for f in self.frames]
        self.pb = pkg('packing').pack_frames(self.processed, calib.params, keep_json=True)
        most = max(len(b) for b in self.bodies)
        self.pcap = pcap if pcap is not None else most + 1
        F = n_frames
        self.persons = np.full((F, self.pcap, self.pb.V), -1, np.int32)
        for f in range(F):
            h0, H, _, _ = self.pb.frame_counts(f)
            for i in range(H):
                c = int(self.pb.head_cam[h0 + i])
                o = self.owners[f][self.names[c]][int(self.pb.skeleton_index[h0 + i])]
                self.persons[f, o, c] = i
        self.n_persons = np.array([len(b) for b in self.bodies], np.int32)
        self.truth = np.zeros((F, self.pcap, J, 3))
        for f, b in enumerate(self.bodies):
            self.truth[f, :len(b)] = b
        self.flags = np.repeat((np.arange(self.pcap)[None, :] < self.n_persons[:, None])[..., None], J, axis=2).astype(np.uint8)
        self.E_true = CB().start_extrinsics(calib)
        if exact:
            self.pb = self.with_detections(noise_px, seed + 1)

    def with_detections(self, noise_px, seed):
        """A copy of the batch whose detections are the rule's own projection of the bodies (+ seeded noise)."""
        _, kd, K = pkg('harness.refine').camera_constants64(self.calib)            # by camera slot, as E_true is
        rng = np.random.default_rng(seed)
        pb = copy.copy(self.pb)
        pb.xy = np.array(self.pb.xy, np.float64, copy=True)
        for f in range(pb.n_frames):
            h0, H, _, _ = pb.frame_counts(f)
            for i in range(H):
                c = int(pb.head_cam[h0 + i])
                o = self.owners[f][self.names[c]][int(pb.skeleton_index[h0 + i])]
                X = self.truth[f, o]
                p = CB().project_camera(self.E_true[c], kd[c], K[c], X[:, 0], X[:, 1], X[:, 2])
                noise = noise_px * rng.normal(size=(J, 2)) if noise_px else np.zeros((J, 2))
                pb.xy[h0 + i, :, 0], pb.xy[h0 + i, :, 1] = p['px'] + noise[:, 0], p['py'] + noise[:, 1]
        return pb

    def one_pass(self, E, sums=None, frames=None, poses=None, flags=None, mask=ALL_JOINTS, huber_px=0.0, pb=None, pass_host=None):
        """calib_pass_host at the extrinsics E (or pass_host -- camfit_pass_host -- at the trial set E) over the scene, or
        over the frames [a, b) of it packed on their own."""
        poses = self.truth if poses is None else poses
        flags = self.flags if flags is None else flags
        pb = self.pb if pb is None else pb
        sl = slice(None)
        if frames is not None:
            a, b = frames
            pb, sl = self.sub_batch(a, b), slice(a, b)
        if pass_host is None:
            return CB().calib_pass_host(self.calib, E, pb, self.persons[sl], self.n_persons[sl], poses[sl], flags[sl], mask, huber_px=huber_px, sums=sums)
        return pass_host(E, pb, self.persons[sl], self.n_persons[sl], poses[sl], flags[sl], mask, huber_px=huber_px, sums=sums)

    def sub_batch(self, a, b):
        """Frames [a, b) packed on their own, with this scene's detections."""
        sub = pkg('packing').pack_frames(self.processed[a:b], self.calib.params, keep_json=True)
        h0, h1 = int(self.pb.frame_head_off[a]), int(self.pb.frame_head_off[b])
        sub = copy.copy(sub)
        sub.xy = np.array(np.asarray(self.pb.xy, np.float64).reshape(-1, J, 2)[h0:h1], copy=True).reshape(np.asarray(sub.xy).shape)
        return sub


def perturbed_start(E, deg, mm, seed):
    """Every camera of E [V,3,4] rotated by `deg` degrees about a seeded axis and shifted by `mm` millimetres."""
    return np.stack([CB().perturbed(E[c], deg, mm, seed + c) for c in range(len(E))])


def run_host(scene, E0, passes, rot_tol, trans_tol, hold=(), min_obs=6, huber_px=0.0, until_done=True, **pass_kw):
    """Passes and steps of the statement -> (HostCalibrator, the reports in order)."""
    state = CB().HostCalibrator(E0, hold=hold, min_obs=min_obs)
    reports = []
    for _ in range(passes):
        sums = scene.one_pass(state.trial(), huber_px=huber_px, **pass_kw)
        reports.append(CB().calib_step_host(state, sums, rot_tol, trans_tol))
        if until_done and reports[-1]['all_done']:
            break
    return state, reports


def camera_residuals(scene, c):
    """-> fn(xi, E0): the residual vector (rx and ry of every observation of camera c) with the camera at compose(E0, xi):
    what scipy's optimiser is given, on the same observations from the same start."""
    calib = scene.calib
    sel, xy = pkg('harness.reprojection').selection(scene.pb, scene.persons, scene.n_persons, scene.flags, ALL_JOINTS)
    _, kd, K = pkg('harness.refine').camera_constants64(calib)
    pick = sel[:, :, c]
    X = scene.truth[pick]
    obs = xy[:, :, c][pick]

    def fn(xi, E0):
        p = CB().project_camera(CB().compose(E0, xi), kd[c], K[c], X[:, 0], X[:, 1], X[:, 2])
        return np.concatenate([p['px'] - obs[:, 0], p['py'] - obs[:, 1]])
    return fn


def scipy_fit(scene, c, E0):
    """scipy's Levenberg-Marquardt on camera c from E0 -> (E [3,4], cost = sum of squared residuals)."""
    from scipy.optimize import least_squares
    fn = camera_residuals(scene, c)
    sol = least_squares(lambda xi: fn(xi, E0), np.zeros(6), method='lm', ftol=1e-15, xtol=1e-15, gtol=1e-15, max_nfev=2000)
    return CB().compose(E0, sol.x), float(np.sum(sol.fun ** 2))


def systems(n=24, seed=515):
    """Seeded 6 x 6 systems for the solver: (A [21], g [6], lambda, Ea [12]) -- Gram matrices of a few rows with the scales
    a camera's normal equations have (rotation columns ~ f * depth, translation columns ~ f / depth), some of them
    indefinite (a pivot that is not > 0 until lambda has grown, or never within the retries), some all zero (the retry cap)."""
    rng = np.random.default_rng(seed)
    tri = CB().TRI
    out = []
    for i in range(n):
        rows = 40 if i % 8 else 0                            # i % 8 == 0: no rows at all
        Jm = rng.normal(size=(rows, 6)) * np.array([3000., 3000., 3000., 400., 400., 400.])
        r = rng.normal(size=rows) * 3.0
        A, g = Jm.T @ Jm, Jm.T @ r
        if i % 8 == 4 or i % 8 == 2:                         # indefinite until lambda > 0.02
            A[0, 1] = A[1, 0] = 1.02 * math.sqrt(A[0, 0] * A[1, 1])
        w = rng.normal(size=3)
        Ea = CB().compose(np.hstack([np.eye(3), rng.normal(size=(3, 1))]), list(w / np.linalg.norm(w) * rng.uniform(0, 3)) + [0., 0., 0.])
        out.append((np.array([A[k, l] for k, l in tri]), g, [1e-3, 1e-12, 10.0][i % 3], Ea.reshape(12)))
    return out


def host_trial(A, g, lam, Ea):
    """The statement's calib_cam_trial on one system -> (delta or None, lambda after, E_t [12], stalled)."""
    cam = CB().CameraState(np.asarray(Ea).reshape(3, 4))
    cam.Aa = np.concatenate([A, g, [0.0]])
    cam.lam = lam
    cam.trial()
    stalled = bool(cam.status & CB().STALLED)
    return (None if stalled else list(cam.delta)), cam.lam, cam.Et.reshape(12), stalled


# ---- the small device cases --------------------------------------------------------------------------------------------

def small_damage(frames, owners, used=None):
    """Frame 0: person 1 loses its skeleton in the third camera (of two used cameras: the first); frame 1: a joint removed
    from a skeleton; frame 2: a confidence below the threshold and one exactly at it.  used: the cameras the rig's engine
    takes (default: every stream of the frame)."""
    cams = list(frames[0]) if used is None else list(used)
    cam = cams[2 % len(cams)]
    i = owners[0][cam].index(1)
    sks = json.loads(frames[0][cam][0])
    del sks[i]
    del owners[0][cam][i]
    frames[0][cam][0] = json.dumps(sks)
    sks = json.loads(frames[1][cams[0]][0])
    assert '7' in sks[0] and '4' in json.loads(frames[2][cams[1]][0])[1] and '9' in json.loads(frames[2][cams[1]][0])[0]
    del sks[0]['7']
    frames[1][cams[0]][0] = json.dumps(sks)
    sks = json.loads(frames[2][cams[1]][0])
    sks[1]['4'][3] = 0.25
    sks[0]['9'][3] = 0.5
    frames[2][cams[1]][0] = json.dumps(sks)


def small(variant='panoptic', n_frames=3, n_bodies=2, pcap=None, seed=4300):
    """n_frames of the rig x n_bodies persons with the damage above, 1 px of noise, and both kinds of poses: 'triang' the
    bodies moved by a few millimetres (float64, joint flags, one of them off, all joints) and 'est' (float32, person
    flags, one of them off, the used joints)."""
    used = list(env(variant).params.used_cameras_skeleton_matching)
    s = Scene(variant, n_frames, n_bodies, seed=seed, noise_px=1.0, pcap=pcap,
              damage=(lambda frames, owners: small_damage(frames, owners, used)) if n_frames >= 3 and n_bodies >= 2 else None)
    rng = np.random.default_rng(seed + 7)
    tri = s.truth + rng.uniform(-0.004, 0.004, s.truth.shape)
    jf = s.flags.copy()
    jf[0, 0, 5] = 0
    est = (s.truth + rng.uniform(-0.01, 0.01, s.truth.shape)).astype(np.float32)
    pf = (np.arange(s.pcap)[None, :] < s.n_persons[:, None]).astype(np.uint8)
    if n_frames > 1:
        pf[1, 0] = 0
    used = sum(1 << j for j in s.calib.params.used_joints)
    s.kinds = {'triang': (tri, jf, ALL_JOINTS), 'est': (est, pf, used)}
    return s
