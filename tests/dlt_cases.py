"""Two-view DLT systems for the solver tests (test_dlt_solver_host.py, test_gpu_dlt_solver.py): the same seeded pairs on the CPU and
on the GPU, from the package's own calibrations, with numpy's SVD of the same matrices as the reference and the bounds both tests
hold the solver to.

Per calibration (PANOPTIC, ARPLAB) 2000 matched and 2000 mismatched pairs of distinct cameras:
  matched     one point inside the capture volume seen by both cameras, 0 / 0.1 / 1 / 4 px of image noise (500 pairs each)
  mismatched  the second view looks at the point displaced by N(0, 1 m) per axis (the pairs of two different persons), same noise
Bounds (X the solver's point, X_l LAPACK's, sigma the singular values of the system):
  matched                                    |X - X_l| <= 1e-10 m, a tenth of the 1e-9 m triangulation is held to against the reference
  mismatched, sigma4/sigma3 <= 0.5, |X| <= 10 m   |X - X_l| <= 1e-10 m * max(1, |X|); these must be >= 80 % of the mismatched pairs
  every mismatched pair                      |A (X,1)| / |(X,1)| <= sigma4 (1 + 1e-9) + 1e-15 sigma1: the point IS the right vector
"""
import numpy as np

from conftest import env, oracle, pkg

N_PER_CLASS = 2000
NOISE_PX = (0.0, 0.1, 1.0, 4.0)
MATCHED_BOUND = 1e-10
WELL_POSED_SHARE = 0.80
_cache = {}


class Systems:
    """cams (n,2) i32, pix (n,4) f64 pixel points (x1,y1,x2,y2), und (n,4) undistorted, A (n,4,4), mismatched (n,) bool,
    noise (n,) px; lapack (n,3), sigma (n,4) from numpy.linalg.svd."""

    def __init__(self, variant, seed):
        e = env(variant)
        calib, par = e.calib, e.params
        rng = np.random.default_rng(seed)
        V = calib.n_cameras
        syn = pkg('synthetic')
        W, H = par.image_width, par.image_height

        def view(cam, X, noise):
            uv, z = syn.project_panoptic(X.T, calib.K32[cam].astype(np.float64), calib.T_d[cam], calib.dist[cam])
            ok = (z > 0.1) & (uv[0] >= 0) & (uv[0] < W) & (uv[1] >= 0) & (uv[1] < H)
            return uv.T + noise[:, None] * rng.standard_normal((len(X), 2)), ok

        cams, pix, mism, noise = [], [], [], []
        for mismatched in (False, True):
            have = 0
            while have < N_PER_CLASS:
                n = 4 * N_PER_CLASS
                X = np.stack([rng.uniform(-1.4, 1.4, n), rng.uniform(-1.9, -0.1, n), rng.uniform(-1.4, 1.4, n)], axis=1)
                X2 = X + rng.standard_normal((n, 3)) if mismatched else X
                c1 = rng.integers(0, V, n)
                c2 = (c1 + rng.integers(1, V, n)) % V
                c1, c2 = np.minimum(c1, c2), np.maximum(c1, c2)
                nz = np.asarray(NOISE_PX)[np.arange(n) % len(NOISE_PX)]
                p = np.zeros((n, 4))
                ok = np.ones(n, bool)
                for c in range(V):
                    for col, sel, pts in ((0, c1 == c, X), (2, c2 == c, X2)):
                        uv, good = view(c, pts[sel], nz[sel])
                        p[sel, col:col + 2] = uv
                        ok[sel] &= good
                keep = np.flatnonzero(ok)
                # the same count of every noise level: the first N/4 of each that both cameras see
                take = np.concatenate([keep[nz[keep] == v][:N_PER_CLASS // len(NOISE_PX)] for v in NOISE_PX])
                assert len(take) == N_PER_CLASS, 'too few visible pairs'
                cams.append(np.stack([c1[take], c2[take]], axis=1))
                pix.append(p[take])
                mism.append(np.full(len(take), mismatched))
                noise.append(nz[take])
                have = len(take)
        self.variant = variant
        self.cams = np.concatenate(cams).astype(np.int32)
        self.pix = np.ascontiguousarray(np.concatenate(pix))
        self.mismatched = np.concatenate(mism)
        self.noise = np.concatenate(noise)
        n = len(self.cams)
        und = np.zeros((n, 4))
        for c in range(V):
            for col in (0, 1):
                sel = self.cams[:, col] == c
                und[sel, 2 * col:2 * col + 2] = oracle().undistort_points(self.pix[sel, 2 * col:2 * col + 2], calib.K32[c], calib.dist[c])
        self.und = und
        self.P1, self.P2 = calib.P[self.cams[:, 0]], calib.P[self.cams[:, 1]]
        self.A = np.stack([und[:, 0, None] * self.P1[:, 2] - self.P1[:, 0], und[:, 1, None] * self.P1[:, 2] - self.P1[:, 1],
                           und[:, 2, None] * self.P2[:, 2] - self.P2[:, 0], und[:, 3, None] * self.P2[:, 2] - self.P2[:, 1]], axis=1)
        _, self.sigma, vh = np.linalg.svd(self.A)
        self.lapack = vh[:, 3, :3] / vh[:, 3, 3:4]

    def host_input(self):
        """n x 28 f64 for tests/native/dlt_solve_host.cpp."""
        return np.ascontiguousarray(np.concatenate([self.P1.reshape(-1, 12), self.P2.reshape(-1, 12), self.und], axis=1))


def systems(variant):
    if variant not in _cache:
        _cache[variant] = Systems(variant, {'panoptic': 20260, 'arplab': 20261}[variant])
    return _cache[variant]


def check(s, X, label):
    """The three bounds of the module docstring on the solver's points X (n,3) for the systems s; prints each figure first."""
    X = np.asarray(X, np.float64)
    assert X.shape == s.lapack.shape and np.isfinite(X[~s.mismatched]).all()
    dist = np.linalg.norm(X - s.lapack, axis=1)
    m = ~s.mismatched
    print('%s %s matched: n %d, max |X - X_lapack| %.3g m (noise-free %.3g m)' % (label, s.variant, m.sum(), dist[m].max(), dist[m & (s.noise == 0)].max()))
    assert m.sum() == N_PER_CLASS and (m & (s.noise == 0)).sum() == N_PER_CLASS // len(NOISE_PX)
    assert dist[m].max() <= MATCHED_BOUND
    mm = s.mismatched
    size = np.linalg.norm(s.lapack, axis=1)
    well = mm & (s.sigma[:, 3] <= 0.5 * s.sigma[:, 2]) & (size <= 10.0)
    rel = dist[well] / np.maximum(1.0, size[well])
    print('%s %s mismatched: n %d, well posed %.1f %%, max |X - X_lapack| / max(1, |X|) %.3g m' % (label, s.variant, mm.sum(), 100.0 * well.sum() / mm.sum(), rel.max()))
    assert mm.sum() == N_PER_CLASS and well.sum() >= WELL_POSED_SHARE * mm.sum()
    assert rel.max() <= MATCHED_BOUND
    Xh = np.concatenate([X, np.ones((len(X), 1))], axis=1)
    res = np.linalg.norm(np.einsum('nij,nj->ni', s.A, Xh), axis=1) / np.linalg.norm(Xh, axis=1)
    bound = s.sigma[:, 3] * (1 + 1e-9) + 1e-15 * s.sigma[:, 0]
    print('%s %s mismatched: max residual / bound %.6f' % (label, s.variant, (res[mm] / bound[mm]).max()))
    assert np.isfinite(res[mm]).all() and (res[mm] <= bound[mm]).all()
