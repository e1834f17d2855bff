"""numpy statement of what mpe_refine_batch computes (csrc/refine.hip): every joint of every pose moved to the minimum of
its reprojection cost over the cameras that saw it, one Levenberg-Marquardt problem of three unknowns per joint.  The GPU
tests hold the kernel to this module bit for bit.  include/mpe.h words the rule; the lines below are its lines.

All arithmetic is float64, every operation rounded on its own (numpy fuses nothing), in the header's order.  The
observing cameras of a joint are the entries harness/reprojection.py counts (`selection`).  Vectorised over the joints of
the batch; Python loops over the iterations and the cameras.
"""
import numpy as np

from . import reprojection as R

SOLVED, MOVED, CONVERGED, FEW_VIEWS, BAD_START = 1, 2, 4, 8, 16
MAX_ITERS = 64


def camera_constants64(calib):
    """-> (T [V,3,4], kd [V,3], K [V,3,3]) float64, by camera slot (reprojection.engine_calibration): P and the radial
    terms as stored, the float32 K widened."""
    P, dist, K32 = R.engine_calibration(calib)
    return P, np.ascontiguousarray(dist[:, [0, 1, 4]]), K32.astype(np.float64)


def project64(T, kd, K, X0, X1, X2, jacobian=False):
    """One camera (T [3,4], kd [3], K [3,3], float64), points X0 / X1 / X2 [...] float64 -> a dict with px, py, pc2 (and
    the lines between: pc, h0, h1, r, f, u2) and, with jacobian, jx / jy (lists of three arrays: the derivatives by X0, X1,
    X2).  The header's projection lines; csrc/project64.h has the same ones for the kernels."""
    with np.errstate(all='ignore'):
        pc = [((T[i, 0] * X0 + T[i, 1] * X1) + T[i, 2] * X2) + T[i, 3] for i in range(3)]
        h0 = pc[0] / pc[2]
        h1 = pc[1] / pc[2]
        r = h0 * h0 + h1 * h1
        f = ((1.0 + kd[0] * r) + (kd[1] * r) * r) + ((kd[2] * r) * r) * r
        d0 = h0 * f
        d1 = h1 * f
        u = [(K[i, 0] * d0 + K[i, 1] * d1) + K[i, 2] for i in range(3)]
        px = u[0] / u[2]
        py = u[1] / u[2]
        out = {'px': px, 'py': py, 'pc2': pc[2], 'pc': pc, 'h0': h0, 'h1': h1, 'r': r, 'f': f, 'u2': u[2]}
        if jacobian:
            fd = radial_slope(kd, r)
            rows = [jacobian_tail(out, K, fd, (T[0, k] - h0 * T[2, k]) / pc[2], (T[1, k] - h1 * T[2, k]) / pc[2]) for k in range(3)]
            out['jx'], out['jy'] = [x for x, _ in rows], [y for _, y in rows]
    return out


def radial_slope(kd, r):
    """d f / d r of the lens model"""
    return (kd[0] + (2.0 * kd[1]) * r) + ((3.0 * kd[2]) * r) * r


def jacobian_tail(p, K, fd, a, b):
    """The tail of every Jacobian of (px, py).  p: project64's dict; (a, b): the derivative of (h0, h1) by one unknown;
    fd = radial_slope -> (the derivative of px, of py) by that unknown."""
    with np.errstate(all='ignore'):
        q = fd * (2.0 * (p['h0'] * a + p['h1'] * b))
        m = a * p['f'] + p['h0'] * q
        n = b * p['f'] + p['h1'] * q
        v = [K[i, 0] * m + K[i, 1] * n for i in range(3)]
        return (v[0] - p['px'] * v[2]) / p['u2'], (v[1] - p['py'] * v[2]) / p['u2']


def _rho(e, huber):
    with np.errstate(all='ignore'):
        if huber <= 0.0:
            return e * e
        return np.where(e <= huber, e * e, (2.0 * huber) * e - huber * huber)


def huber_weight(e, huber):
    """the weight of a residual of length e in the normal equations; huber <= 0: 1"""
    with np.errstate(all='ignore'):
        return np.ones_like(e) if huber <= 0.0 else np.where(e <= huber, 1.0, huber / e)


PAIRS = ((0, 0), (0, 1), (0, 2), (1, 1), (1, 2), (2, 2))          # the six entries of a symmetric 3 x 3 A, as the dicts below key them


def lm_step3(A, g, lam):
    """A {(k, l): array} over PAIRS, g [3] arrays, lam: (A + lam diag A) delta = -g, LDL^T written out -> (delta [..., 3],
    ok: every pivot positive and delta finite)."""
    with np.errstate(all='ignore'):
        M00, M11, M22 = (A[k, k] + lam * A[k, k] for k in range(3))
        D0 = M00
        L10 = A[0, 1] / D0
        L20 = A[0, 2] / D0
        D1 = M11 - L10 * A[0, 1]
        t = A[1, 2] - L20 * A[0, 1]
        L21 = t / D1
        D2 = (M22 - L20 * A[0, 2]) - L21 * t
        z0 = -g[0]
        z1 = -g[1] - L10 * z0
        z2 = (-g[2] - L20 * z0) - L21 * z1
        e2 = z2 / D2
        e1 = z1 / D1 - L21 * e2
        e0 = (z0 / D0 - L10 * e1) - L20 * e2
        delta = np.stack([e0, e1, e2], axis=-1)
        return delta, (D0 > 0.0) & (D1 > 0.0) & (D2 > 0.0) & np.isfinite(delta).all(axis=-1)


def _cost(cams, X, xy, obs, huber):
    """-> (C [N], every observing camera has pc2 > 0 [N])."""
    C = np.zeros(X.shape[0])
    front = np.ones(X.shape[0], bool)
    with np.errstate(all='ignore'):
        for c, (T, kd, K) in enumerate(cams):
            p = project64(T, kd, K, X[:, 0], X[:, 1], X[:, 2])
            rx = p['px'] - xy[:, c, 0]
            ry = p['py'] - xy[:, c, 1]
            C = np.where(obs[:, c], C + _rho(np.sqrt(rx * rx + ry * ry), huber), C)
            front &= ~obs[:, c] | (p['pc2'] > 0.0)
    return C, front


def refine(calib, pb, persons, n_persons, poses, flags, joint_mask, threshold=0.5, max_iters=10, step_tol=1e-6, huber_px=0.0):
    """pb, persons, n_persons, poses, flags, joint_mask, threshold: as reprojection.residuals takes them (poses float32 or
    float64 [F,Pcap,J,3]).  -> {'poses' (the type of the input), 'status' u8, 'cost0', 'cost1' f64, 'iters' u8,
    'n_views' u8}, the last five [F,Pcap,J]."""
    if not 1 <= int(max_iters) <= MAX_ITERS or not step_tol >= 0.0 or not huber_px >= 0.0:
        raise ValueError('max_iters in 1..%d, step_tol >= 0 and huber_px >= 0' % MAX_ITERS)
    poses = np.asarray(poses)
    if poses.dtype not in (np.float32, np.float64):
        raise ValueError('poses must be float32 or float64')
    huber, step_tol = float(huber_px), float(step_tol)
    F, Pcap, V = np.asarray(persons).shape
    J = pb.J
    sel, xy = R.selection(pb, persons, n_persons, flags, joint_mask, threshold)
    obs = np.ascontiguousarray(np.moveaxis(sel, 2, 3)).reshape(-1, V)                 # [N, V], N = F * Pcap * J
    xy = np.ascontiguousarray(np.moveaxis(xy, 2, 3)).reshape(-1, V, 2)
    start = poses.reshape(-1, 3)
    N = start.shape[0]
    cams = list(zip(*camera_constants64(calib)))
    views = obs.sum(axis=1)
    status = np.zeros(N, np.uint8)
    status[views == 1] = FEW_VIEWS
    X = start.astype(np.float64)
    many = views >= 2
    C, front = _cost(cams, X, xy, obs & many[:, None], huber)
    solved = many & np.isfinite(X).all(axis=1) & front
    status[many & ~solved] = BAD_START
    status[solved] = SOLVED
    obs = obs & solved[:, None]
    C = np.where(solved, C, 0.0)
    cost0 = C.copy()
    active = solved.copy()
    lam = np.full(N, 1e-3)
    iters = np.zeros(N, np.uint8)
    with np.errstate(all='ignore'):
        for _ in range(int(max_iters)):
            if not active.any():
                break
            A = {kl: np.zeros(N) for kl in PAIRS}
            g = [np.zeros(N) for _ in range(3)]
            for c, (T, kd, K) in enumerate(cams):
                p = project64(T, kd, K, X[:, 0], X[:, 1], X[:, 2], jacobian=True)
                rx = p['px'] - xy[:, c, 0]
                ry = p['py'] - xy[:, c, 1]
                e = np.sqrt(rx * rx + ry * ry)
                w = huber_weight(e, huber)
                jx, jy = p['jx'], p['jy']
                for (k, l) in A:
                    A[k, l] = np.where(obs[:, c], A[k, l] + w * (jx[k] * jx[l] + jy[k] * jy[l]), A[k, l])
                for k in range(3):
                    g[k] = np.where(obs[:, c], g[k] + w * (jx[k] * rx + jy[k] * ry), g[k])
            delta, ok = lm_step3(A, g, lam)
            ok = active & ok
            Y = X + delta
            Ct, front = _cost(cams, Y, xy, obs, huber)
            accept = ok & front & (Ct < C)
            iters[active] += 1
            reject = active & ~accept
            X = np.where(accept[:, None], Y, X)
            C = np.where(accept, Ct, C)
            status[accept] |= MOVED
            lam = np.where(accept, np.maximum(lam / 10.0, 1e-12), np.where(reject, lam * 10.0, lam))
            done = accept & (np.abs(delta).max(axis=1) < step_tol)
            status[done] |= CONVERGED
            active = active & ~done
    moved = (status & MOVED) != 0
    out = np.where(moved[:, None], X.astype(poses.dtype), start)
    shape = (F, Pcap, J)
    return {'poses': out.reshape(poses.shape), 'status': status.reshape(shape), 'cost0': np.where(solved, cost0, -1.0).reshape(shape),
            'cost1': np.where(solved, C, -1.0).reshape(shape), 'iters': iters.reshape(shape), 'n_views': views.astype(np.uint8).reshape(shape)}


def summary(outs):
    """Engine.refine's (or refine's) outputs of one or more batches, as host arrays -> {'solved', 'moved_share',
    'mean_cost0', 'mean_cost1'} over all solved joints (the extra line of the metrics scripts)."""
    n = moved = 0
    c0 = c1 = 0.0
    for o in outs:
        s = (np.asarray(o['status']) & SOLVED) != 0
        n += int(s.sum())
        moved += int(((np.asarray(o['status']) & MOVED) != 0).sum())
        c0 += float(np.asarray(o['cost0'])[s].sum())
        c1 += float(np.asarray(o['cost1'])[s].sum())
    return {'solved': n, 'moved_share': moved / n if n else 0.0, 'mean_cost0': c0 / n if n else float('nan'),
            'mean_cost1': c1 / n if n else float('nan')}
