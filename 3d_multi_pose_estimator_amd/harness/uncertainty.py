"""numpy statement of what mpe_posecov_batch computes (csrc/posecov.hip, csrc/cov3.h): the 3 x 3 covariance of every joint
of every pose from the cameras that saw it, Sigma = sigma_px^2 * A^-1 with A the normal matrix the refinement builds at
that point.  The GPU tests hold the kernel to this module bit for bit.  include/mpe.h words the rule; the lines below are
its lines.

This is the Gauss-Newton approximation of the covariance of the per-frame estimate: exact for a linear model with
independent pixel noise of standard deviation sigma_px in x and in y, and the usual weighted approximation (not the
sandwich estimator) with a Huber weight.  It is untimed (camera lags are ignored, as in the DLT) and says nothing about what
smoothing or a bone-length fit do to the pose afterwards.

All arithmetic is float64, every operation rounded on its own.  Observing cameras, x, y, the projection, the Jacobian and
the weight are harness/refine.py's.  Vectorised over the joints of the batch; a Python loop over the cameras.
"""
import numpy as np

from . import refine as RF
from . import reprojection as R

COMPUTED, FEW_VIEWS, BAD_POSE, SINGULAR, GATED = 1, 8, 16, 32, 64
ORDER = RF.PAIRS                                 # cov [..., 6]: (00, 01, 02, 11, 12, 22)


def inverse3(A):
    """A {(k, l): array} over refine.PAIRS -> (S likewise: the inverse by the LDL^T lines of refine.lm_step3 without
    damping, ok: every pivot > 0).  csrc/cov3.h has the same lines."""
    with np.errstate(all='ignore'):
        D0 = A[0, 0]
        L10 = A[0, 1] / D0
        L20 = A[0, 2] / D0
        D1 = A[1, 1] - L10 * A[0, 1]
        t = A[1, 2] - L20 * A[0, 1]
        L21 = t / D1
        D2 = (A[2, 2] - L20 * A[0, 2]) - L21 * t
        i0, i1, i2 = 1.0 / D0, 1.0 / D1, 1.0 / D2
        m = L10 * L21 - L20
        S22 = i2
        S12 = -L21 * i2
        S02 = m * i2
        S11 = i1 - L21 * S12
        S01 = (-L10) * i1 + m * S12
        S00 = (i0 + (L10 * L10) * i1) + m * S02
        return {(0, 0): S00, (0, 1): S01, (0, 2): S02, (1, 1): S11, (1, 2): S12, (2, 2): S22}, (D0 > 0.0) & (D1 > 0.0) & (D2 > 0.0)


def finish(S, s2):
    """S from inverse3, s2 = sigma_px * sigma_px -> (cov [..., 6] in ORDER, sigma, ok: every entry of both finite)."""
    with np.errstate(all='ignore'):
        cov = np.stack([s2 * S[kl] for kl in ORDER], axis=-1)
        sigma = np.sqrt((cov[..., 0] + cov[..., 3]) + cov[..., 5])
        return cov, sigma, np.isfinite(cov).all(axis=-1) & np.isfinite(sigma)


def normal_matrix(cams, X, xy, obs, huber):
    """A {(k, l): [N]} at the points X [N,3]: the fold of refine.refine's iteration over the observing cameras in increasing c,
    and front [N]: pc_2 > 0 in every observing camera."""
    N = X.shape[0]
    A = {kl: np.zeros(N) for kl in RF.PAIRS}
    front = np.ones(N, bool)
    with np.errstate(all='ignore'):
        for c, (T, kd, K) in enumerate(cams):
            p = RF.project64(T, kd, K, X[:, 0], X[:, 1], X[:, 2], jacobian=True)
            rx = p['px'] - xy[:, c, 0]
            ry = p['py'] - xy[:, c, 1]
            w = RF.huber_weight(np.sqrt(rx * rx + ry * ry), huber)
            jx, jy = p['jx'], p['jy']
            for (k, l) in A:
                A[k, l] = np.where(obs[:, c], A[k, l] + w * (jx[k] * jx[l] + jy[k] * jy[l]), A[k, l])
            front &= ~obs[:, c] | (p['pc2'] > 0.0)
    return A, front


def pose_covariance(calib, pb, persons, n_persons, poses, flags, joint_mask, sigma_px, threshold=0.5, huber_px=0.0, gate_m=0.0,
                    flags_out=False, diagnostics=False):
    """pb, persons, n_persons, poses, flags, joint_mask, threshold: as refine.refine takes them.  -> {'cov' f64 [F,Pcap,J,6],
    'sigma' f64 (metres; -1 where not computed), 'status' u8, 'n_views' u8}, the last three [F,Pcap,J]; with flags_out
    (joint flags only) 'flags': the input flags with the GATED joints cleared; with diagnostics 'A' [F,Pcap,J,6], the normal
    matrix in ORDER."""
    if not (sigma_px > 0.0 and np.isfinite(sigma_px)) or not gate_m >= 0.0 or not huber_px >= 0.0:
        raise ValueError('sigma_px > 0 and finite, gate_m >= 0 and huber_px >= 0')
    poses = np.asarray(poses)
    if poses.dtype not in (np.float32, np.float64):
        raise ValueError('poses must be float32 or float64')
    flags = np.asarray(flags)
    F, Pcap, V = np.asarray(persons).shape
    J = pb.J
    if flags_out and flags.ndim != 3:
        raise ValueError('flags_out needs joint flags [F,Pcap,J]')
    huber, s2 = float(huber_px), np.float64(sigma_px) * np.float64(sigma_px)
    sel, xy = R.selection(pb, persons, n_persons, flags, joint_mask, threshold)
    obs = np.ascontiguousarray(np.moveaxis(sel, 2, 3)).reshape(-1, V)                 # [N, V], N = F * Pcap * J
    xy = np.ascontiguousarray(np.moveaxis(xy, 2, 3)).reshape(-1, V, 2)
    X = poses.reshape(-1, 3).astype(np.float64)
    N = X.shape[0]
    cams = list(zip(*RF.camera_constants64(calib)))
    views = obs.sum(axis=1)
    many = views >= 2
    A, front = normal_matrix(cams, X, xy, obs & many[:, None], huber)
    good = many & np.isfinite(X).all(axis=1) & front
    S, pivots = inverse3(A)
    cov, sigma, finite = finish(S, s2)
    computed = good & pivots & finite
    status = np.zeros(N, np.uint8)
    status[views == 1] = FEW_VIEWS
    status[many & ~good] = BAD_POSE
    status[good & ~computed] = SINGULAR
    status[computed] = COMPUTED
    with np.errstate(all='ignore'):
        gated = computed & (sigma > gate_m) if gate_m > 0.0 else np.zeros(N, bool)
    status[gated] |= GATED
    shape = (F, Pcap, J)
    out = {'cov': np.where(computed[:, None], cov, 0.0).reshape(shape + (6,)), 'sigma': np.where(computed, sigma, -1.0).reshape(shape),
           'status': status.reshape(shape), 'n_views': views.astype(np.uint8).reshape(shape)}
    if flags_out:
        out['flags'] = np.where(gated.reshape(shape), 0, flags).astype(flags.dtype)
    if diagnostics:
        out['A'] = np.stack([A[kl] for kl in ORDER], axis=-1).reshape(shape + (6,))
    return out


def full(c6):
    """[..., 6] in ORDER -> the symmetric matrices [..., 3, 3]"""
    c6 = np.asarray(c6)
    return np.stack([c6[..., [0, 1, 2]], c6[..., [1, 3, 4]], c6[..., [2, 4, 5]]], axis=-2)


def pixel_sigma(refine_outs):
    """Engine.refine's (or refine.refine's) outputs of one or more batches, run with huber_px = 0 -> (the pooled pixel noise
    sqrt(sum cost1 / sum (2 n_views - 3)) over the SOLVED joints: every view gives two residuals and the joint takes three
    degrees of freedom; NaN without any, the degrees of freedom)."""
    cost, dof = 0.0, 0
    for o in refine_outs:
        s = (np.asarray(o['status']) & RF.SOLVED) != 0
        cost += float(np.asarray(o['cost1'], np.float64)[s].sum())
        dof += int((2 * np.asarray(o['n_views'], np.int64)[s] - 3).sum())
    return (float(np.sqrt(cost / dof)) if dof > 0 else float('nan')), dof


def summary(outs):
    """Engine.pose_covariance's (or pose_covariance's) outputs of one or more batches, as host arrays -> {'computed',
    'median_mm', 'p95_mm', 'max_mm', 'gated'} (the extra line of the metrics scripts)."""
    sig = [np.asarray(o['sigma'])[(np.asarray(o['status']) & COMPUTED) != 0] for o in outs]
    sig = np.concatenate([s.reshape(-1) for s in sig]) if sig else np.zeros(0)
    gated = sum(int(((np.asarray(o['status']) & GATED) != 0).sum()) for o in outs)
    nan = float('nan')
    return {'computed': int(sig.size), 'median_mm': 1000.0 * float(np.median(sig)) if sig.size else nan,
            'p95_mm': 1000.0 * float(np.percentile(sig, 95)) if sig.size else nan, 'max_mm': 1000.0 * float(sig.max()) if sig.size else nan,
            'gated': gated}


def report_line(sigma_px, gate_mm, r, pooled=None):
    line = 'Uncertainty (sigma %g px): %d joints computed, sigma median %.3f mm, 95 %% %.3f mm, max %.3f mm' % (
        sigma_px, r['computed'], r['median_mm'], r['p95_mm'], r['max_mm'])
    if gate_mm:
        line += ', %d gated above %g mm' % (r['gated'], gate_mm)
    if pooled is not None:
        line += '; pooled pixel sigma of the recording %.4g px' % pooled
    return line
