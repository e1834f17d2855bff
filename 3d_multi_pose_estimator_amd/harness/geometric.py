"""numpy statement of what mpe_geom_scores_batch computes (csrc/geom.hip): a matching score per edge-node from the
calibration alone -- the mean distance between the back-projected rays of the two skeletons over the joints both have.
The GPU tests hold the kernel to this module bit for bit.  include/mpe.h words the rule; the lines below are its lines.

All arithmetic is float64, every operation rounded on its own (numpy fuses nothing), in the header's order; only the
score is rounded to float32.  Vectorised over the edge-nodes (and their joints) of the batch; no transcendental function.
"""
import numpy as np

from .reprojection import engine_calibration

DEFAULTS = dict(sigma=0.10, clip=0.5, min_joints=1, joint_mask=None, min_conf=0.0)


def camera_constants(calib):
    """-> (K [V,3,3] f64 from the float32 intrinsics, dist [V,5], T [V,3,4]) in the order of the matching cameras (the index
    head_cam holds; reprojection.engine_calibration)."""
    P, dist, K32 = engine_calibration(calib)
    return K32.astype(np.float64), dist, P


def undistort(K, dist, cam, u, v):
    """csrc/dlt_common.h: undistort_point, elementwise (cam, u, v arrays of one shape) -> (x, y)."""
    fx, fy, cx, cy = K[cam, 0, 0], K[cam, 1, 1], K[cam, 0, 2], K[cam, 1, 2]
    k1, k2, p1, p2, k3 = (dist[cam, i] for i in range(5))
    with np.errstate(all='ignore'):
        ifx, ify = 1.0 / fx, 1.0 / fy
        x0, y0 = (u - cx) * ifx, (v - cy) * ify
        x, y = x0.copy(), y0.copy()
        alive = np.ones(x.shape, bool)
        for _ in range(5):
            r2 = x * x + y * y
            icdist = 1.0 / (1.0 + ((k3 * r2 + k2) * r2 + k1) * r2)
            neg = alive & (icdist < 0)
            dx = 2 * p1 * x * y + p2 * (r2 + 2 * x * x)
            dy = p1 * (r2 + 2 * y * y) + 2 * p2 * x * y
            upd = alive & ~neg
            x = np.where(upd, (x0 - dx) * icdist, np.where(neg, x0, x))
            y = np.where(upd, (y0 - dy) * icdist, np.where(neg, y0, y))
            alive = upd
    return x, y


def polish(K, dist, cam, u, v, x, y):
    """Two Newton steps on the lens model from undistort's (x, y): the header's lines, elementwise."""
    fx, fy, cx, cy = K[cam, 0, 0], K[cam, 1, 1], K[cam, 0, 2], K[cam, 1, 2]
    k1, k2, p1, p2, k3 = (dist[cam, i] for i in range(5))
    with np.errstate(all='ignore'):
        xt, yt = (u - cx) * (1.0 / fx), (v - cy) * (1.0 / fy)
        for _ in range(2):
            r = x * x + y * y
            f = 1.0 + ((k3 * r + k2) * r + k1) * r
            fd = ((3.0 * k3) * r + 2.0 * k2) * r + k1
            tx, ty = 2.0 * x, 2.0 * y
            ex = ((x * f + p1 * (tx * y)) + p2 * (r + tx * x)) - xt
            ey = ((y * f + p1 * (r + ty * y)) + p2 * (tx * y)) - yt
            a = ((f + (tx * x) * fd) + p1 * ty) + (3.0 * p2) * tx
            b = ((tx * y) * fd + p1 * tx) + p2 * ty
            d = ((f + (ty * y) * fd) + (3.0 * p1) * ty) + p2 * tx
            det = a * d - b * b
            x, y = x - (d * ex - b * ey) / det, y - (a * ey - b * ex) / det
    return x, y


def rays(calib, head_cam, xy):
    """head_cam [H], xy [H,J,2] -> (o [V,3] camera centres, r [H,J,3] unit directions), world frame."""
    K, dist, T = camera_constants(calib)
    cam = np.broadcast_to(np.asarray(head_cam, np.int64)[:, None], np.asarray(xy).shape[:2])
    xy = np.asarray(xy, np.float64)
    x, y = undistort(K, dist, cam, xy[..., 0], xy[..., 1])
    x, y = polish(K, dist, cam, xy[..., 0], xy[..., 1], x, y)
    with np.errstate(all='ignore'):
        q = [(T[cam, 0, k] * x + T[cam, 1, k] * y) + T[cam, 2, k] for k in range(3)]
        n = np.sqrt((q[0] * q[0] + q[1] * q[1]) + q[2] * q[2])
        r = np.stack([q[k] / n for k in range(3)], axis=-1)
    o = np.stack([-((T[:, 0, k] * T[:, 0, 3] + T[:, 1, k] * T[:, 1, 3]) + T[:, 2, k] * T[:, 2, 3]) for k in range(3)], axis=-1)
    return o, r


def _dot(a, b):
    return (a[..., 0] * b[..., 0] + a[..., 1] * b[..., 1]) + a[..., 2] * b[..., 2]


def pair_distance(o1, r1, o2, r2, clip=0.0):
    """The header's closest-point lines, elementwise: the rays (o1, r1) of h1 and (o2, r2) of h2 ([..., 3], broadcast
    against each other) -> (dist, clamped, parallel): the distance of the two rays at their closest points in front of
    both cameras (clip > 0 bounds it), whether a ray parameter was negative, whether the den < 1e-12 branch was taken.
    scores() and harness/consolidate.py both call this."""
    with np.errstate(all='ignore'):
        w = o1 - o2
        b, d, e = _dot(r1, r2), _dot(r1, w), _dot(r2, w)
        den = 1.0 - b * b
        parallel = den < 1e-12
        t1 = np.where(parallel, 0.0, (b * e - d) / den)
        t2 = np.where(parallel, e, (e - b * d) / den)
        clamped = (t1 < 0.0) | (t2 < 0.0)
        t1 = np.where(t1 < 0.0, 0.0, t1)
        t2 = np.where(t2 < 0.0, 0.0, t2)
        g = (o1 + t1[..., None] * r1) - (o2 + t2[..., None] * r2)
        dist = np.sqrt(_dot(g, g))
        if clip > 0.0:
            dist = np.where(dist > clip, clip, dist)
    return dist, clamped, parallel


def check_options(J, sigma, clip, min_joints, min_conf):
    if not sigma > 0.0 or not clip >= 0.0:
        raise ValueError('sigma must be positive and clip must not be negative')
    if not 1 <= int(min_joints) <= J:
        raise ValueError('min_joints in 1..%d' % J)
    if not min_conf >= 0.0:
        raise ValueError('min_conf must not be negative')


def batch_pairs(pb):
    """-> [n_edge_nodes, 2] batch-wide head indices of every edge-node (implicit or explicit list)."""
    out = [np.asarray(pb.pairs(f), np.int64).reshape(-1, 2) + int(pb.frame_head_off[f]) for f in range(pb.n_frames)]
    return np.concatenate(out) if out else np.zeros((0, 2), np.int64)


def scores(calib, pb, sigma=0.10, clip=0.5, min_joints=1, joint_mask=None, min_conf=0.0):
    """pb: a PackedBatch (host arrays).  -> {'scores' f32 [M], 'n_votes' u8 [M], 'mean' f64 [M] (-1 without a vote),
    'vote' bool [M,J], 'dist' f64 [M,J], 'clamped' bool [M,J] (a ray parameter was negative), 'parallel' bool [M,J] (the
    den < 1e-12 branch); the last three mean something where 'vote' is set."""
    J = pb.J
    sigma, clip, min_conf = float(sigma), float(clip), np.float32(min_conf)
    check_options(J, sigma, clip, min_joints, min_conf)
    every = (1 << J) - 1
    jm = (int(joint_mask) & every) if joint_mask else every
    pairs = batch_pairs(pb)
    h1, h2 = pairs[:, 0], pairs[:, 1]
    head_cam = np.asarray(pb.head_cam, np.int64)
    o, r = rays(calib, head_cam, pb.xy)
    bit = (np.uint32(1) << np.arange(J, dtype=np.uint32))[None, :]
    present = (np.asarray(pb.joint_mask, np.uint32)[:, None] & np.uint32(jm) & bit) != 0            # [H, J]
    conf = np.asarray(pb.vp, np.float32)[:, :, 0] >= min_conf
    c1, c2 = head_cam[h1], head_cam[h2]
    vote = (c1 != c2)[:, None] & present[h1] & present[h2] & conf[h1] & conf[h2]
    dist, clamped, parallel = pair_distance(o[c1][:, None, :], r[h1], o[c2][:, None, :], r[h2], clip)
    with np.errstate(all='ignore'):
        n = vote.sum(axis=1)
        total = np.zeros(len(pairs))
        for j in range(J):
            total = np.where(vote[:, j], total + dist[:, j], total)
        mean = np.where(n > 0, total / np.maximum(n, 1), -1.0)
        sc = np.where(n >= int(min_joints), (sigma / (sigma + mean)).astype(np.float32), np.float32(0.0)).astype(np.float32)
    return {'scores': sc, 'n_votes': n.astype(np.uint8), 'mean': mean, 'vote': vote, 'dist': dist, 'clamped': clamped & vote,
            'parallel': parallel & vote}


def report_line(opts):
    """The further line of the harness scripts under --matcher geometric."""
    return ('Matcher: geometric (ray distance; sigma %g m, clip %g m, at least %d joints, confidence >= %g)'
            % (opts['sigma'], opts['clip'], opts['min_joints'], opts['min_conf']))
