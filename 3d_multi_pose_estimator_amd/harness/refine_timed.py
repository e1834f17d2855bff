"""numpy statement of what mpe_refine_timed_batch computes (csrc/refine_timed.hip): harness/refine.py's refinement with every
camera looking at the joint where the joint's track says it was at that camera's time.  A camera that lags by L frames saw,
in its picture of frame f, the world at f + L; the table of tracked poses gives how far the joint moved between f and f + L,
and camera c projects the unknown point displaced by that much.  The GPU tests hold the kernel to this module bit for bit.
include/mpe.h words the rule; the lines below are its lines.

All arithmetic is float64, every operation rounded on its own, in the header's order.  The projection, the cost, the step
and the acceptance are harness/refine.py's own functions; the rows of a track are harness/lag.py's.
"""
import math

import numpy as np

from . import reprojection as R
from .lag import MAX_WINDOW, track_rows
from .refine import MAX_ITERS, PAIRS, SOLVED, MOVED, CONVERGED, FEW_VIEWS, BAD_START, _rho, camera_constants64, huber_weight, lm_step3, project64


def split_lag(lag):
    """L -> (s, alpha): s = floor(L), alpha = L - s (one subtraction)."""
    L = float(lag)
    if not math.isfinite(L) or abs(L) > MAX_WINDOW:
        raise ValueError('a lag must be finite and within %d frames' % MAX_WINDOW)
    s = math.floor(L)
    return int(s), L - float(s)


def offsets(frame_start, n_frames, table_poses, table_flags, table_n_persons, table_ids, lags):
    """-> (d [F,Pcap,V,J,3] float64, has [F,Pcap,V,J] bool): per joint of the call's frames and camera, X_l - X_f from the rows
    of the joint's track in the table, and whether the three (or two) rows exist with the joint flagged and finite.  A
    camera with lag 0 has none."""
    poses = np.asarray(table_poses)
    flags = np.asarray(table_flags)
    n_table, Pcap, J = poses.shape[:3]
    F, V = int(n_frames), len(lags)
    parts = [split_lag(x) for x in lags]
    W = max([0] + [max(abs(s), abs(s + 1)) for s, _ in parts])
    rows = track_rows(frame_start, F, flags, table_n_persons, table_ids, W)      # [F,Pcap,2W+1]: the row in frame f - W + w
    X = poses.astype(np.float64)
    flagged = (flags != 0) if flags.ndim == 3 else np.repeat((flags != 0)[..., None], J, axis=2)
    good = flagged & np.isfinite(X).all(axis=-1)                                  # [n_table,Pcap,J]
    fl = np.arange(F)[:, None]

    def joint_of(shift):
        g = np.clip(frame_start + fl + shift, 0, max(n_table - 1, 0))
        row = rows[:, :, W + shift]
        at = np.maximum(row, 0)
        return X[g, at], (row >= 0)[..., None] & good[g, at]                      # [F,Pcap,J,3], [F,Pcap,J]

    d = np.zeros((F, Pcap, V, J, 3))
    has = np.zeros((F, Pcap, V, J), bool)
    if F == 0:
        return d, has
    Xf, ok_f = joint_of(0)
    with np.errstate(all='ignore'):
        for c, (s, alpha) in enumerate(parts):
            if float(lags[c]) == 0.0:
                continue
            Xl, ok = joint_of(s)
            if alpha != 0.0:
                Xb, ok_b = joint_of(s + 1)
                Xl = Xl + alpha * (Xb - Xl)
                ok = ok & ok_b
            has[:, :, c] = ok & ok_f
            d[:, :, c] = np.where(has[:, :, c, :, None], Xl - Xf, 0.0)
    return d, has


def _cost(cams, X, d, timed, xy, obs, huber):
    """refine._cost with camera c projecting X + d[:, c] where timed[:, c] -> (C [N], every observing camera has pc2 > 0 [N])."""
    C = np.zeros(X.shape[0])
    front = np.ones(X.shape[0], bool)
    with np.errstate(all='ignore'):
        for c, (T, kd, K) in enumerate(cams):
            Z = np.where(timed[:, c, None], X + d[:, c], X)
            p = project64(T, kd, K, Z[:, 0], Z[:, 1], Z[:, 2])
            rx = p['px'] - xy[:, c, 0]
            ry = p['py'] - xy[:, c, 1]
            C = np.where(obs[:, c], C + _rho(np.sqrt(rx * rx + ry * ry), huber), C)
            front &= ~obs[:, c] | (p['pc2'] > 0.0)
    return C, front


def refine_timed(calib, pb, frame_start, persons, table_poses, table_flags, table_n_persons, table_ids, lags, joint_mask, threshold=0.5,
                 max_iters=10, step_tol=1e-6, huber_px=0.0, start=None):
    """One mpe_refine_timed_batch call on the host: pb holds the detections of the table frames frame_start .. frame_start +
    F - 1, persons [F,Pcap,V] their rows; the table is poses [n_table,Pcap,J,3] float32 or float64, flags [n_table,Pcap] or
    [n_table,Pcap,J], n_persons [n_table], ids [n_table,Pcap]; lags: V floats, frames, with the sign of the lag report.
    start: poses [F,Pcap,J,3] of the table's type to start from instead of the table's own rows (an experiment of the host
    tests; the entry point always starts at the table).  -> refine.refine's dict plus 'n_timed' u8 [F,Pcap,J]."""
    if not 1 <= int(max_iters) <= MAX_ITERS or not step_tol >= 0.0 or not huber_px >= 0.0:
        raise ValueError('max_iters in 1..%d, step_tol >= 0 and huber_px >= 0' % MAX_ITERS)
    table = np.asarray(table_poses)
    if table.dtype not in (np.float32, np.float64):
        raise ValueError('poses must be float32 or float64')
    huber, step_tol = float(huber_px), float(step_tol)
    persons = np.asarray(persons)
    F, Pcap, V = persons.shape
    flags = np.asarray(table_flags)
    n_table, J = table.shape[0], pb.J
    if len(lags) != V:
        raise ValueError('%d lags for %d cameras' % (len(lags), V))
    if frame_start < 0 or frame_start + F > n_table:
        raise ValueError('the frames of the call lie outside the table')
    sl = slice(frame_start, frame_start + F)
    poses = table[sl] if start is None else np.asarray(start)
    if poses.dtype != table.dtype or poses.shape != table[sl].shape:
        raise ValueError('start must have the type of the table and the shape of the call\'s frames of it')
    sel, xy = R.selection(pb, persons, np.asarray(table_n_persons)[sl], flags[sl], joint_mask, threshold)
    obs = np.ascontiguousarray(np.moveaxis(sel, 2, 3)).reshape(-1, V)                 # [N, V], N = F * Pcap * J
    xy = np.ascontiguousarray(np.moveaxis(xy, 2, 3)).reshape(-1, V, 2)
    d, has = offsets(frame_start, F, table, flags, table_n_persons, table_ids, lags)
    d = np.ascontiguousarray(np.moveaxis(d, 2, 3)).reshape(-1, V, 3)
    timed = obs & np.ascontiguousarray(np.moveaxis(has, 2, 3)).reshape(-1, V)
    n_timed = timed.sum(axis=1)
    start = poses.reshape(-1, 3)
    N = start.shape[0]
    cams = list(zip(*camera_constants64(calib)))
    views = obs.sum(axis=1)
    status = np.zeros(N, np.uint8)
    status[views == 1] = FEW_VIEWS
    X = start.astype(np.float64)
    many = views >= 2
    C, front = _cost(cams, X, d, timed, xy, obs & many[:, None], huber)
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
                Z = np.where(timed[:, c, None], X + d[:, c], X)
                p = project64(T, kd, K, Z[:, 0], Z[:, 1], Z[:, 2], jacobian=True)
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
            Ct, front = _cost(cams, Y, d, timed, xy, obs, huber)
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
            'cost1': np.where(solved, C, -1.0).reshape(shape), 'iters': iters.reshape(shape), 'n_views': views.astype(np.uint8).reshape(shape),
            'n_timed': n_timed.astype(np.uint8).reshape(shape)}


def summary(outs, lags):
    """refine_timed's (or Engine.refine_timed's) outputs of one or more batches, as host arrays -> harness.refine.summary's
    figures plus 'cameras_lagged' and 'joints_timed' (joints with at least one timed camera)."""
    from .refine import summary as plain
    out = plain(outs)
    out['cameras_lagged'] = int(sum(1 for x in lags if float(x) != 0.0))
    out['joints_timed'] = int(sum(int((np.asarray(o['n_timed']) > 0).sum()) for o in outs))
    return out
