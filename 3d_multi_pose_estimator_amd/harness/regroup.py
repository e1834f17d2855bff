"""numpy statement of what mpe_regroup_batch computes (csrc/regroup.hip): the person proposals of a frame checked against
the 3D poses they led to -- the cost of every head against every person, heads released from rows they do not fit, free
heads attached to rows that lack their camera.  The GPU tests hold the kernel to this module bit for bit.  include/mpe.h
words the rule; the lines below are its lines.

All arithmetic is float64, every operation rounded on its own (numpy fuses nothing), in the header's order; the projection
is harness/refine.py's project64.  The cost table is vectorised per frame and camera; the release and attach passes are
plain Python over the entries of a frame.
"""
import numpy as np

from . import refine as RF

BAD_ROWS, OVER_CAP = 1, 2
RELEASE, ATTACH = 1, 2
MAX_PERSONS = 128
KEYS = ('persons', 'change', 'n_views', 'cost', 'counts', 'status')


def _has_pose(flags, n_persons, Pcap):
    """[F,Pcap] bool: row p < n_persons with a pose (joint flags: every row; person flags: the flag)."""
    flags = np.asarray(flags) != 0
    rows = np.arange(Pcap)[None, :] < np.clip(np.asarray(n_persons).astype(np.int64), 0, Pcap)[:, None]
    return rows if flags.ndim == 3 else rows & flags


def cost_table(calib, pb, poses, flags, n_persons, joint_mask, threshold=0.5, clip_px=0.0, min_joints=3, counts=False):
    """pb: the packed batch (host arrays); poses [F,Pcap,J,3] float32 or float64; flags [F,Pcap] (per person) or [F,Pcap,J]
    (per joint); n_persons [F].  -> cost [n_heads,Pcap] float64, -1 where the pair is unscored; with counts=True also n
    [n_heads,Pcap] int32, the counting joints of every pair (the tests' diagnostics)."""
    poses = np.asarray(poses)
    if poses.dtype not in (np.float32, np.float64):
        raise ValueError('poses must be float32 or float64')
    F, Pcap, J = poses.shape[:3]
    clip = float(clip_px)
    cost = np.full((pb.n_heads, Pcap), -1.0)
    n_all = np.zeros((pb.n_heads, Pcap), np.int32)
    if F == 0 or pb.n_heads == 0:
        return (cost, n_all) if counts else cost
    flags = np.asarray(flags) != 0
    has = _has_pose(flags, n_persons, Pcap)
    off = np.asarray(pb.frame_head_off).astype(np.int64)
    cam = np.asarray(pb.head_cam).astype(np.int64)
    T, kd, K = RF.camera_constants64(calib)
    V = T.shape[0]
    j = np.arange(J)
    picked = ((int(joint_mask) >> j) & 1) != 0
    in_dict = ((np.asarray(pb.joint_mask)[:, None] >> j.astype(np.uint32)) & 1) != 0             # [n_heads, J]
    valid = np.asarray(pb.vp, np.float32).reshape(-1, J, 2)[..., 0] > np.float32(threshold)
    head_ok = in_dict & valid & picked[None, :]
    xy = np.asarray(pb.xy, np.float64).reshape(-1, J, 2)
    with np.errstate(all='ignore'):
        for f in range(F):
            X = poses[f].astype(np.float64)                                                     # [Pcap, J, 3]
            person_ok = has[f][:, None] & np.isfinite(X).all(axis=2)
            if flags.ndim == 3:
                person_ok = person_ok & flags[f]
            for c in range(V):
                heads = off[f] + np.nonzero(cam[off[f]:off[f + 1]] == c)[0]
                if not len(heads):
                    continue
                p = RF.project64(T[c], kd[c], K[c], X[..., 0], X[..., 1], X[..., 2])
                rx = p['px'][None] - xy[heads, None, :, 0]                                      # [h, Pcap, J]
                ry = p['py'][None] - xy[heads, None, :, 1]
                e = np.sqrt(rx * rx + ry * ry)
                take = head_ok[heads, None, :] & (person_ok & (p['pc2'] > 0.0))[None] & (e < np.inf)
                if clip > 0.0:
                    e = np.where(e > clip, clip, e)
                s = np.zeros(e.shape[:2])
                for k in range(J):
                    s = np.where(take[..., k], s + e[..., k], s)
                n = take.sum(axis=2)
                q = s / n
                cost[heads] = np.where((n >= int(min_joints)) & (q < np.inf), q, -1.0)
                n_all[heads] = n
    return (cost, n_all) if counts else cost


def regroup(calib, pb, persons, n_persons, poses, flags, joint_mask, threshold=0.5, gate_px=15.0, clip_px=0.0, min_joints=3,
            release=True, attach=True, min_views=None, max_heads_per_frame=None, out=None):
    """persons [F,Pcap,V] / n_persons [F] as the matching stage wrote them; the rest as cost_table takes it; min_views:
    the context's (default: the parameters'); max_heads_per_frame: the context's cap (None: none); out: the int32 array
    that takes the rows (d_persons_out; `persons` itself regroups in place; None: a new array, `persons` is left alone).
    -> {'persons' [F,Pcap,V] i32, 'change' [F,Pcap,V] u8, 'n_views' [F,Pcap] i32, 'cost' [n_heads,Pcap] f64, 'counts'
    [F,4] i32, 'status' [F] i32}, what mpe_regroup_batch writes."""
    persons = np.asarray(persons, np.int32)
    F, Pcap, V = persons.shape
    if out is not None and (not isinstance(out, np.ndarray) or out.dtype != np.int32 or out.shape != persons.shape):
        raise ValueError('out must be an int32 array of the shape of persons')
    J = pb.J
    gate = float(gate_px)
    if not gate > 0.0 or not float(clip_px) >= 0.0:
        raise ValueError('gate_px > 0 and clip_px >= 0')
    if not 1 <= int(min_joints) <= J:
        raise ValueError('min_joints in 1..%d' % J)
    if not (release or attach):
        raise ValueError('release, attach or both')
    if Pcap > MAX_PERSONS:
        raise ValueError('at most %d rows per frame' % MAX_PERSONS)
    if min_views is None:
        min_views = calib.params.min_number_of_views
    cost = cost_table(calib, pb, poses, flags, n_persons, joint_mask, threshold, clip_px, min_joints)
    has = _has_pose(flags, n_persons, Pcap)
    off = np.asarray(pb.frame_head_off).astype(np.int64)
    cam = np.asarray(pb.head_cam).astype(np.int64)
    if out is None:
        out = persons.copy()
    elif out is not persons:
        out[...] = persons
    change =np.zeros((F, Pcap, V), np.uint8)
    n_views = np.zeros((F, Pcap), np.int32)
    counts = np.zeros((F, 4), np.int32)
    status = np.zeros(F, np.int32)
    for f in range(F):
        h0, H = int(off[f]), int(off[f + 1] - off[f])
        n = int(min(max(int(n_persons[f]), 0), Pcap))
        rows = out[f]
        was = rows.copy()                     # `persons` may be `out`
        copy = False
        if max_heads_per_frame is not None and H > max_heads_per_frame:
            status[f], copy = OVER_CAP, True
        else:
            named = np.zeros(H, bool)
            for p in range(n):
                for c in range(V):
                    e = int(rows[p, c])
                    if e < 0:
                        continue
                    if e >= H or cam[h0 + e] != c or named[e]:
                        status[f], copy = BAD_ROWS, True
                    else:
                        named[e] = True
        if not copy:
            if release:
                for p in range(n):
                    for c in range(V):
                        h = int(rows[p, c])
                        if h >= 0 and has[f, p] and cost[h0 + h, p] >= 0.0 and not cost[h0 + h, p] < gate:
                            rows[p, c] = -1
                            named[h] = False
            if attach:
                for c in range(V):
                    while True:
                        best = None
                        for h in range(H):
                            if cam[h0 + h] != c or named[h]:
                                continue
                            for p in range(n):
                                x = cost[h0 + h, p]
                                if has[f, p] and rows[p, c] < 0 and x >= 0.0 and x < gate and (best is None or (x, h, p) < best):
                                    best = (x, h, p)
                        if best is None:
                            break
                        rows[best[2], c] = best[1]
                        named[best[1]] = True
            moved = rows != was
            change[f] = (moved & (was >= 0)) * np.uint8(1) + (moved & (rows >= 0)) * np.uint8(2)
            n_views[f, :n] = (rows[:n] >= 0).sum(axis=1)
            counts[f] = (int(((change[f] & 1) != 0).sum()), int(((change[f] & 2) != 0).sum()), int((~named).sum()),
                         int((has[f] & (n_views[f] < int(min_views))).sum()))
        else:
            n_views[f, :n] = (rows[:n] >= 0).sum(axis=1)
    return {'persons': out, 'change': change, 'n_views': n_views, 'cost': cost, 'counts': counts, 'status': status}


def summary(outs):
    """Engine.regroup's (or regroup's) outputs of one or more batches, as host arrays -> {'released', 'attached', 'free',
    'below_min_views', 'copied'} summed over all frames (the extra line of the harness scripts; 'copied': the frames
    copied through)."""
    tot = np.zeros(4, np.int64)
    copied = 0
    for o in outs:
        tot += np.asarray(o['counts']).reshape(-1, 4).sum(axis=0)
        copied += int((np.asarray(o['status']) != 0).sum())
    return {'released': int(tot[0]), 'attached': int(tot[1]), 'free': int(tot[2]), 'below_min_views': int(tot[3]), 'copied': copied}
