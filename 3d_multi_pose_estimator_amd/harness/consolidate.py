"""numpy statement of what mpe_consolidate_batch computes (csrc/consolidate.hip): the two repairs the regrouping leaves
open -- rows whose poses lie on one body are merged, and the skeletons no row names found new rows where their rays
meet.  The GPU tests hold the kernel to this module bit for bit.  include/mpe.h words the rule; the lines below are its
lines.

All arithmetic is float64, every operation rounded on its own (numpy fuses nothing), in the header's order.  The merge
distance is harness/tracking.py's cost; the pair cost of two free heads is harness/geometric.py's mean ray distance
(rays and pair_distance, the functions scores() calls) under the regrouping's vote rule.  The two tables are vectorised
per frame; the merge and found passes are plain Python over a frame.
"""
import numpy as np

from . import geometric as G
from .regroup import MAX_PERSONS, _has_pose

BAD_ROWS, OVER_CAP, FREE_OVER_CAP, ROWS_FULL = 1, 2, 4, 8
MERGE, FOUND = 1, 2
MAX_FREE = 64
RAY_DOUBLES = 3520
KEYS = ('persons', 'n_persons', 'change', 'n_views', 'dist', 'pair', 'free', 'counts', 'status')


def default_fcap(J, max_heads_per_frame=None):
    """min(the context's head cap, 64), within the ray store of the kernel."""
    cap = min(MAX_FREE, RAY_DOUBLES // (3 * J + 1))
    return max(1, cap if max_heads_per_frame is None else min(cap, int(max_heads_per_frame)))


def dist_table(poses, flags, n_persons, joint_mask, min_joints=3, counts=False):
    """poses [F,Pcap,J,3] float32 or float64; flags [F,Pcap] (per person) or [F,Pcap,J] (per joint); n_persons [F].
    -> dist [F,Pcap,Pcap] float64: the tracker's cost of rows p < q < n at [p][q], -1 where the pair is unscored and
    everywhere else; with counts=True also n [F,Pcap,Pcap] int32, the joints both rows have."""
    poses = np.asarray(poses)
    if poses.dtype not in (np.float32, np.float64):
        raise ValueError('poses must be float32 or float64')
    F, Pcap, J = poses.shape[:3]
    flags = np.asarray(flags) != 0
    has = _has_pose(flags, n_persons, Pcap)
    picked = ((int(joint_mask) >> np.arange(J)) & 1) != 0
    X = poses.astype(np.float64)
    present = has[:, :, None] & picked[None, None, :] & np.isfinite(X).all(axis=3)
    if flags.ndim == 3:
        present = present & flags
    dist = np.full((F, Pcap, Pcap), -1.0)
    n_all = np.zeros((F, Pcap, Pcap), np.int32)
    upper = np.triu(np.ones((Pcap, Pcap), bool), 1)
    with np.errstate(all='ignore'):
        for f in range(F):
            both = present[f][:, None, :] & present[f][None, :, :]                             # [p, q, J]
            d = X[f][:, None] - X[f][None]                                                     # a - b, p in the role of a
            s = d[..., 0] * d[..., 0]
            s = s + d[..., 1] * d[..., 1]
            s = s + d[..., 2] * d[..., 2]
            nrm = np.sqrt(s)
            tot = np.zeros((Pcap, Pcap))
            for j in range(J):
                tot = np.where(both[..., j], tot + nrm[..., j], tot)
            n = both.sum(axis=2)
            q = tot / n
            dist[f] = np.where(upper & (n >= int(min_joints)) & (q < np.inf), q, -1.0)
            n_all[f] = np.where(upper, n, 0)
    return (dist, n_all) if counts else dist


def head_votes(pb, joint_mask, threshold=0.5):
    """-> [n_heads, J] bool: the joints of every head that may vote (asked for, in the head's dictionary, d_vp[h][j][0] >
    threshold, a camera index inside 0..V-1)."""
    J = pb.J
    j = np.arange(J)
    picked = ((int(joint_mask) >> j) & 1) != 0
    in_dict = ((np.asarray(pb.joint_mask, np.uint32)[:, None] >> j.astype(np.uint32)) & 1) != 0
    valid = np.asarray(pb.vp, np.float32).reshape(-1, J, 2)[..., 0] > np.float32(threshold)
    cam = np.asarray(pb.head_cam).astype(np.int64)
    return in_dict & valid & picked[None, :] & ((cam >= 0) & (cam < pb.V))[:, None]


def pair_costs(o, r, cam, votes, heads, clip_m=0.0, min_joints=3, counts=False):
    """o [V,3], r [n_heads,J,3] (geometric.rays), cam and votes per head of the batch; heads: batch-wide indices of the K
    free heads of a frame in increasing order -> [K,K] float64: the mean ray distance of heads a < b at [a][b], -1 where
    the pair is unscored and everywhere else; with counts=True also n [K,K]."""
    K = len(heads)
    cost = np.full((K, K), -1.0)
    n_all = np.zeros((K, K), np.int32)
    ia, ib = np.triu_indices(K, 1)
    if len(ia):
        ha, hb = heads[ia], heads[ib]
        ca, cb = np.clip(cam[ha], 0, len(o) - 1), np.clip(cam[hb], 0, len(o) - 1)
        vote = (cam[ha] != cam[hb])[:, None] & votes[ha] & votes[hb]
        dist, _, _ = G.pair_distance(o[ca][:, None, :], r[ha], o[cb][:, None, :], r[hb], float(clip_m))
        with np.errstate(all='ignore'):
            total = np.zeros(len(ia))
            for j in range(vote.shape[1]):
                total = np.where(vote[:, j], total + dist[:, j], total)
            n = vote.sum(axis=1)
            mean = total / n
            cost[ia, ib] = np.where((n >= int(min_joints)) & (mean < np.inf), mean, -1.0)
        n_all[ia, ib] = n
    return (cost, n_all) if counts else cost


def merge_rows(rows, n, dist, merge_m):
    """The merge pass on the rows [Pcap,V] of a frame, in place -> the rows merged away, in order."""
    gone = []
    while True:
        best = None
        for p in range(n):
            for q in range(p + 1, n):
                x = dist[p, q]
                if p in gone or q in gone or not (x >= 0.0 and x < merge_m) or ((rows[p] >= 0) & (rows[q] >= 0)).any():
                    continue
                if best is None or (x, p, q) < best:
                    best = (x, p, q)
        if best is None:
            return gone
        _, p, q = best
        rows[p] = np.where(rows[q] >= 0, rows[q], rows[p])
        rows[q] = -1
        gone.append(q)


def found_rows(rows, n, pair, free, cam, found_m, found_min_views, trace=None):
    """The found pass on the rows [Pcap,V] of a frame, in place.  pair [K,K] by rank, free [K] frame-local head ids, cam [K]
    their cameras -> (the new row count, heads placed, ROWS_FULL or 0); trace takes (seed a, seed b, members, founded)."""
    Pcap, K = rows.shape[0], len(free)
    is_free = np.ones(K, bool)
    placed = 0

    def cost(x, y):
        return pair[min(x, y), max(x, y)]

    cursor = (-1.0, -1, -1)
    while True:
        best = None
        for a in range(K):
            for b in range(a + 1, K):
                x = pair[a, b]
                if is_free[a] and is_free[b] and x >= 0.0 and x < found_m and (x, a, b) > cursor and (best is None or (x, a, b) < best):
                    best = (x, a, b)
        if best is None:
            return n, placed, 0
        if n == Pcap:
            return n, placed, ROWS_FULL
        cursor = best
        members = [best[1], best[2]]
        while True:
            pick = None
            for h in range(K):
                if not is_free[h] or h in members or cam[h] in [cam[m] for m in members]:
                    continue
                cs = [cost(h, m) for m in members]
                if all(c >= 0.0 and c < found_m for c in cs) and (pick is None or (max(cs), h) < pick):
                    pick = (max(cs), h)
            if pick is None:
                break
            members.append(pick[1])
        ok = len(members) >= found_min_views
        if trace is not None:
            trace.append((best[1], best[2], list(members), ok))
        if not ok:
            continue
        rows[n] = -1
        for m in members:
            rows[n, cam[m]] = free[m]
            is_free[m] = False
        n += 1
        placed += len(members)


def consolidate(calib, pb, persons, n_persons, poses, flags, joint_mask, threshold=0.5, merge_m=0.10, found_m=0.05, clip_m=0.0,
                min_joints=3, found_min_views=None, fcap=None, merge=True, found=True, max_heads_per_frame=None, out=None, n_out=None,
                trace=None):
    """persons [F,Pcap,V] / n_persons [F] / poses / flags / joint_mask / threshold as harness.regroup.regroup takes them;
    found_min_views: None = max(2, the parameters' minimum number of views); fcap: None = default_fcap; max_heads_per_frame:
    the context's cap (None: none); out / n_out: the int32 arrays that take the rows and the counts (`persons` / `n_persons`
    themselves consolidate in place; None: new arrays); trace: a list that takes (frame, seed a, seed b, members, founded)
    of every seed.  -> {'persons' [F,Pcap,V] i32, 'n_persons' [F] i32, 'change' [F,Pcap,V] u8, 'n_views' [F,Pcap] i32, 'dist'
    [F,Pcap,Pcap] f64, 'pair' [F,fcap,fcap] f64, 'free' [F,fcap] i32, 'counts' [F,4] i32, 'status' [F] i32}, what
    mpe_consolidate_batch writes."""
    persons = np.asarray(persons, np.int32)
    n_persons = np.asarray(n_persons, np.int32)
    F, Pcap, V = persons.shape
    J = pb.J
    if out is not None and (not isinstance(out, np.ndarray) or out.dtype != np.int32 or out.shape != persons.shape):
        raise ValueError('out must be an int32 array of the shape of persons')
    if n_out is not None and (not isinstance(n_out, np.ndarray) or n_out.dtype != np.int32 or n_out.shape != (F,)):
        raise ValueError('n_out must be an int32 array of the shape of n_persons')
    merge_m, found_m, clip_m = float(merge_m), float(found_m), float(clip_m)
    if not merge_m > 0.0 or not found_m > 0.0 or not clip_m >= 0.0:
        raise ValueError('merge_m > 0, found_m > 0 and clip_m >= 0')
    if not 1 <= int(min_joints) <= J:
        raise ValueError('min_joints in 1..%d' % J)
    if found_min_views is None:
        found_min_views = max(2, int(calib.params.min_number_of_views))
    if int(found_min_views) < 2:
        raise ValueError('found_min_views >= 2')
    if fcap is None:
        fcap = default_fcap(J, max_heads_per_frame)
    fcap = int(fcap)
    if not 1 <= fcap <= MAX_FREE or fcap * (3 * J + 1) > RAY_DOUBLES:
        raise ValueError('fcap in 1..%d, within %d ray doubles' % (MAX_FREE, RAY_DOUBLES))
    if not (merge or found):
        raise ValueError('merge, found or both')
    if Pcap > MAX_PERSONS:
        raise ValueError('at most %d rows per frame' % MAX_PERSONS)
    dist = dist_table(poses, flags, n_persons, joint_mask, min_joints)
    off = np.asarray(pb.frame_head_off).astype(np.int64)
    cam = np.asarray(pb.head_cam).astype(np.int64)
    votes = head_votes(pb, joint_mask, threshold)
    if pb.n_heads:
        o, r = G.rays(calib, np.clip(cam, 0, V - 1), np.asarray(pb.xy, np.float64).reshape(-1, J, 2))
    else:
        o, r = np.zeros((V, 3)), np.zeros((0, J, 3))
    n_in = n_persons.copy()                   # `n_persons` may be `n_out`
    if out is None:
        out = persons.copy()
    elif out is not persons:
        out[...] = persons
    if n_out is None:
        n_out = np.zeros(F, np.int32)
    change = np.zeros((F, Pcap, V), np.uint8)
    n_views = np.zeros((F, Pcap), np.int32)
    pair = np.full((F, fcap, fcap), -1.0)
    free = np.full((F, fcap), -1, np.int32)
    counts = np.zeros((F, 4), np.int32)
    status = np.zeros(F, np.int32)
    for f in range(F):
        h0, H = int(off[f]), int(off[f + 1] - off[f])
        n = int(min(max(int(n_in[f]), 0), Pcap))
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
        if copy:
            dist[f] = -1.0
            n_views[f, :n] = (rows[:n] >= 0).sum(axis=1)
            n_out[f] = n_in[f]
            continue
        gone = merge_rows(rows, n, dist[f], merge_m) if merge else []
        heads = np.flatnonzero(~named)
        K = len(heads)
        free[f, :min(K, fcap)] = heads[:fcap]
        n_now, placed = n, 0
        if K > fcap:
            status[f] |= FREE_OVER_CAP
        else:
            pair[f, :K, :K] = pair_costs(o, r, cam, votes, h0 + heads, clip_m, min_joints)
            if found:
                tr = None if trace is None else []
                n_now, placed, full = found_rows(rows, n, pair[f, :K, :K], heads, cam[h0 + heads], found_m, int(found_min_views), tr)
                status[f] |= full
                if trace is not None:
                    trace.extend((f,) + t for t in tr)
        moved = rows != was
        change[f] = (moved & (was >= 0)) * np.uint8(1) + (moved & (rows >= 0)) * np.uint8(2)
        n_views[f, :n_now] = (rows[:n_now] >= 0).sum(axis=1)
        counts[f] = (len(gone), n_now - n, placed, K - placed)
        n_out[f] = n_now
    return {'persons': out, 'n_persons': n_out, 'change': change, 'n_views': n_views, 'dist': dist, 'pair': pair, 'free': free,
            'counts': counts, 'status': status}


def summary(outs):
    """Engine.consolidate's (or consolidate's) outputs of one or more batches, as host arrays -> {'merged', 'founded',
    'placed', 'free', 'copied'} summed over all frames (the further line of the harness scripts; 'copied': the frames
    copied through)."""
    tot = np.zeros(4, np.int64)
    copied = 0
    for o in outs:
        tot += np.asarray(o['counts']).reshape(-1, 4).sum(axis=0)
        copied += int((np.asarray(o['status']) & (BAD_ROWS | OVER_CAP) != 0).sum())
    return {'merged': int(tot[0]), 'founded': int(tot[1]), 'placed': int(tot[2]), 'free': int(tot[3]), 'copied': copied}
