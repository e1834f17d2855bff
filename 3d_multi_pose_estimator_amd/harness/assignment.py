"""numpy statement of what mpe_eval_batch computes (csrc/eval.hip): the callers' per-frame error table and their
pose-to-ground-truth assignment (metrics_from_model.py:303-337, metrics_from_triangulation.py:281-320).  The host
finishes here the frames the device search declines, and the tests hold the kernel to it.

Semantics -- the contract of the device path:

Detections.  As `infer()` hands them to `Metrics`, in the same order: MLP mode, persons p < n_persons[f] with
valid[f, p] (every joint present); triangulation mode, every p < n_persons[f] with the joint mask jvalid[f, p, :].
Frames whose graph has no cross-camera pair (M == 0) are skipped and not counted in n_data.

Error table.  table[g, r] is the mean, over the used joints present in GT body g (increasing joint index) that
detection r has, of |pose - gt|; 0 when there is none.  In triangulation mode a used GT joint missing from the
detection marks it invalid (for every body) and is left out of the mean.  Arithmetic is numpy's on the host
(`np.linalg.norm` of the difference, i.e. `x.dot(x)` through OpenBLAS, then sqrt):
  MLP mode: float32 poses minus float32 GT in float32; the dot takes the three float32 squares, sums them in
    float64 from 0 ((px + py) + pz) and rounds to float32; float32 sqrt (correctly rounded), float32 running sum,
    float32 divide.
  Triangulation mode: float64 poses minus float32 GT in float64; the dot is dx*dx followed by two fused
    multiply-adds (fma(dz, dz, fma(dy, dy, dx*dx))); float64 sqrt, sum and divide.
Nothing else is contracted.  (These are the orders numpy's dot takes here; the plain un-fused
((dx*dx + dy*dy) + dz*dz) differs from np.linalg.norm in the last bit for about one difference in ten.)

Assignment.  Exactly what the reference's loop returns: the minimum, under strict `<` starting from 10000., of the
left-fold float64 sum over rows g = 0..G-1, permutations in itertools order over range(max(G, R)), columns >= R
contributing nothing; ties go to the lexicographically first permutation; None when no sum is below 10000.
`assign_bnb` finds it by a depth-first branch-and-bound in the same order: a child is kept while the left fold of
its partial sum followed by the row minima (np.fmin) of the rows below is < the incumbent.  Rounding is monotone
(x <= y implies fl(x + c) <= fl(y + c)), so a pruned subtree holds no sum the strict `<` would accept.  Of the
columns >= R (all zero) only the lowest unused one is tried: the others give the same sums later in itertools order.
"""
from fractions import Fraction

import numpy as np


def _fma(a, b, c):
    return float(Fraction(float(a)) * Fraction(float(b)) + Fraction(float(c)))   # int / int: correctly rounded


_fma_v = np.frompyfunc(_fma, 3, 1)


def error_table(poses, present, gt_xyz, gt_joint, used):
    """poses [R,J,3] (float32: MLP mode, float64: triangulation), present [R,J] bool, gt_xyz [G,J,3] float32,
    gt_joint [G,J] bool, used [J] bool -> (table [G,R] float64, invalid [R] bool)."""
    poses = np.asarray(poses)
    present = np.asarray(present, bool)
    gt_xyz = np.asarray(gt_xyz, np.float32)
    R, G = poses.shape[0], gt_xyz.shape[0]
    J = gt_xyz.shape[1] if G else poses.shape[1] if R else 0
    m = np.asarray(gt_joint, bool)[:, None, :] & np.asarray(used, bool)[None, None, :]          # [G,1,J]
    invalid = (m & ~present[None]).any(axis=(0, 2)) if G and R else np.zeros(R, bool)
    take = m & present[None]                                                                     # [G,R,J]
    if poses.dtype == np.float32:
        d = poses[None] - gt_xyz[:, None]                                                        # f32
        p = d * d
        s = ((p[..., 0].astype(np.float64) + p[..., 1]) + p[..., 2]).astype(np.float32)
        nrm = np.sqrt(s)
        tot = np.zeros((G, R), np.float32)
    else:
        d = poses.astype(np.float64)[None] - gt_xyz[:, None].astype(np.float64)
        s = d[..., 0] * d[..., 0]
        if s.size:
            s = _fma_v(d[..., 1], d[..., 1], s).astype(np.float64)
            s = _fma_v(d[..., 2], d[..., 2], s).astype(np.float64)
        nrm = np.sqrt(s)
        tot = np.zeros((G, R), np.float64)
    for j in range(J):
        tot = np.where(take[..., j], tot + nrm[..., j], tot)
    n = take.sum(axis=2)
    mean = (tot / np.maximum(n, 1).astype(tot.dtype)).astype(tot.dtype)
    return np.where(n > 0, mean.astype(np.float64), 0.0), invalid


def assign_bnb(table, node_budget=None):
    """table [G,R] float64 -> best_p as the reference's loop leaves it (tuple: column of each row over
    range(max(G, R))) or None.  node_budget: raise RuntimeError after that many loop iterations (None: no limit)."""
    t0 = np.asarray(table, np.float64)
    G, R = t0.shape
    if G == 0:
        return ()
    N = max(G, R)
    t = np.zeros((G, N))
    t[:, :R] = t0
    rm = np.fmin.reduce(t, axis=1)
    used = np.zeros(N, bool)
    path = [0] * G
    cand = [None] * G
    accs = [0.0] * G
    cand[0] = np.ones(N, bool)
    best, best_p = 10000., None
    d = iters = 0
    while True:
        iters += 1
        if node_budget is not None and iters > node_budget:
            raise RuntimeError('assign_bnb: node budget exhausted')
        acc = accs[d]
        ok = cand[d] & ~used
        if N > R:
            free = np.flatnonzero(~used[R:])
            keep = bool(ok[R + free[0]]) if len(free) else False
            ok[R:] = False
            if keep:
                ok[R + free[0]] = True
        b = acc + t[d]
        for k in range(d + 1, G):
            b = b + rm[k]
        ok &= b < best
        idx = np.flatnonzero(ok)
        if len(idx) == 0:
            if d == 0:
                break
            d -= 1
            used[path[d]] = False
            continue
        c = int(idx[0])
        ok[c] = False
        cand[d] = ok
        path[d] = c
        na = acc + t[d, c]
        if d + 1 == G:
            best, best_p = na, tuple(path)
            continue
        used[c] = True
        d += 1
        accs[d] = na
        cand[d] = np.ones(N, bool)
    return best_p


def frame_records(table, best_p):
    """-> (assign [R] int32, err [R] float64) of one frame from the reference's best_p (None: nothing assigned)."""
    G, R = np.shape(table)
    assign = np.full(R, -1, np.int32)
    err = np.zeros(R, np.float64)
    if best_p is not None:
        for g, r in enumerate(best_p):
            if r < R:
                assign[r] = g
                err[r] = table[g][r]
    return assign, err
