"""numpy statement of what mpe_partition_labels, mpe_group_bodies and mpe_partition_scores compute (csrc/partition.hip):
the scoring of test/sm_metrics.py and test/sm_metrics_without_gt.py.  The GPU tests hold the kernels to this module bit
for bit; the host tests hold this module to sklearn and to the harness's own loops.  No sklearn here.

Labels.  One label per head: the index of the first proposal that holds it, else the number of proposals
(sm_metrics.py:211-218, sm_metrics_without_gt.py:133-141).

Ground-truth grouping (sm_metrics.py:125-157).  The skeletons of a frame's bodies_3D, in (used camera, list) order, are
taken one by one; against every person founded so far the distance is the sum, over the PERSON's keys in the order of its
founding body's dict, of |skeleton[key] - person[key]| for the keys the skeleton has too; the person with the smallest sum
wins (strict `<` from 1e9: the first of equals, and never a NaN); without a shared key, or with a mean distance > 1.,
the skeleton founds a new person.  A frame without any skeleton, or with a body that lacks '-1', is skipped.  The
distance of one key is float64 sqrt(dot(d, d)) with numpy's float64 dot of three elements, the rule csrc/eval.hip and
harness/assignment.py use for float64 poses: fma(dz, dz, fma(dy, dy, dx*dx)).

Scores.  sklearn's adjusted_rand_score and homogeneity_completeness_v_measure (metrics/cluster/_supervised.py), with
every sum taken in a written order:
  n_ij = samples of true class i in predicted class j, a_i / b_j its row / column sums, n their total
  tp = sum n_ij^2 - n ; fp = sum b_j^2 - sum n_ij^2 ; fn = sum a_i^2 - sum n_ij^2 ; tn = n^2 - fp - fn - sum n_ij^2   (integers)
  ari = 1.0 if fn == 0 and fp == 0 else 2.0 * (tp*tn - fn*fp) / ((tp+fn)*(fn+tn) + (tp+fp)*(fp+tn))
  H(counts) = 0.0 for one class, else -(sum over the classes in ascending label order of (c/n) * (log c - log n))
  mi = 0.0 if either side has one class, else max(0, sum over the non-zero cells in ascending (i, j) order of
       t = nm*(log n_ij - log n) + nm*(((-log(a_i*b_j)) + log n) + log n), nm = n_ij / n, t = 0 where |t| < eps)
  h = mi / H_true if H_true else 1.0 ; c = mi / H_pred if H_pred else 1.0 ; v = 0.0 if h + c == 0 else ((2.0*h)*c) / (h + c)
Sums start from 0.0 and run left to right; no product is fused into a sum.  Every logarithm is of an integer <= n^2 and is
read from ONE table, log_table(): np.log(np.arange(1, K + 1, dtype=float64)); the device is handed the same table, so
host and device use the same logarithms bit for bit.  (sklearn sums pairwise and takes some logarithms from libm: the
two differ in the last bits, below 1e-12.)
"""
from fractions import Fraction

import numpy as np

from ..lib import MPE_PART_MAX_KEYS
from ..logtable import log_table
from ..parameters import parameters

KEY_CAP = MPE_PART_MAX_KEYS   # distinct joint keys of a packed batch: one presence bit each
EPS = float(np.finfo(np.float64).eps)


def proposal_labels(persons_row, n_persons, H):
    """persons_row: the proposals of one frame, [>= n_persons] rows of head ids (entries < 0: None) -> [H] int32."""
    out = np.full(H, int(n_persons), np.int32)
    for p in range(int(n_persons) - 1, -1, -1):
        for h in persons_row[p]:
            h = int(h)
            if 0 <= h < H:
                out[h] = p
    return out


# ---- ground-truth grouping ---------------------------------------------------------------------------------------------
def pack_bodies(frames, used_cameras=None):
    """bodies_3D of every frame (frame[cam][3]; cameras outside `used_cameras` are passed over, as gt_labels does), packed
    densely in (used camera, list) order -> dict:
      keys   the distinct joint keys of the batch, slot k = keys[k]
      n      [B] int32        skeletons of the frame
      xyz    [B,Scap,Kcap,3]  float64 coordinates per key slot (0 where the body has no such key)
      mask   [B,Scap] uint32  bit k: the body has key k
      nkeys  [B,Scap] int32   keys of the body;  order [B,Scap,Kcap] uint8: their slots in the order of the body's dict
      m1     [B,Scap] uint8   '-1' in body
    Scap / Kcap = the largest count, at least 1.  ValueError for a value that is not three numbers, or for more than
    KEY_CAP distinct keys."""
    used = parameters.used_cameras if used_cameras is None else used_cameras
    per = [[body for cam in f if cam in used for body in f[cam][3]] for f in frames]
    keys = {}
    for bodies in per:
        for body in bodies:
            for k in body:
                keys.setdefault(k, len(keys))
    if len(keys) > KEY_CAP:
        raise ValueError('pack_bodies: %d distinct joint keys, at most %d' % (len(keys), KEY_CAP))
    B, scap, kcap = len(per), max([1] + [len(b) for b in per]), max(1, len(keys))
    out = {'keys': list(keys), 'n': np.array([len(b) for b in per], np.int32).reshape(B),
           'xyz': np.zeros((B, scap, kcap, 3), np.float64), 'mask': np.zeros((B, scap), np.uint32),
           'nkeys': np.zeros((B, scap), np.int32), 'order': np.zeros((B, scap, kcap), np.uint8), 'm1': np.zeros((B, scap), np.uint8)}
    for f, bodies in enumerate(per):
        for s, body in enumerate(bodies):
            out['m1'][f, s] = '-1' in body
            if not body:
                continue
            slots = [keys[k] for k in body]
            try:
                v = np.array(list(body.values()), np.float64)
            except (ValueError, TypeError):
                v = np.zeros(0)
            if v.shape != (len(slots), 3):
                raise ValueError('pack_bodies: a joint of a body is not three numbers')
            out['nkeys'][f, s] = len(slots)
            out['xyz'][f, s, slots] = v
            out['mask'][f, s] = sum(1 << k for k in slots)
            out['order'][f, s, :len(slots)] = slots
    return out


def _fma(a, b, c):
    return float(Fraction(float(a)) * Fraction(float(b)) + Fraction(float(c)))   # int / int: correctly rounded


def _distance(a, b):
    with np.errstate(all='ignore'):
        d = a - b
        try:
            return float(np.sqrt(np.float64(_fma(d[2], d[2], _fma(d[1], d[1], d[0] * d[0])))))
        except (OverflowError, ValueError):          # a non-finite term: any order gives the same inf / NaN
            return float(np.sqrt(np.dot(d, d)))


def group_bodies(n, xyz, mask, nkeys, order, m1):
    """One frame of pack_bodies (n and the frame's rows of the arrays) -> (labels [n] int32, number of persons, skip)."""
    n = int(n)
    founders, labels = [], np.zeros(n, np.int32)
    for s in range(n):
        best, matched, n_joints = 1000000000., -1, 0
        for pid, q in enumerate(founders):
            dist, cnt = 0.0, 0
            for k in order[q, :nkeys[q]]:
                if (int(mask[s]) >> int(k)) & 1:
                    dist = dist + _distance(xyz[s, k], xyz[q, k])
                    cnt += 1
            if dist < best:
                best, matched, n_joints = dist, pid, cnt
        if n_joints == 0 or best / n_joints > 1.:
            matched = -1
        if matched < 0:
            matched = len(founders)
            founders.append(s)
        labels[s] = matched
    skip = not founders or not bool(np.all(np.asarray(m1[:n]) != 0))
    return labels, len(founders), skip


# ---- scores ------------------------------------------------------------------------------------------------------------
def partition_scores(labels_true, labels_pred):
    """-> (ari, homogeneity, completeness, v_measure), float64."""
    lt, lp = np.asarray(labels_true).reshape(-1), np.asarray(labels_pred).reshape(-1)
    n = len(lt)
    if len(lp) != n:
        raise ValueError('partition_scores: %d true labels, %d predicted' % (n, len(lp)))
    if n == 0:
        return 1.0, 1.0, 1.0, 1.0
    _, ti = np.unique(lt, return_inverse=True)
    _, pi = np.unique(lp, return_inverse=True)
    ti, pi = ti.reshape(-1), pi.reshape(-1)
    a = [int(x) for x in np.bincount(ti)]
    b = [int(x) for x in np.bincount(pi)]
    cells = {}
    for i, j in zip(ti.tolist(), pi.tolist()):
        cells[(i, j)] = cells.get((i, j), 0) + 1
    ss = sum(c * c for c in cells.values())
    tp = ss - n
    fp = sum(x * x for x in b) - ss
    fn = sum(x * x for x in a) - ss
    tn = n * n - fp - fn - ss
    if fn == 0 and fp == 0:
        ari = 1.0
    else:
        ari = 2.0 * (tp * tn - fn * fp) / ((tp + fn) * (fn + tn) + (tp + fp) * (fp + tn))
    lg = log_table(n * n)
    log_n = float(lg[n - 1])

    def entropy(counts):
        if len(counts) == 1:
            return 0.0
        acc = 0.0
        for c in counts:
            acc = acc + (float(c) / float(n)) * (float(lg[c - 1]) - log_n)
        return -acc

    h_true, h_pred = entropy(a), entropy(b)
    mi = 0.0
    if len(a) > 1 and len(b) > 1:
        acc = 0.0
        for (i, j) in sorted(cells):
            nij = cells[(i, j)]
            nm = float(nij) / float(n)
            t = nm * (float(lg[nij - 1]) - log_n) + nm * (((-float(lg[a[i] * b[j] - 1])) + log_n) + log_n)
            if abs(t) < EPS:
                t = 0.0
            acc = acc + t
        mi = acc if acc > 0.0 else 0.0
    h = mi / h_true if h_true else 1.0
    c = mi / h_pred if h_pred else 1.0
    v = 0.0 if h + c == 0.0 else ((2.0 * h) * c) / (h + c)
    return float(ari), float(h), float(c), float(v)


def batch_scores(labels_true, labels_pred, count, skip=None, count_true=None):
    """partition_scores over the frames of a batch, as mpe_partition_scores returns them: labels [B,Hcap], count [B] ->
    [B,4] float64, NaN for a frame with count 0, with skip set or with another count on the true side."""
    B = len(count)
    out = np.full((B, 4), np.nan, np.float64)
    for f in range(B):
        n = int(count[f])
        if n <= 0 or (skip is not None and skip[f]) or (count_true is not None and int(count_true[f]) != n):
            continue
        out[f] = partition_scores(labels_true[f][:n], labels_pred[f][:n])
    return out
