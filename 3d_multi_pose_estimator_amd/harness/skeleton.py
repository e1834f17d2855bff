"""numpy statement of what mpe_skel_observe_batch / mpe_skel_update / mpe_skel_fit_batch compute (csrc/skel.hip): bone
lengths held constant along a track.  The tracker (mpe_track_batch, harness/tracking.py) says which rows are one body over
time; the lengths of that body's bones are learned from its own frames and every pose of the track is then moved, within
its own frame, towards them.  The tests hold the kernels to `observe_sequence`, `length_table` and `fit_sequence`, bit for
bit.  Everything below is a plain loop over numpy float64 scalars in the stated order.

The rule -- the contract of the device path:

State.  tid_cap track ids, a bone list of (parent, child) joint pairs, a bin width in metres.  hist uint32
[tid_cap, n_bones, BINS]; len float64 and count int32 [tid_cap, n_bones]; the counters out_of_range and over_ids; the
sticky status word.

Detections, presence, activity.  As in mpe_smooth_batch.  Row p of frame f is a detection when p < n_persons[f],
ids[f, p] >= 0 and, in mode 'mlp', flags[f, p] != 0.  Mode 'mlp': float32 poses, every joint of a detection is present.
Mode 'tri': float64 poses, joint j is present when flags[f, p, j] != 0.  A joint is ACTIVE when it is present, inside
joint_mask and its three stored coordinates are finite; a bone is LIVE in a row when both its joints are active.
Coordinates are widened to float64.

Length of a bone from coordinates x.  d = x_child - x_parent; s = (dx*dx + dy*dy) + dz*dz; l = sqrt(s), every operation
rounded on its own.

observe.  For every detection with id t < tid_cap and every live bone b: l from the stored coordinates, q = l / bin_width;
when l > 0 and q < BINS, hist[t, b, int(q)] += 1, otherwise out_of_range += 1.  A detection with t >= tid_cap adds 1 to
over_ids (once per row) and sets OVER_IDS; it reaches neither hist nor out_of_range.  Only integers are added: the state
does not depend on chunking or frame order.

update(min_samples).  For every (t, b): n = hist[t, b].sum(), count = n.  n < max(min_samples, 1): len = 0.0, no length.
Otherwise k* = the smallest k with 2 * hist[t, b, :k + 1].sum() >= n (the lower median), len = (float(k*) + 0.5) * bin_width.
set_lengths puts a caller's table in the place of len as it is; an entry has a length when it is > 0 and finite.

fit(iters).  Every (frame, row) on its own.  A bone is CONSTRAINED in a row when it is live and len[t, b] has a length; a
row is PROCESSED when it is a detection with t < tid_cap and a constrained bone.  The working copy x holds the joints in
float64.  For sweep = 1 .. iters, for each constrained bone in LIST ORDER with L = len[t, b]: l from x; unless l > 0 the
bone is skipped; e = (l - L) / l; h = 0.5 * e; per axis a, with d taken before any update of this bone: m = h * d[a];
x[parent, a] = x[parent, a] + m; x[child, a] = x[child, a] - m.
poses: a joint that is an end of a constrained bone of a processed row gets its working value rounded once to the pose
type; every other joint and every other row is copied through bit for bit.  err[f, p] = (e0, e1): the left fold from 0.0
over the constrained bones in list order of `if v > m: m = v` with v = |l - L|, l from the stored input (e0) and from the
final working values before rounding (e1); both -1.0 for a row that is not processed.  n_bones[f, p] = the constrained
bones, 0 for a row that is not processed.  The fit changes nothing in the state.
"""
import numpy as np

BINS = 512
MAX_BONES = 32
MAX_ITERS = 64
OVER_IDS = 1
MAX_HIST_BYTES = 256 << 20

# OpenPose-style 18 joints as the package's joint_list names them: nose 0, eyes 1 2, ears 3 4, shoulders 5 6, elbows 7 8,
# wrists 9 10, hips 11 12, knees 13 14, ankles 15 16, neck 17.  (parent, child), every parent before its subtree: a sweep
# runs from the neck outwards.
BONES_18 = ((17, 0), (0, 1), (0, 2), (1, 3), (2, 4), (17, 5), (17, 6), (5, 7), (6, 8), (7, 9), (8, 10), (17, 11), (17, 12),
            (11, 12), (11, 13), (12, 14), (13, 15), (14, 16))


def check_bones(bones, n_joints):
    """-> the bone list as int32 [n_bones, 2]; ValueError where mpe_skel_create would decline it"""
    b = np.asarray(bones, np.int64)
    if b.ndim != 2 or b.shape[1] != 2 or not 1 <= len(b) <= MAX_BONES:
        raise ValueError('bones must be 1 .. %d (parent, child) pairs' % MAX_BONES)
    if (b < 0).any() or (b >= n_joints).any() or (b[:, 0] == b[:, 1]).any():
        raise ValueError('every bone joins two different joints within 0 .. %d' % (n_joints - 1))
    return b.astype(np.int32)


def new_state(tid_cap, bones, bin_width, n_joints=18):
    bones = check_bones(bones, n_joints)
    bin_width = np.float64(bin_width)
    if not (np.isfinite(bin_width) and bin_width > 0) or tid_cap < 1:
        raise ValueError('bin_width must be finite and > 0, tid_cap at least 1')
    if tid_cap * len(bones) * BINS * 4 > MAX_HIST_BYTES:
        raise ValueError('the histogram of %d ids x %d bones is over %d bytes' % (tid_cap, len(bones), MAX_HIST_BYTES))
    nb = len(bones)
    return {'tid_cap': int(tid_cap), 'bones': bones, 'bin_width': bin_width, 'hist': np.zeros((tid_cap, nb, BINS), np.uint32),
            'len': np.zeros((tid_cap, nb)), 'count': np.zeros((tid_cap, nb), np.int32), 'out_of_range': 0, 'over_ids': 0, 'status': 0}


def _rows(poses, flags, n_persons, ids, mode, joint_mask):
    """every detection of the sequence -> (f, p, id, active [J] bool)"""
    if mode not in ('mlp', 'tri'):
        raise ValueError('mode must be mlp or tri')
    B, pcap, J = poses.shape[:3]
    in_mask = np.array([(int(joint_mask) >> j) & 1 for j in range(J)], bool)
    for f in range(B):
        for p in range(max(0, min(int(n_persons[f]), pcap))):
            t = int(ids[f, p])
            if t < 0 or (mode == 'mlp' and not flags[f, p]):
                continue
            present = np.ones(J, bool) if mode == 'mlp' else flags[f, p] != 0
            yield f, p, t, present & in_mask & np.isfinite(poses[f, p]).all(axis=1)


def _length(x, jp, jc):
    """x [J,3] float64 -> (d [3], l), every operation rounded on its own"""
    d = [x[jc, a] - x[jp, a] for a in range(3)]
    s = (d[0] * d[0] + d[1] * d[1]) + d[2] * d[2]
    return d, np.sqrt(s)


def observe_sequence(state, poses, flags, n_persons, ids, mode, joint_mask):
    """adds the frames to state['hist'] and the counters (in place) -> state"""
    poses, flags, ids = np.asarray(poses), np.asarray(flags), np.asarray(ids)
    bones, w = state['bones'], state['bin_width']
    with np.errstate(all='ignore'):
        for f, p, t, active in _rows(poses, flags, n_persons, ids, mode, joint_mask):
            if t >= state['tid_cap']:
                state['over_ids'] += 1
                state['status'] |= OVER_IDS
                continue
            x = poses[f, p].astype(np.float64)
            for b, (jp, jc) in enumerate(bones):
                if not (active[jp] and active[jc]):
                    continue
                _, l = _length(x, jp, jc)
                q = l / w
                if l > 0 and q < BINS:
                    state['hist'][t, b, int(q)] += 1
                else:
                    state['out_of_range'] += 1
    return state


def length_table(state, min_samples=10):
    """the lower median of every histogram into state['len'] / state['count'] (in place) -> state"""
    hist, w = state['hist'], state['bin_width']
    need = max(int(min_samples), 1)
    total = hist.sum(axis=2, dtype=np.uint64)
    state['count'][...] = np.minimum(total, 2 ** 31 - 1)
    state['len'][...] = 0.0
    for t in range(hist.shape[0]):
        for b in range(hist.shape[1]):
            n = int(total[t, b])
            if n < need:
                continue
            cum = 0
            for k in range(BINS):
                cum += int(hist[t, b, k])
                if 2 * cum >= n:
                    state['len'][t, b] = (np.float64(k) + np.float64(0.5)) * w
                    break
    return state


def set_lengths(state, table):
    """a caller's table [tid_cap, n_bones] in the place of state['len'], as it is -> state"""
    table = np.asarray(table, np.float64)
    if table.shape != state['len'].shape:
        raise ValueError('the table must be %s' % (state['len'].shape,))
    state['len'] = table.copy()
    return state


def fit_sequence(state, poses, flags, n_persons, ids, mode, joint_mask, iters=16):
    """-> {'poses' (the type and shape of poses), 'err' [B,Pcap,2] float64, 'n_bones' [B,Pcap] uint8}; the state is read only"""
    if not 1 <= int(iters) <= MAX_ITERS:
        raise ValueError('iters is within 1 .. %d' % MAX_ITERS)
    poses, flags, ids = np.asarray(poses), np.asarray(flags), np.asarray(ids)
    B, pcap = poses.shape[:2]
    bones, table = state['bones'], state['len']
    out = poses.copy()
    err = np.full((B, pcap, 2), -1.0)
    n_bones = np.zeros((B, pcap), np.uint8)
    half = np.float64(0.5)
    with np.errstate(all='ignore'):
        for f, p, t, active in _rows(poses, flags, n_persons, ids, mode, joint_mask):
            if t >= state['tid_cap']:
                continue
            con = [(int(jp), int(jc), table[t, b]) for b, (jp, jc) in enumerate(bones)
                   if active[jp] and active[jc] and table[t, b] > 0 and np.isfinite(table[t, b])]
            if not con:
                continue
            x = poses[f, p].astype(np.float64)

            def worst():
                m = np.float64(0.0)
                for jp, jc, L in con:
                    v = np.abs(_length(x, jp, jc)[1] - L)
                    if v > m:
                        m = v
                return m
            err[f, p, 0] = worst()
            for _ in range(int(iters)):
                for jp, jc, L in con:
                    d, l = _length(x, jp, jc)
                    if not l > 0:
                        continue
                    e = (l - L) / l
                    h = half * e
                    for a in range(3):
                        m = h * d[a]
                        x[jp, a] = x[jp, a] + m
                        x[jc, a] = x[jc, a] - m
            err[f, p, 1] = worst()
            n_bones[f, p] = len(con)
            for j in sorted({j for jp, jc, _ in con for j in (jp, jc)}):
                out[f, p, j] = x[j].astype(poses.dtype)
    return {'poses': out, 'err': err, 'n_bones': n_bones}


class SkeletonSummary:
    """What the fit did to a sequence, from the inputs and outputs of its chunks and the last length table."""

    def __init__(self):
        self.rows = self.bones = 0
        self.err0 = self.err1 = self.moved = 0.0
        self.max0 = self.max1 = 0.0
        self.joints = 0

    def add(self, poses_in, out):
        """rows: the processed rows; bones: their constrained bones; the length error is the rows' worst bone before and
        after (err); moved: the joints whose bits changed."""
        p0, p1 = np.asarray(poses_in, np.float64), np.asarray(out['poses'], np.float64)
        err, nb = np.asarray(out['err']), np.asarray(out['n_bones'])
        sel = nb > 0
        self.rows += int(sel.sum())
        self.bones += int(nb.sum())
        if sel.any():
            e0, e1 = err[..., 0][sel], err[..., 1][sel]
            e0, e1 = e0[np.isfinite(e0)], e1[np.isfinite(e1)]
            self.err0 += float(e0.sum())
            self.err1 += float(e1.sum())
            self.max0 = max([self.max0] + e0.tolist())
            self.max1 = max([self.max1] + e1.tolist())
        d = p1 - p0
        changed = sel[..., None] & np.isfinite(d).all(axis=3) & (d != 0).any(axis=3)
        self.joints += int(changed.sum())
        self.moved += float(np.sqrt((d[changed] ** 2).sum(axis=1)).sum())

    def result(self, lengths=None):
        """lengths: Skeleton.lengths()'s dict or a state of this module -> {'tracks' (ids with a length), 'rows', 'bones',
        'over_ids' (observed rows whose id the tables do not hold: neither learned nor fitted), 'out_of_range' (lengths
        no bin holds), 'err_mean_mm' / 'err_max_mm' [before, after] (over the fitted rows' worst bone), 'mean_move_mm'
        (over the joints that moved)}"""
        tracks = over_ids = out_of_range = 0
        if lengths is not None:
            table = np.asarray(lengths['len'])
            tracks = int(((table > 0) & np.isfinite(table)).any(axis=1).sum())
            over_ids, out_of_range = int(lengths['over_ids']), int(lengths['out_of_range'])
        n = max(self.rows, 1)
        return {'tracks': tracks, 'rows': self.rows, 'bones': self.bones, 'over_ids': over_ids, 'out_of_range': out_of_range,
                'err_mean_mm': [1000.0 * self.err0 / n, 1000.0 * self.err1 / n], 'err_max_mm': [1000.0 * self.max0, 1000.0 * self.max1],
                'mean_move_mm': 1000.0 * self.moved / self.joints if self.joints else 0.0}


def report_line(iters, bin_mm, min_samples, r):
    """the harness's line; what was left out is appended when there is any"""
    left_out = ''.join(', %d %s' % (r[k], what) for k, what in (('over_ids', 'rows over the id capacity'), ('out_of_range', 'lengths out of range'))
                       if r.get(k))
    return ('Bones (%d sweeps, bin %g mm, min %d): %d tracks, %d rows, %d bones, length error mean/max %.3f/%.3f -> %.3f/%.3f mm, '
            'mean move %.3f mm' % (iters, bin_mm, min_samples, r['tracks'], r['rows'], r['bones'], r['err_mean_mm'][0], r['err_max_mm'][0],
                                   r['err_mean_mm'][1], r['err_max_mm'][1], r['mean_move_mm']) + left_out)
