"""numpy statement of what mpe_track_batch computes (csrc/track.hip): one identity per person over the frames of a
sequence.  The engine's poses[n_frames][Pcap][J][3] carry no identity -- row p of one frame is not row p of the next --
and neither do the reference's (its viewers colour people by `person_id = enumerate(final_output)`,
test/show_results_from_model.py:276,321,329).  The tests hold the kernel to `track_sequence`, which is written as the
online loop -- one frame at a time against the frames before it -- while the device works on all frames of a batch at
once, one cascade stage per launch: that the two agree is part of what they check.

The rule -- the contract of the device path:

Detections.  As in mpe_eval_batch.  Mode 'mlp': float32 poses, persons p < n_persons[f] with flags[f, p] != 0, every
joint present.  Mode 'tri': float64 poses, every p < n_persons[f], joint j present when flags[f, p, j] != 0.  Only
used joints count; a person with no present used joint is not a detection (id -1, cost -1.0, gap -1).

Cost of a newer detection a against an older one b: over the used joints both have, in increasing j, the stored
coordinates widened to float64: dx, dy, dz = a - b; s = dx*dx; s = s + dy*dy; s = s + dz*dz, every product and sum
rounded on its own; d = sqrt(s), correctly rounded; the left-fold sum of d divided by the count.  +inf without a common
joint.  A pair is linkable when cost < gate (strict; a NaN never links).

Cascade.  For g = 1 .. max_gap + 1 (the tracks seen last choose first): rows = the detections of the frame that have no
parent yet, columns = the detections of the frame g frames back that have no child yet; take the linkable pair of least
cost, ties to the lowest row, then the lowest column (detection order), link it, remove both, until none is left.

Ids.  A detection without a parent starts a track: consecutive integers in birth order (frame, then detection order)
from the count in the state; every other detection takes its parent's id.

State.  The detections of the last max_gap + 1 frames with their ids and has-child marks, and the count: a sequence
fed in any chunking gets the same ids.
"""
import numpy as np


def detections_of(poses_f, flags_f, n, mode, used):
    """-> [(row, pose [J,3] float64, present-and-used [J] bool)] of one frame, in detection order."""
    out = []
    J = poses_f.shape[1]
    for p in range(max(0, min(int(n), poses_f.shape[0]))):
        if mode == 'mlp':
            m = used.copy() if flags_f[p] else np.zeros(J, bool)
        else:
            m = (np.asarray(flags_f[p]) != 0) & used
        if m.any():
            out.append((p, poses_f[p].astype(np.float64), m))
    return out


def cost_table(rows, cols):
    """[R,C] float64 of the costs above; rows / cols: lists of (pose [J,3] float64, mask [J])."""
    a = np.stack([r[0] for r in rows])[:, None]
    b = np.stack([c[0] for c in cols])[None]
    both = np.stack([r[1] for r in rows])[:, None] & np.stack([c[1] for c in cols])[None]
    d = a - b
    s = d[..., 0] * d[..., 0]
    s = s + d[..., 1] * d[..., 1]
    s = s + d[..., 2] * d[..., 2]
    nrm = np.sqrt(s)
    tot = np.zeros(both.shape[:2])
    for j in range(both.shape[2]):
        tot = np.where(both[..., j], tot + nrm[..., j], tot)
    n = both.sum(axis=2)
    with np.errstate(invalid='ignore', divide='ignore'):
        return np.where(n > 0, tot / np.maximum(n, 1), np.inf)


def new_state():
    return {'frames': [], 'issued': 0}


def track_sequence(poses, flags, n_persons, mode, used_joints, gate, max_gap, state=None):
    """The online cascade over the frames of `poses` [B,Pcap,J,3] -> {'ids' [B,Pcap] int32, 'cost' [B,Pcap] float64,
    'gap' [B,Pcap] int32, 'issued': ids issued so far, 'state': what the next call continues from}.  `state` is a
    former call's (it is not modified); None starts a sequence."""
    if mode not in ('mlp', 'tri'):
        raise ValueError('mode must be mlp or tri')
    poses, flags = np.asarray(poses), np.asarray(flags)
    B, pcap, J = poses.shape[:3]
    used = np.isin(np.arange(J), list(used_joints))
    H = int(max_gap) + 1
    st = new_state() if state is None else state
    history = [[dict(d) for d in fr] for fr in st['frames']]
    issued = int(st['issued'])
    ids = np.full((B, pcap), -1, np.int32)
    cost = np.full((B, pcap), -1.0)
    gap = np.full((B, pcap), -1, np.int32)
    for f in range(B):
        dets = [{'row': p, 'pose': x, 'mask': m, 'parent': None, 'child': False, 'id': -1}
                for p, x, m in detections_of(poses[f], flags[f], n_persons[f], mode, used)]
        for d in dets:
            gap[f, d['row']] = 0
        for g in range(1, H + 1):
            if g > len(history):
                break
            rows = [d for d in dets if d['parent'] is None]
            cols = [c for c in history[-g] if not c['child']]
            if not rows or not cols:
                continue
            table = cost_table([(d['pose'], d['mask']) for d in rows], [(c['pose'], c['mask']) for c in cols])
            open_ = np.where(table < gate, table, np.inf)          # what is neither linkable nor free any more: +inf
            while True:
                r, c = divmod(int(np.argmin(open_)), len(cols))     # the first minimum in row-major order: lowest row, then column
                best = open_[r, c]
                if not best < np.inf:
                    break
                open_[r, :] = np.inf
                open_[:, c] = np.inf
                rows[r]['parent'] = cols[c]
                cols[c]['child'] = True
                gap[f, rows[r]['row']] = g
                cost[f, rows[r]['row']] = best
        for d in dets:
            if d['parent'] is None:
                d['id'] = issued
                issued += 1
            else:
                d['id'] = d['parent']['id']
            ids[f, d['row']] = d['id']
        history = (history + [dets])[-H:]
    keep = [[{'row': d['row'], 'pose': d['pose'], 'mask': d['mask'], 'parent': None, 'child': d['child'], 'id': d['id']} for d in fr]
            for fr in history]
    return {'ids': ids, 'cost': cost, 'gap': gap, 'issued': issued, 'state': {'frames': keep, 'issued': issued}}


class TrackSummary:
    """Tracks of a sequence from the ids and gaps of its chunks, in order."""

    def __init__(self):
        self.length = {}
        self.frames = 0
        self.late_births = 0

    def add(self, ids, gap):
        ids, gap = np.asarray(ids), np.asarray(gap)
        for f in range(ids.shape[0]):
            for i in ids[f][ids[f] >= 0]:
                self.length[int(i)] = self.length.get(int(i), 0) + 1
            if self.frames > 0:
                self.late_births += int((gap[f] == 0).sum())
            self.frames += 1

    def result(self):
        """-> {'tracks', 'mean_length' (frames a track is seen in), 'late_births' (births after the first frame)}"""
        n = len(self.length)
        return {'tracks': n, 'mean_length': float(sum(self.length.values())) / n if n else 0.0, 'late_births': self.late_births}
