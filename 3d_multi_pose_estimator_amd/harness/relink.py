"""numpy statement of what mpe_relink_batch computes (csrc/relink.hip): a person who comes back after a long gap gets
the identity they had.  The tracker (mpe_track_batch, harness/tracking.py) links a detection only a few frames back and
only within its gate; a person who walks behind a pillar, leaves the volume or is lost by the matcher for a dozen frames
returns under a new id.  The lengths of a body's bones survive a gap of any length and any distance: a newborn track
takes the id of a lost track with the same bone lengths and, optionally, a plausible position.  The stage sits between
the tracker and everything that reads its ids; it is causal (an id handed out is never revised) and needs no weights.
The tests hold the kernels to `relink_sequence`, bit for bit.  Everything below is a plain loop over numpy float64
scalars in the stated order.

The rule -- the contract of the device path:

Options (DEFAULTS; all finite, checked by check_options).  The defaults are options, not findings: they suit noise of a
few millimetres per joint and bodies whose statures differ by a few per cent, and nothing here measures either.
  gate_m 0.02             a link needs a bone-length cost strictly below this
  min_gap 4               fewest frames since the lost track was last seen (the harness passes track_gap + 2)
  max_gap 150             most frames since it was last seen
  min_samples 5           a record's bone counts only with this many lengths
  min_bones 8             fewest bones a birth and a record must have in common
  max_bone_m 1.0          longest length that is accepted
  reach_m 0.0             0: no position gate
  reach_per_frame_m 0.0   growth of the position gate per frame of gap
  used_joint_mask         joints the position gate looks at (default: parameters.used_joints)
  joint_mask              joints that count at all (default: all)
  tid_cap 256             ids 0 .. tid_cap - 1 have a record, 1 .. MAX_TID_CAP

State of a sequence.  frame: the frames seen.  canon int32 [tid_cap], -1 until the id has been seen.  One record per
canonical id: last_frame (-1: none), last_pose float64 [J,3] with its active-joint mask, sum float64 [n_bones], cnt int32
[n_bones].  The counters births, linked, over_ids; the sticky status word (OVER_IDS).

Detections, presence, activity, live bones, the length of a bone.  Word for word harness/skeleton.py: row p of frame f is
a detection when p < n_persons[f], ids[f, p] >= 0 and, in mode 'mlp', flags[f, p] != 0; mode 'mlp': float32 poses, every
joint of a detection present; mode 'tri': float64 poses, joint j present when flags[f, p, j] != 0.  A joint is ACTIVE when
it is present, inside joint_mask and its three stored coordinates are finite; a bone is LIVE when both its joints are
active.  d = x_child - x_parent; s = (dx*dx + dy*dy) + dz*dz; l = sqrt(s), every operation rounded on its own.  A length
is ACCEPTED when the bone is live, l > 0 and l <= max_bone_m.

Per frame, in order; f counts over the whole sequence, an empty frame counts too.
 1. A detection with t >= tid_cap keeps its id, adds 1 to over_ids and sets OVER_IDS.  It takes no further part.
 2. A detection with canon[t] >= 0 is KNOWN and its record canon[t] is PRESENT in this frame.  Every other detection is
    a BIRTH.  Ids are unique within a frame as the tracker gives them; a later row that repeats an id gets the same
    output id and touches nothing.
 3. Rows: the births in row order.  Columns: the records c in increasing canonical id with last_frame >= 0, not present
    in this frame and min_gap <= g <= max_gap, g = f - last_frame.
 4. Cost of (row, column) over the bones in list order: a bone counts when it has an accepted length l in the birth and
    cnt >= min_samples in the record; m = sum / float(cnt); v = |l - m|; the cost is the left fold of v from 0.0 divided
    by the count of such bones, +inf with fewer than min_bones of them.
 5. Position gate, when reach_m > 0: d = the tracker's pair cost (harness/tracking.py, "Cost of a newer detection")
    between the birth's pose and last_pose over the joints active in both and inside used_joint_mask; the pair is kept
    only when d < reach_m + reach_per_frame_m * float(g), every operation rounded on its own; a pair with no common
    joint is not kept.
 6. A pair is linkable when its cost < gate_m (strict; a NaN never links).
 7. Greedy, as in the tracker: the linkable pair of least cost, ties to the lowest row and then the lowest column, is
    linked and both are removed, until none is left.
 8. A linked birth t -> c: canon[t] = c; link_cost and link_gap = g are written for that row; linked += 1.
 9. An unlinked birth: canon[t] = t; births += 1.
10. Then every detection with t < tid_cap, taking the FIRST row of each canonical id (two tracker ids that one record
    stands for can both be in a frame when min_gap is no longer than the tracker's own gap; the later row touches
    nothing), updates its record: per accepted bone sum = sum + l and cnt += 1; last_pose and its mask are replaced by
    this row's active joints; last_frame = f.

Outputs.  ids int32 [B,Pcap]: canon[t]; -1 where the input has no detection; t itself for t >= tid_cap.  link_cost
float64 [B,Pcap]: -1.0 unless the row is a linked birth.  link_gap int32 [B,Pcap]: the gap of a linked birth, 0 for any
other detection, -1 for no detection.  counters int64 [3] = births, linked, over_ids; status.

A canonical id is always a tracker id and never larger than the id it replaces (a record exists before the birth that
takes it), so the tid_cap / gid_cap sizing of the later stages is unaffected.
"""
import numpy as np

from . import skeleton as S

OVER_IDS = 1
MAX_TID_CAP = 4096
MAX_GAP = 1 << 30
USED_JOINTS_18 = (0, 5, 6, 7, 8, 9, 10, 11, 12, 13, 14, 15, 16, 17)      # parameters.used_joints
DEFAULTS = {'gate_m': 0.02, 'min_gap': 4, 'max_gap': 150, 'min_samples': 5, 'min_bones': 8, 'max_bone_m': 1.0, 'reach_m': 0.0,
            'reach_per_frame_m': 0.0, 'used_joint_mask': sum(1 << j for j in USED_JOINTS_18), 'joint_mask': 0xFFFFFFFF, 'tid_cap': 256}
_INTS = ('min_gap', 'max_gap', 'min_samples', 'min_bones', 'used_joint_mask', 'joint_mask', 'tid_cap')


def check_options(options=None, n_bones=None):
    """-> the options with the defaults filled in; ValueError where mpe_relink_create would decline them"""
    o = dict(DEFAULTS)
    for k, v in (options or {}).items():
        if k not in DEFAULTS:
            raise ValueError('unknown option %r' % (k,))
        o[k] = v
    for k in DEFAULTS:
        if not np.isfinite(float(o[k])):
            raise ValueError('%s must be finite' % k)
        if k in _INTS:
            if int(o[k]) != o[k]:
                raise ValueError('%s must be an integer' % k)
            o[k] = int(o[k])
        else:
            o[k] = float(o[k])
    if not o['gate_m'] > 0 or not o['max_bone_m'] > 0 or o['reach_m'] < 0 or o['reach_per_frame_m'] < 0:
        raise ValueError('gate_m and max_bone_m are > 0, reach_m and reach_per_frame_m not negative')
    if not 1 <= o['min_gap'] <= o['max_gap'] <= MAX_GAP:
        raise ValueError('1 <= min_gap <= max_gap <= %d' % MAX_GAP)
    if o['min_samples'] < 1 or o['min_bones'] < 1 or (n_bones is not None and o['min_bones'] > n_bones):
        raise ValueError('min_samples is at least 1, min_bones within 1 .. the bones')
    if not 1 <= o['tid_cap'] <= MAX_TID_CAP:
        raise ValueError('tid_cap is within 1 .. %d' % MAX_TID_CAP)
    if not 0 <= o['used_joint_mask'] <= 0xFFFFFFFF or not 0 <= o['joint_mask'] <= 0xFFFFFFFF:
        raise ValueError('the joint masks are 32-bit')
    return o


def new_state(tid_cap, n_bones, n_joints=18):
    return {'frame': 0, 'canon': np.full(tid_cap, -1, np.int32), 'last_frame': np.full(tid_cap, -1, np.int64),
            'last_pose': np.zeros((tid_cap, n_joints, 3)), 'last_mask': np.zeros((tid_cap, n_joints), bool),
            'sum': np.zeros((tid_cap, n_bones)), 'cnt': np.zeros((tid_cap, n_bones), np.int32),
            'births': 0, 'linked': 0, 'over_ids': 0, 'status': 0}


def _copy_state(st):
    return {k: (v.copy() if isinstance(v, np.ndarray) else v) for k, v in st.items()}


def bone_cost(lengths, rec_sum, rec_cnt, min_samples, min_bones):
    """step 4: lengths [n_bones] of the birth (nan: not accepted) against a record's sums and counts"""
    tot, n = np.float64(0.0), 0
    for b in range(len(lengths)):
        if lengths[b] == lengths[b] and rec_cnt[b] >= min_samples:
            m = rec_sum[b] / np.float64(rec_cnt[b])
            tot = tot + np.abs(lengths[b] - m)
            n += 1
    return tot / np.float64(n) if n >= min_bones else np.float64(np.inf)


def pose_cost(xa, ma, xb, mb):
    """step 5: the tracker's pair cost of the newer pose xa against the older xb over the joints of both masks"""
    tot, n = np.float64(0.0), 0
    for j in range(len(ma)):
        if ma[j] and mb[j]:
            dx, dy, dz = xa[j, 0] - xb[j, 0], xa[j, 1] - xb[j, 1], xa[j, 2] - xb[j, 2]
            s = dx * dx
            s = s + dy * dy
            s = s + dz * dz
            tot = tot + np.sqrt(s)
            n += 1
    return tot / np.float64(n) if n else np.float64(np.inf)


def relink_sequence(poses, flags, n_persons, ids, mode, bones, options=None, state=None):
    """The frames of `poses` [B,Pcap,J,3] with the tracker's `ids` [B,Pcap] -> ({'ids' int32 [B,Pcap], 'link_cost' float64
    [B,Pcap], 'link_gap' int32 [B,Pcap], 'counters' int64 [3] (births, linked, over_ids), 'status'}, the state the next
    call continues from).  `state` is a former call's (it is not modified); None starts a sequence."""
    poses, flags, ids = np.asarray(poses), np.asarray(flags), np.asarray(ids)
    B, pcap, J = poses.shape[:3]
    bones = S.check_bones(bones, J)
    o = check_options(options, len(bones))
    tid_cap, nb = o['tid_cap'], len(bones)
    st = new_state(tid_cap, nb, J) if state is None else _copy_state(state)
    if len(st['canon']) != tid_cap or st['sum'].shape[1] != nb:
        raise ValueError('the state was made for another tid_cap or bone list')
    used = np.array([(o['used_joint_mask'] >> j) & 1 for j in range(J)], bool)
    gate, max_bone = np.float64(o['gate_m']), np.float64(o['max_bone_m'])
    reach, speed = np.float64(o['reach_m']), np.float64(o['reach_per_frame_m'])
    out_ids = np.full((B, pcap), -1, np.int32)
    cost = np.full((B, pcap), -1.0)
    gap = np.full((B, pcap), -1, np.int32)
    by_frame = [[] for _ in range(B)]
    for f, p, t, active in S._rows(poses, flags, n_persons, ids, mode, o['joint_mask']):
        by_frame[f].append((p, t, active))
    canon, last_frame = st['canon'], st['last_frame']
    with np.errstate(all='ignore'):
        for fl in range(B):
            f = st['frame']
            dets, births, present, seen_id = [], [], set(), set()
            for p, t, active in by_frame[fl]:
                gap[fl, p] = 0
                if t >= tid_cap:                             # 1
                    out_ids[fl, p] = t
                    st['over_ids'] += 1
                    st['status'] |= OVER_IDS
                    continue
                x = poses[fl, p].astype(np.float64)
                lengths = np.full(nb, np.nan)
                for b, (jp, jc) in enumerate(bones):
                    if active[jp] and active[jc]:
                        l = S._length(x, jp, jc)[1]
                        if l > 0 and l <= max_bone:
                            lengths[b] = l
                d = {'row': p, 't': t, 'x': x, 'active': active, 'len': lengths, 'first': t not in seen_id}
                seen_id.add(t)
                dets.append(d)
                if canon[t] >= 0:                            # 2
                    present.add(int(canon[t]))
                elif d['first']:
                    births.append(d)
            cols = [c for c in range(tid_cap)                # 3
                    if last_frame[c] >= 0 and c not in present and o['min_gap'] <= f - last_frame[c] <= o['max_gap']]
            if births and cols:
                table = np.full((len(births), len(cols)), np.inf)
                for r, d in enumerate(births):
                    for k, c in enumerate(cols):
                        v = bone_cost(d['len'], st['sum'][c], st['cnt'][c], o['min_samples'], o['min_bones'])    # 4
                        if reach > 0:                        # 5
                            g = np.float64(f - last_frame[c])
                            dist = pose_cost(d['x'], d['active'] & used, st['last_pose'][c], st['last_mask'][c] & used)
                            if not dist < reach + speed * g:
                                continue
                        if v < gate:                         # 6
                            table[r, k] = v
                while True:                                  # 7
                    r, k = divmod(int(np.argmin(table)), len(cols))
                    best = table[r, k]
                    if not best < np.inf:
                        break
                    table[r, :] = np.inf
                    table[:, k] = np.inf
                    d, c = births[r], cols[k]
                    canon[d['t']] = c                        # 8
                    cost[fl, d['row']] = best
                    gap[fl, d['row']] = f - last_frame[c]
                    st['linked'] += 1
            for d in births:                                 # 9
                if canon[d['t']] < 0:
                    canon[d['t']] = d['t']
                    st['births'] += 1
            updated = set()
            for d in dets:                                   # 10
                c = int(canon[d['t']])
                out_ids[fl, d['row']] = c
                if c in updated:
                    continue
                updated.add(c)
                for b in range(nb):
                    if d['len'][b] == d['len'][b]:
                        st['sum'][c, b] = st['sum'][c, b] + d['len'][b]
                        st['cnt'][c, b] += 1
                st['last_pose'][c] = np.where(d['active'][:, None], d['x'], 0.0)
                st['last_mask'][c] = d['active']
                last_frame[c] = f
            st['frame'] = f + 1
    counters = np.array([st['births'], st['linked'], st['over_ids']], np.int64)
    return {'ids': out_ids, 'link_cost': cost, 'link_gap': gap, 'counters': counters, 'status': st['status']}, st


class RelinkSummary:
    """What the relinker did to a sequence, from the tracker's ids and the outputs of its chunks, in order."""

    def __init__(self):
        self.before, self.after = set(), set()
        self.gap_sum = self.gap_max = self.links = 0

    def add(self, track_ids, out):
        t, i, g = np.asarray(track_ids), np.asarray(out['ids']), np.asarray(out['link_gap'])
        self.before.update(t[t >= 0].tolist())
        self.after.update(i[i >= 0].tolist())
        linked = g[g > 0]
        self.links += int(linked.size)
        self.gap_sum += int(linked.sum())
        self.gap_max = max([self.gap_max] + linked.tolist())

    def result(self, counters):
        """counters: Relinker.counters()'s dict or a statement's output -> {'births', 'links', 'tracks_before',
        'tracks_after', 'mean_gap', 'max_gap', 'over_ids'}"""
        if 'counters' in counters:
            births, linked, over_ids = (int(v) for v in counters['counters'])
        else:
            births, linked, over_ids = int(counters['births']), int(counters['linked']), int(counters['over_ids'])
        return {'births': births, 'links': linked, 'tracks_before': len(self.before), 'tracks_after': len(self.after),
                'mean_gap': float(self.gap_sum) / self.links if self.links else 0.0, 'max_gap': int(self.gap_max), 'over_ids': over_ids}


def report_line(gate_mm, max_gap, r):
    """the harness's line; the ids over the capacity are appended when there are any"""
    return ('Relinked (gate %g mm, gap up to %d): %d births, %d links, %d -> %d tracks, link gap mean/max %.3f/%d frames'
            % (gate_mm, max_gap, r['births'], r['links'], r['tracks_before'], r['tracks_after'], r['mean_gap'], r['max_gap'])
            + (', %d rows over the id capacity' % r['over_ids'] if r['over_ids'] else ''))
