"""numpy statement of what mpe_track_score_batch / mpe_track_score_result compute (csrc/track_score.hip, csrc/assign_int.h):
how well the track ids of mpe_track_batch follow the ground-truth identities over a recording.  The measures are the
published ones -- CLEAR-MOT (Bernardin & Stiefelhagen 2008: MOTA, MOTP, ID switches, fragmentations, mostly tracked /
partially tracked / mostly lost) and the identity measures of Ristani et al. 2016 (IDF1, IDP, IDR) -- written out so that
every output is an exact integer or one float64 left fold.  The reference has no tracking and no such metric.

The wire format carries no GT identity (frame[cam][3] is a bare list of bodies), so the harness gets the identities from
a second tracker run over the GT bodies themselves (Engine.tracker('gt')).

The rule -- the contract of the device path:

Frames arrive in sequence order, in any chunking.  A frame with skip[f] != 0 changes neither the state nor the frame
count; its frame_counts are 0 and its match_tid are -2.

Prediction side of frame f.  Detections and their order are mpe_eval_batch's: joint_flags == 0: detection r is the r-th
row p < n_persons[f] with flags[f, p] != 0; joint_flags == 1: r = p < n_persons[f].  Those with r < n_res[f] exist.
Detection r carries g = assign[f, r], e = err[f, r] (metres), invalid[f, r] (None: 0) and the track id
h = track_ids[f, p(r)] (row order, as the tracker writes it).

GT side.  Row g < n_gt[f] carries o = gt_ids[f, g] and gt_valid[f, g]; it is COUNTED when valid and o >= 0, every other
row is an IGNORE row.

Classes.  A detection with 0 <= g < n_gt[f] whose row is an ignore row is IGNORED and counts nowhere.  A detection is a
CANDIDATE when g names a counted row, e * 1000. < threshold_mm (float64, strict: the reference's own AP test,
test/metrics_from_model.py:357), it is not invalid and h >= 0; the candidate of lowest r of a row is its MATCH.  Every
other detection that is not ignored is a FALSE POSITIVE; a counted row without a match is a MISS.

Per frame.  frame_counts[f] = (tp, fp, fn, idsw); match_tid[f, g] = h of the match, -1 for a miss, -2 for a row that is not
counted.

Identity pass.  The RECORD of a counted row is (o, h) or (o, miss).  For every identity o, over the frames with a record
of o in order: present[o] += 1; with a match: matched[o] += 1, table[o, h] += 1, an ID switch when last[o] >= 0 and
last[o] != h, then last[o] = h, and a fragmentation when o was matched in an earlier frame and its previous record was a
miss; last[o] survives misses and absences.  pred_count[h] += 1 for every detection with h >= 0 that is not ignored.
Left out, each adding 1 to over_ids and setting the sticky OVER_IDS bit: a record with o >= gid_cap, with a matched
h >= tid_cap, or whose o a lower counted row of the frame already carries; a pred_count increment with h >= tid_cap.
tp / fp / fn count them all the same.

Totals: frames, n_gt (counted rows), n_pred (detections not ignored), tp, fp, fn, idsw, frag, ignored, over_ids;
err_sum is the float64 left fold of e over the matches in (frame, detection) order (what np.cumsum gives).

Result.  MOTA = 1 - (fn + fp + idsw) / n_gt; MOTP_mm = err_sum * 1000 / tp; IDTP = the largest sum of table over
one-to-one pairings of identities and tracks; IDP = IDTP / n_pred, IDR = IDTP / n_gt, IDF1 = 2 IDTP / (n_gt + n_pred);
an identity with present > 0 is mostly tracked when 5 * matched >= 4 * present, mostly lost when 5 * matched < present,
partially tracked otherwise.  A ratio with a zero denominator is NaN.
"""
import numpy as np

OVER_IDS = 1
INT_KEYS = ('frames', 'n_gt', 'n_pred', 'tp', 'fp', 'fn', 'idsw', 'frag', 'ignored', 'over_ids')
RESULT_INT_KEYS = INT_KEYS + ('idtp', 'n_ids', 'n_tracks', 'mt', 'pt', 'ml', 'status')
RESULT_FLOAT_KEYS = ('err_sum', 'mota', 'motp_mm', 'idp', 'idr', 'idf1')


def assign_int_max(table):
    """The largest sum a one-to-one pairing of rows and columns collects from a table of non-negative integers: the
    shortest-augmenting-path method of csrc/assign_int.h over the used rows and columns, in Python integers."""
    table = np.asarray(table)
    if table.size == 0:
        return 0
    rows, cols = np.flatnonzero((table != 0).any(1)), np.flatnonzero((table != 0).any(0))
    if not len(rows):
        return 0
    t = table[np.ix_(rows, cols)]
    if t.shape[0] > t.shape[1]:
        t = t.T
    val = [[int(x) for x in row] for row in t]
    n, m = len(val), len(val[0])
    INF = 1 << 62
    u, v, p, way = [0] * (n + 1), [0] * (m + 1), [0] * (m + 1), [0] * (m + 1)
    for i in range(1, n + 1):
        p[0], j0 = i, 0
        minv, used = [INF] * (m + 1), [False] * (m + 1)
        while True:
            used[j0] = True
            i0, delta, j1 = p[j0], INF, 0
            for j in range(1, m + 1):
                if used[j]:
                    continue
                cur = -val[i0 - 1][j - 1] - u[i0] - v[j]
                if cur < minv[j]:
                    minv[j], way[j] = cur, j0
                if minv[j] < delta:
                    delta, j1 = minv[j], j
            for j in range(m + 1):
                if used[j]:
                    u[p[j]] += delta
                    v[j] -= delta
                else:
                    minv[j] -= delta
            j0 = j1
            if p[j0] == 0:
                break
        while j0:
            j1 = way[j0]
            p[j0] = p[j1]
            j0 = j1
    return sum(val[p[j] - 1][j - 1] for j in range(1, m + 1) if p[j])


def ratios(r):
    """MOTA, MOTP, IDP, IDR, IDF1 from the integer totals, err_sum and idtp of `r` (in place)."""
    nan = float('nan')
    r['mota'] = 1.0 - float(r['fn'] + r['fp'] + r['idsw']) / float(r['n_gt']) if r['n_gt'] else nan
    r['motp_mm'] = r['err_sum'] * 1000. / float(r['tp']) if r['tp'] else nan
    r['idp'] = float(r['idtp']) / float(r['n_pred']) if r['n_pred'] else nan
    r['idr'] = float(r['idtp']) / float(r['n_gt']) if r['n_gt'] else nan
    r['idf1'] = 2.0 * float(r['idtp']) / float(r['n_gt'] + r['n_pred']) if r['n_gt'] + r['n_pred'] else nan
    return r


class TrackScoreRef:
    """The rule above, frame by frame.  update() takes the arrays mpe_track_score_batch takes, for the next frames of the
    recording; state() and result() are what mpe_track_score_read and mpe_track_score_result return."""

    def __init__(self, threshold_mm=150., gid_cap=256, tid_cap=4096):
        self.threshold_mm, self.gid_cap, self.tid_cap = float(threshold_mm), int(gid_cap), int(tid_cap)
        self.reset()

    def reset(self):
        G, T = self.gid_cap, self.tid_cap
        self.tot = dict.fromkeys(INT_KEYS, 0)
        self.err_sum = np.float64(0.0)
        self.status = 0
        self.last = np.full(G, -1, np.int32)
        self.present, self.matched, self.bits = np.zeros(G, np.int32), np.zeros(G, np.int32), np.zeros(G, np.int32)
        self.pred_count = np.zeros(T, np.int32)
        self.table = np.zeros((G, T), np.int32)

    def update(self, flags, n_persons, track_ids, assign, err, invalid, n_res, n_gt, gt_ids, gt_valid, joint_flags, skip=None):
        """-> {'frame_counts' [B,4] i32, 'match_tid' [B,gcap] i32, 'status' int}."""
        B, pcap = np.asarray(track_ids).shape
        gcap = np.asarray(gt_ids).shape[1]
        counts, mtid = np.zeros((B, 4), np.int32), np.full((B, gcap), -2, np.int32)
        tot = self.tot
        for f in range(B):
            if skip is not None and skip[f]:
                continue
            n_p, n_g = max(0, min(int(n_persons[f]), pcap)), max(0, min(int(n_gt[f]), gcap))
            rows = [p for p in range(n_p) if joint_flags or flags[f, p]]
            rows = rows[:max(0, min(int(n_res[f]), pcap))]
            counted = [bool(gt_valid[f, g]) and int(gt_ids[f, g]) >= 0 for g in range(n_g)]
            match = {}                                      # GT row -> (r, h, e) of its match
            ignored, named = [], []
            for r, p in enumerate(rows):
                g, e, h = int(assign[f, r]), np.float64(err[f, r]), int(track_ids[f, p])
                inv = invalid is not None and bool(invalid[f, r])
                ignored.append(0 <= g < n_g and not counted[g])
                named.append(h)
                if 0 <= g < n_g and counted[g] and e * 1000. < self.threshold_mm and not inv and h >= 0 and g not in match:
                    match[g] = (r, h, e)
            tp = len(match)
            fp = len(rows) - sum(ignored) - tp
            fn = sum(counted) - tp
            for r, h, e in sorted(match.values()):          # detection order
                self.err_sum = self.err_sum + e
            over = idsw = 0
            for r in range(len(rows)):
                if not ignored[r] and named[r] >= 0:
                    if named[r] < self.tid_cap:
                        self.pred_count[named[r]] += 1
                    else:
                        over += 1
            seen = set()
            for g in range(n_g):
                if not counted[g]:
                    continue
                o, h = int(gt_ids[f, g]), match[g][1] if g in match else -1
                mtid[f, g] = h
                if o >= self.gid_cap or h >= self.tid_cap or o in seen:
                    over += 1
                    continue
                seen.add(o)
                self.present[o] += 1
                if h >= 0:
                    self.matched[o] += 1
                    self.table[o, h] += 1
                    if self.last[o] >= 0 and self.last[o] != h:
                        idsw += 1
                    self.last[o] = h
                    if self.bits[o] == 3:
                        tot['frag'] += 1
                    self.bits[o] = 1
                else:
                    self.bits[o] |= 2
            counts[f] = (tp, fp, fn, idsw)
            for k, x in (('frames', 1), ('n_gt', sum(counted)), ('n_pred', tp + fp), ('tp', tp), ('fp', fp), ('fn', fn), ('idsw', idsw),
                         ('ignored', sum(ignored)), ('over_ids', over)):
                tot[k] += x
            if over:
                self.status |= OVER_IDS
        return {'frame_counts': counts, 'match_tid': mtid, 'status': self.status}

    def state(self):
        return {'last': self.last.copy(), 'present': self.present.copy(), 'matched': self.matched.copy(), 'bits': self.bits.copy(),
                'pred_count': self.pred_count.copy(), 'table': self.table.copy()}

    def result(self):
        r = dict(self.tot)
        r['err_sum'], r['status'] = float(self.err_sum), self.status
        r['idtp'] = assign_int_max(self.table)
        seen = self.present > 0
        m5, p1 = 5 * self.matched[seen].astype(np.int64), self.present[seen].astype(np.int64)
        r['n_ids'], r['n_tracks'] = int(seen.sum()), int((self.pred_count > 0).sum())
        r['mt'], r['ml'] = int((m5 >= 4 * p1).sum()), int((m5 < p1).sum())
        r['pt'] = r['n_ids'] - r['mt'] - r['ml']
        return ratios(r)


def report_line(r, threshold_mm):
    """The harness's report line for a result() dict."""
    return ('Track score (%g mm): MOTA %.4f, MOTP %.3f mm, IDF1 %.4f, IDP %.4f, IDR %.4f, %d ID switches, %d fragmentations, '
            'MT/PT/ML %d/%d/%d' % (threshold_mm, r['mota'], r['motp_mm'], r['idf1'], r['idp'], r['idr'], r['idsw'], r['frag'],
                                   r['mt'], r['pt'], r['ml']))
