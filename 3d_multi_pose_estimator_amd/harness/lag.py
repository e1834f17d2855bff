"""numpy statement of what mpe_lag_batch and mpe_lag_estimate compute (csrc/lag.hip, csrc/lag_pick.h): how many frames
each camera runs ahead of or behind the poses of a recording, from the recording's own tracked poses -- and the script that
alternates this with the matching / triangulation / tracking stages and re-pairs the cameras' entries by the integer parts.
The GPU tests hold the kernel's sums to `lag_pass_host` bit for bit and the estimate to `lag_estimate_host` bit for bit.
include/mpe.h words the rule; the lines below are its lines.

All arithmetic is float64, every operation rounded on its own (numpy fuses nothing; the pick runs on Python floats, which
are IEEE doubles), in the header's order.  The observations of a camera are the entries harness/reprojection.py counts.

As a script:

    python -m 3d_multi_pose_estimator_amd.harness.lag --testfiles F.json --tmdir DIR --matcher geometric \
        --window 4 --sub 4 --rounds 3 [--lag-huber PX] [--hold NAME] [--refine ITERS] [--track-gate M --track-gap N] [--correct N --correct-inner M] [--out lags.json]

A round matches, triangulates, (with --refine) refines and tracks every batch, makes the table from the kept poses and ids on
the device, takes one pass over the kept batches and estimates.  Per camera it prints the observations supported, the mean
cost at zero lag and at the best entry as RMS pixels, the grid and the refined lag relative to the held camera (the first by
default: the common shift of all cameras is not observable from poses the cameras made themselves) and the total integer
shift applied so far.  The integer parts, rounded relative to the held camera, are then applied with `retime_frames` and the
recording is packed again; the script stops early when a round applies nothing.  The fractional remainder is relative to
the poses' own time and biased towards zero.  --correct N [--correct-inner M] corrects it in the poses: N times, the lags
relative to the held camera go to M rounds of the time-aware refinement over all batches (harness/refine_timed.py,
Engine.refine_timed; the first round reads the round's uncorrected tracked poses, each later one the output of the one
before), one more pass of the estimator runs against the corrected table, and per camera the lag and the RMS pixels at the
best entry before and after are printed, with the joints timed.  --out then also holds 'lags': the whole lag of every
camera (integer shift plus remainder), what --lags of the metrics scripts takes.
--synthetic N --lags 0,2,-1,0,1 runs on generated frames (bodies on seeded smooth walks, every camera's column projected
from the bodies at its own time) and also prints the true lags.
"""
import json
import math

import numpy as np

from . import reprojection as R
from .refine import camera_constants64, project64, _rho

FEW_OBS, EDGE, FLAT = 1, 2, 4
MAX_WINDOW, MAX_SUB = 8, 8


def grid(window, sub):
    """-> [(k, s, r, alpha)] for i = 0 .. K-1: k = i - W*sub, s = floor(k / sub), r = k - s*sub, alpha = r / sub."""
    W, sub = int(window), int(sub)
    if not 0 <= W <= MAX_WINDOW or not 1 <= sub <= MAX_SUB:
        raise ValueError('window within 0 .. %d, sub within 1 .. %d' % (MAX_WINDOW, MAX_SUB))
    out = []
    for i in range(2 * W * sub + 1):
        k = i - W * sub
        s = k // sub                                  # Python's // rounds towards -inf
        r = k - s * sub
        out.append((k, s, r, float(r) / float(sub)))
    return out


def new_sums(V, K):
    return {'cost': np.zeros((V, K)), 'n_obs': np.zeros((V, K), np.int64), 'n_skipped': np.zeros((V, K), np.int64),
            'n_support': np.zeros(V, np.int64), 'n_unsupported': np.zeros(V, np.int64)}


def track_rows(frame_start, n_frames, table_flags, table_n_persons, table_ids, window):
    """-> rows [F,Pcap,2W+1] int: the row of the track of row p of frame f in table frame f - W + w, -1 without one (the
    header's row of a track: the lowest row with that id and, with per-row flags, the flag set)."""
    ids = np.asarray(table_ids)
    n_table, Pcap = ids.shape
    flags = np.asarray(table_flags) != 0
    n_rows = np.clip(np.asarray(table_n_persons).astype(np.int64), 0, Pcap)
    W = int(window)
    rows = np.full((n_frames, Pcap, 2 * W + 1), -1, np.int64)
    for fl in range(n_frames):
        f = frame_start + fl
        for p in range(int(n_rows[f])):
            t = int(ids[f, p])
            if t < 0:
                continue
            for w in range(2 * W + 1):
                g = f - W + w
                if not 0 <= g < n_table:
                    continue
                hit = ids[g, :n_rows[g]] == t
                if flags.ndim == 2:
                    hit = hit & flags[g, :n_rows[g]]
                where = np.nonzero(hit)[0]
                if len(where):
                    rows[fl, p, w] = int(where[0])
    return rows


def lag_terms(calib, pb, frame_start, persons, table_poses, table_flags, table_n_persons, table_ids, window, sub, huber_px=0.0,
              joint_mask=None, threshold=0.5):
    """-> (sel [F,Pcap,V,J] bool: the observations; supported [F,Pcap,J] bool; summed [F,Pcap,V,J,K] bool: the supported
    observations whose term is summed at entry k (the others are skipped there); terms [F,Pcap,V,J,K] float64: rho(e),
    unspecified where summed is False)."""
    if not huber_px >= 0.0:
        raise ValueError('huber_px >= 0')
    huber = float(huber_px)
    persons = np.asarray(persons)
    F, Pcap, V = persons.shape
    poses = np.asarray(table_poses)
    if poses.dtype not in (np.float32, np.float64):
        raise ValueError('poses must be float32 or float64')
    flags = np.asarray(table_flags)
    n_table, J = poses.shape[0], poses.shape[2]
    if frame_start < 0 or frame_start + F > n_table:
        raise ValueError('the frames of the call lie outside the table')
    G = grid(window, sub)
    W, K = int(window), len(G)
    joint_mask = (1 << J) - 1 if joint_mask is None else int(joint_mask)
    sl = slice(frame_start, frame_start + F)
    sel, xy = R.selection(pb, persons, np.asarray(table_n_persons)[sl], flags[sl], joint_mask, threshold)
    rows = track_rows(frame_start, F, flags, table_n_persons, table_ids, W)
    X = poses.astype(np.float64)
    finite = np.isfinite(X).all(axis=-1)                                          # [n_table,Pcap,J]
    flagged = (flags != 0) if flags.ndim == 3 else np.repeat((flags != 0)[..., None], J, axis=2)
    fl = np.arange(F)[:, None]
    supported = np.ones((F, Pcap, J), bool)
    for w in range(2 * W + 1):
        g = np.clip(frame_start + fl - W + w, 0, n_table - 1)                     # [F,1]
        row = rows[:, :, w]
        at = np.maximum(row, 0)
        supported &= (row >= 0)[..., None] & flagged[g, at] & finite[g, at]
    _, kd, Kc = camera_constants64(calib)
    T = R.engine_calibration(calib)[0]
    summed = np.zeros((F, Pcap, V, J, K), bool)
    terms = np.zeros((F, Pcap, V, J, K))
    with np.errstate(all='ignore'):
        for i, (k, s, r, alpha) in enumerate(G):
            ga = np.clip(frame_start + fl + s, 0, n_table - 1)
            Xk = X[ga, np.maximum(rows[:, :, s + W], 0)]                          # [F,Pcap,J,3]
            if r:
                gb = np.clip(frame_start + fl + s + 1, 0, n_table - 1)
                Xb = X[gb, np.maximum(rows[:, :, s + W + 1], 0)]
                Xk = Xk + alpha * (Xb - Xk)
            for c in range(V):
                p = project64(T[c], kd[c], Kc[c], Xk[..., 0], Xk[..., 1], Xk[..., 2])
                good = (p['pc2'] > 0.0) & np.isfinite(p['px']) & np.isfinite(p['py'])
                rx = p['px'] - xy[:, :, c, :, 0]
                ry = p['py'] - xy[:, :, c, :, 1]
                e = np.sqrt(rx * rx + ry * ry)
                summed[:, :, c, :, i] = sel[:, :, c] & supported & good
                terms[:, :, c, :, i] = _rho(e, huber)
    return sel, supported, summed, terms


def lag_pass_host(calib, pb, frame_start, persons, table_poses, table_flags, table_n_persons, table_ids, window, sub, huber_px=0.0,
                  sums=None, joint_mask=None, threshold=0.5):
    """One mpe_lag_batch call on the host: pb holds the detections of the table frames frame_start .. frame_start + F - 1,
    persons [F,Pcap,V] their rows; the table is poses [n_table,Pcap,J,3] float32 or float64, flags [n_table,Pcap] (per row)
    or [n_table,Pcap,J] (per joint), n_persons [n_table], ids [n_table,Pcap].  sums: what earlier calls of the pass left
    (new_sums(V, K) at the start of a pass); it is updated and returned: {'cost' [V,K], 'n_obs' [V,K], 'n_skipped' [V,K],
    'n_support' [V], 'n_unsupported' [V]}."""
    persons = np.asarray(persons)
    F, Pcap, V = persons.shape
    K = 2 * int(window) * int(sub) + 1
    sums = new_sums(V, K) if sums is None else sums
    if F == 0:
        return sums
    sel, supported, summed, terms = lag_terms(calib, pb, frame_start, persons, table_poses, table_flags, table_n_persons, table_ids,
                                              window, sub, huber_px, joint_mask, threshold)
    J = sel.shape[-1]
    S = np.zeros((F, V, K))                                                       # the frame partials: left folds over p, then j
    for p in range(Pcap):
        for j in range(J):
            S = np.where(summed[:, p, :, j, :], S + terms[:, p, :, j, :], S)
    cost = sums['cost']
    for f in range(F):                                                            # every frame, in order
        cost = cost + S[f]
    sums['cost'] = cost
    sup = sel & supported[:, :, None, :]
    sums['n_obs'] = sums['n_obs'] + summed.sum(axis=(0, 1, 3))
    sums['n_skipped'] = sums['n_skipped'] + (sup[..., None] & ~summed).sum(axis=(0, 1, 3))
    sums['n_support'] = sums['n_support'] + sup.sum(axis=(0, 1, 3))
    sums['n_unsupported'] = sums['n_unsupported'] + (sel & ~sup).sum(axis=(0, 1, 3))
    return sums


# ---- the pick: csrc/lag_pick.h, statement for statement, on Python floats ----------------------------------------------

def lag_pick(cost, n_obs, window, sub, min_obs):
    """One camera's K sums and counts -> {'status', 'k_best', 'lag_grid', 'lag_refined', 'cost_best', 'cost_zero', 'n_obs'}."""
    W, sub, min_obs = int(window), int(sub), int(min_obs)
    K, zero = 2 * W * sub + 1, W * sub
    cost, n_obs = [float(x) for x in cost], [int(x) for x in n_obs]

    def mean(i):
        with np.errstate(all='ignore'):
            return float(np.float64(cost[i]) / np.float64(float(n_obs[i])))
    out = {'status': 0, 'k_best': 0, 'lag_grid': 0.0, 'lag_refined': 0.0, 'cost_best': math.nan, 'cost_zero': math.nan, 'n_obs': 0}
    best, m_best = -1, math.nan
    for i in range(K):
        if n_obs[i] < min_obs:
            continue
        m = mean(i)
        if best < 0 or m < m_best or (m_best != m_best and m == m):
            best, m_best = i, m
    if best < 0:
        out['status'] = FEW_OBS
        return out
    k = best - zero
    out.update(k_best=k, cost_best=m_best, n_obs=n_obs[best], lag_grid=float(k) / float(sub), lag_refined=float(k) / float(sub))
    if n_obs[zero] >= min_obs:
        out['cost_zero'] = mean(zero)
    if best == 0 or best == K - 1 or n_obs[best - 1] < min_obs or n_obs[best + 1] < min_obs:
        out['status'] = EDGE
        return out
    lo, hi = mean(best - 1), mean(best + 1)
    den = (lo - m_best) + (hi - m_best)
    off = 0.0
    if den > 0.0:
        off = float(np.float64(0.5 * (lo - hi)) / np.float64(den))
        off = 0.5 if off > 0.5 else off
        off = -0.5 if off < -0.5 else off
        if off != off:
            off, out['status'] = 0.0, FLAT
    else:
        out['status'] = FLAT
    out['lag_refined'] = (float(k) + off) / float(sub)
    return out


def lag_estimate_host(sums, window, sub, min_obs=50):
    """mpe_lag_estimate on the host: `sums` what a pass left (lag_pass_host, LagEstimator.read) -> {'status', 'k_best'
    int32, 'lag_grid', 'lag_refined', 'cost_best', 'cost_zero' float64, 'n_obs', 'n_support', 'n_unsupported' int64} as arrays
    over the cameras."""
    if int(min_obs) < 1:
        raise ValueError('min_obs >= 1')
    V = len(sums['cost'])
    picks = [lag_pick(sums['cost'][c], sums['n_obs'][c], window, sub, min_obs) for c in range(V)]
    out = {k: np.array([p[k] for p in picks], np.int32) for k in ('status', 'k_best')}
    out.update({k: np.array([p[k] for p in picks], np.float64) for k in ('lag_grid', 'lag_refined', 'cost_best', 'cost_zero')})
    out['n_obs'] = np.array([p['n_obs'] for p in picks], np.int64)
    out['n_support'] = np.asarray(sums['n_support']).astype(np.int64)
    out['n_unsupported'] = np.asarray(sums['n_unsupported']).astype(np.int64)
    return out


# ---- bookkeeping of the script ----------------------------------------------------------------------------------------

def retime_frames(frames, names, shift):
    """Frame f of the result takes camera names[c]'s entry of frame f - shift[c] (shift: integers over `names`, or {name:
    integer}); where that falls outside the recording the camera has no entry.  Cameras that are not named keep their
    entries.  The frames themselves are not modified."""
    if not isinstance(shift, dict):
        shift = dict(zip(names, shift))
    n = len(frames)
    cams = []
    for fr in frames:
        cams += [c for c in fr if c not in cams]         # every camera of the recording, in the order first seen
    out = []
    for f in range(n):
        frame = {}
        for cam in cams:
            src = f - int(shift.get(cam, 0))
            if 0 <= src < n and cam in frames[src]:
                frame[cam] = frames[src][cam]
        out.append(frame)
    return out


def relative_shifts(lags, hold):
    """The integer part of every camera's lag relative to camera `hold`, rounded half away from zero -> list of ints."""
    rel = [float(x) - float(lags[hold]) for x in lags]
    return [int(math.floor(abs(x) + 0.5)) * (1 if x >= 0 else -1) for x in rel]


def correct_rounds(eng, calib, args, names, h, kept, packed, table, rep, estimate):
    """--correct: N alternations of (the lags relative to the held camera; M rounds of the time-aware refinement over all
    batches, the first reading the round's uncorrected tracked poses and each later one the output of the one before -- the
    frames whose neighbours are missing stay as they were, and what they spoil reaches M * ceil(max |lag|) frames at most;
    one pass of the estimator against the corrected table).  -> one dict per alternation; 'report' is its estimate."""
    import torch

    from .refine_timed import refine_timed
    out = []
    iters = args.refine if args.refine else 10
    for n in range(args.correct):
        lags = [float(rep['lag_refined'][c] - rep['lag_refined'][h]) for c in range(len(names))]
        lags = [max(-float(MAX_WINDOW), min(float(MAX_WINDOW), x)) for x in lags]
        corrected, timed = table, 0
        for m in range(max(1, args.correct_inner)):
            if args.host_statement:
                host = [t.cpu().numpy() for t in corrected]
                res = [refine_timed(calib, pb, at, persons.cpu().numpy(), *host, lags, (1 << eng.J) - 1, max_iters=iters, huber_px=args.refine_huber)
                       for (db, at, persons, _, _, _, _), pb in zip(kept, packed)]
                poses = torch.from_numpy(np.concatenate([r['poses'] for r in res])).to(table[0].device)
                timed = int(sum(int((r['n_timed'] > 0).sum()) for r in res))
            else:
                res = [eng.refine_timed(db, at, persons, *corrected, 'triang', lags, max_iters=iters, huber_px=args.refine_huber)
                       for db, at, persons, _, _, _, _ in kept]
                poses = torch.cat([r['poses'] for r in res])
                timed = int(sum(int((r['n_timed'] > 0).sum()) for r in res))
            corrected = [poses.contiguous()] + list(table[1:])
        after = estimate(kept, packed, corrected)
        with np.errstate(all='ignore'):
            rms_b, rms_a = np.sqrt(rep['cost_best']), np.sqrt(after['cost_best'])
        rel_a = [float(after['lag_refined'][c] - after['lag_refined'][h]) for c in range(len(names))]
        for c, name in enumerate(names):
            print('correction %d camera %s: lag %+.4f frames before, %+.4f after; RMS %.4f px at the best entry before, %.4f after%s'
                  % (n + 1, name, lags[c], rel_a[c], rms_b[c], rms_a[c], ' (status %d)' % after['status'][c] if after['status'][c] else ''))
        print('correction %d: %d joints timed in the last of %d rounds' % (n + 1, timed, max(1, args.correct_inner)))
        out.append({'lag_before': lags, 'lag_after': rel_a, 'rms_before': rms_b.tolist(), 'rms_after': rms_a.tolist(), 'joints_timed': timed,
                    'report': after})
        rep = after
    return out


def build_own_parser():
    from .common import build_parser
    p = build_parser('Estimate per-camera time lags from the poses of a recording and re-pair the cameras by their integer parts')
    p.add_argument('--window', type=int, default=4, help='the grid reaches this many frames either way (0 .. %d)' % MAX_WINDOW)
    p.add_argument('--sub', type=int, default=4, help='grid entries per frame (1 .. %d)' % MAX_SUB)
    p.add_argument('--rounds', type=int, default=3, help='match / triangulate / track / estimate alternations, at most')
    p.add_argument('--lag-huber', type=float, default=0.0, metavar='PX', help='Huber threshold of the cost in pixels (0: the plain square)')
    p.add_argument('--hold', type=str, default=None, metavar='NAME', help='the camera the lags are relative to (default: the first)')
    p.add_argument('--min-obs', type=int, default=50, help='a grid entry with fewer observations is not valid')
    p.add_argument('--out', type=str, default=None, metavar='lags.json', help='write the report')
    p.add_argument('--lags', type=str, default=None, metavar='L,L,..', help='--synthetic: the true lag of every camera, frames')
    p.add_argument('--lag-seed', type=int, default=1234, help='--synthetic: the seed of the walks')
    p.add_argument('--weave', type=float, default=0.0, metavar='M', help='--synthetic: the bodies weave sideways by this much, metres')
    p.add_argument('--host-statement', action='store_true', help='take the passes through the numpy statement instead of the device')
    p.add_argument('--correct', type=int, default=0, metavar='N', help='after the integer rounds: N alternations of the time-aware refinement '
                   '(the sub-frame lags corrected in the poses) with the estimate (0: the lags are reported only)')
    p.add_argument('--correct-inner', type=int, default=2, metavar='M', help='--correct: rounds of the time-aware refinement per alternation, '
                   'each reading its offsets from the poses of the one before')
    return p


def run(args):
    import torch

    from ..parameters import parameters
    from ..pipeline import Engine
    from .. import synthetic
    from .calibrate import rig_calibration
    from .common import held_cameras, load_frames, match_stage, max_skeletons_per_camera
    calib = rig_calibration(args)
    names = list(parameters.used_cameras_skeleton_matching)
    true_lags = None
    if args.synthetic:
        true_lags = [float(x) for x in args.lags.split(',')] if args.lags else [0.0] * len(names)
        if len(true_lags) != len(names):
            raise SystemExit('--lags: %d values for %d cameras' % (len(true_lags), len(names)))
        frames = synthetic.lagged_recording(calib, args.synthetic, true_lags, n_bodies=args.persons, seed=args.lag_seed, weave=args.weave)[0]
    else:
        frames = load_frames(args)
    hold = held_cameras(None if args.hold is None else [args.hold], names)[0]
    h = names.index(hold)
    ppc = max(4, args.persons + 1, max_skeletons_per_camera([(f, None, None) for f in frames]))
    eng = Engine(parameters, calib, max_frames=args.batch, max_persons_per_camera=ppc)
    est = eng.lag_estimator('triang', window=args.window, sub=args.sub, huber_px=args.lag_huber)
    tracker = eng.tracker('tri', max_gap=args.track_gap, gate=args.track_gate)
    total = [0] * len(names)
    report = {'cameras': names, 'hold': hold, 'window': args.window, 'sub': args.sub, 'rounds': []}
    if true_lags is not None:
        report['true_lags'] = true_lags
        print('true lags (frames): ' + ', '.join('%s %+g' % (n, x) for n, x in zip(names, true_lags)))
    current = frames

    def stage(current):
        """match, triangulate, (refine,) track every batch -> the kept batches, the packed ones and the table."""
        kept, packed = [], []
        tracker.reset()
        for at in range(0, len(current), args.batch):
            chunk = [{c: [f[c][0], f[c][1]] for c in f if json.loads(f[c][0])} for f in current[at:at + args.batch]]
            pb = eng.pack(chunk)
            db = eng.to_device(pb)
            persons, n_persons = match_stage(eng, args, db)
            poses, flags = eng.triangulate(db, persons, n_persons, all_joints=True)
            if args.refine:
                eng.refine(db, persons, n_persons, poses, flags, 'triang', max_iters=args.refine, huber_px=args.refine_huber, out=poses)
            ids = tracker.update(poses, flags, n_persons)['ids']
            kept.append((db, at, persons, n_persons, poses, flags, ids))
            packed.append(pb)
        eng.sync_status()
        table = [torch.cat([b[i] for b in kept]).contiguous() for i in (4, 5, 3, 6)]          # poses, flags, n_persons, ids
        return kept, packed, table

    def estimate(kept, packed, table):
        """one pass over the kept batches against `table` and the estimate"""
        if args.host_statement:
            sums = None
            host = [t.cpu().numpy() for t in table]
            for (db, at, persons, _, _, _, _), pb in zip(kept, packed):
                sums = lag_pass_host(calib, pb, at, persons.cpu().numpy(), *host, args.window, args.sub, args.lag_huber, sums=sums)
            return lag_estimate_host(sums, args.window, args.sub, args.min_obs)
        est.reset()
        for db, at, persons, _, _, _, _ in kept:
            est.accumulate(db, at, persons, *table)
        return est.estimate(args.min_obs)

    settled = False
    for rnd in range(max(1, args.rounds)):
        kept, packed, table = stage(current)
        rep = estimate(kept, packed, table)
        shifts = relative_shifts(rep['lag_refined'], h)
        total = [a + b for a, b in zip(total, shifts)]
        with np.errstate(all='ignore'):
            rms0, rms1 = np.sqrt(rep['cost_zero']), np.sqrt(rep['cost_best'])
        for c, name in enumerate(names):
            print('round %d camera %s: %d observations supported, RMS %.4f px at zero lag, %.4f px at the best entry, lag %+.4f frames '
                  '(grid %+.4f) relative to %s, shifted %+d frames so far%s'
                  % (rnd + 1, name, int(rep['n_support'][c]), rms0[c], rms1[c], float(rep['lag_refined'][c] - rep['lag_refined'][h]),
                     float(rep['lag_grid'][c] - rep['lag_grid'][h]), hold, total[c], ' (status %d)' % rep['status'][c] if rep['status'][c] else ''))
        report['rounds'].append({'lag_grid': rep['lag_grid'].tolist(), 'lag_refined': rep['lag_refined'].tolist(), 'status': rep['status'].tolist(),
                                 'n_support': rep['n_support'].tolist(), 'rms_zero': rms0.tolist(), 'rms_best': rms1.tolist(),
                                 'applied': shifts, 'total_shift': list(total)})
        if not any(shifts):
            settled = True
            break
        current = retime_frames(frames, names, total)
    if args.correct > 0:
        if not settled:                                      # the last round shifted the cameras: the poses of the recording as it now stands
            kept, packed, table = stage(current)
            rep = estimate(kept, packed, table)
        report['correct'] = correct_rounds(eng, calib, args, names, h, kept, packed, table, rep, estimate)
        rep = report['correct'][-1]['report']
        for r in report['correct']:
            del r['report']
    est.close()
    tracker.close()
    eng.close()
    report['total_shift'] = list(total)
    if args.correct > 0:                                     # what --lags of the metrics scripts takes: the whole lag of every camera, frames
        report['lags'] = {n: float(total[c] + (rep['lag_refined'][c] - rep['lag_refined'][h])) for c, n in enumerate(names)}
    print('integer shifts relative to %s: ' % hold + ', '.join('%s %+d' % (n, s) for n, s in zip(names, total)))
    if args.out:
        with open(args.out, 'w') as fh:
            json.dump(report, fh, indent=1)
        print('wrote', args.out)
    return report


def main(argv=None):
    return run(build_own_parser().parse_args(argv))


if __name__ == '__main__':
    main()
