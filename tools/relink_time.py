"""Milliseconds per call of the relinker (Engine.relinker: Relinker.update, mpe_relink_batch) and, as the yardstick, of
Tracker.update (mpe_track_batch) on the same rows, which are already on the device.

    python tools/relink_time.py [--frames 1000] [--persons 4] [--reps 30] [--calls 20] [--out FILE]

The benchmark shape: 5 views x `persons` people (pcap = 5 * persons / 2), bodies of skel-like proportions whose scales are
8 % apart, on random walks of 2 cm per frame with 2 mm of noise per coordinate, the rows permuted per frame; every body is
away once for 30 frames and returns 1.5 m from where it left (one return per body), as f32 poses with person flags and as
f64 poses with joint flags (10 % of the joints missing).  Both objects carry a sequence, so a timed call is reset() +
update() of the whole batch: the same frames, births and links every time.  One repeat is `--calls` such calls enqueued
back to back between two events on the current stream; relinker and tracker are measured in alternation after a warm-up
and the median of the `--reps` repeats is reported with the spread (min, max).  A batch without any birth after the
first frame (the same bodies, nobody away) is timed beside it: what the walk costs when no frame has a candidate."""
import argparse
import importlib
import json
import os
import sys

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, 'tools'))
PKG = '3d_multi_pose_estimator_amd'

# a standing adult, metres, y up: nose, eyes, ears, shoulders, elbows, wrists, hips, knees, ankles, neck
BODY = np.array([[0.00, 1.62, 0.09], [0.03, 1.66, 0.07], [-0.03, 1.66, 0.07], [0.07, 1.64, 0.00], [-0.07, 1.64, 0.00],
                 [0.19, 1.45, 0.00], [-0.19, 1.45, 0.00], [0.24, 1.17, 0.02], [-0.24, 1.17, 0.02], [0.26, 0.92, 0.08],
                 [-0.26, 0.92, 0.08], [0.10, 0.95, 0.00], [-0.10, 0.95, 0.00], [0.11, 0.52, 0.03], [-0.11, 0.52, 0.03],
                 [0.11, 0.09, 0.00], [-0.11, 0.09, 0.00], [0.00, 1.47, 0.00]])


def walk(rng, B, P, pcap, tri, away):
    dt = np.float64 if tri else np.float32
    J = len(BODY)
    pos = np.stack([3.0 * np.arange(P), np.zeros(P), 3.0 * (np.arange(P) % 2)], axis=1)
    scales = 0.8 + 0.08 * np.arange(P)
    poses = np.zeros((B, pcap, J, 3), dt)
    flags = np.zeros((B, pcap, J) if tri else (B, pcap), np.uint8)
    n_persons = np.zeros(B, np.int32)
    for f in range(B):
        step = rng.normal(size=(P, 3)) * np.array([1.0, 0.0, 1.0])
        pos = pos + 0.02 * step / np.linalg.norm(step, axis=1, keepdims=True)
        for k in range(P):
            if away and f == away[k][1] + 1:
                pos[k, 0] += 1.5
        seen = rng.permutation([k for k in range(P) if not (away and away[k][0] <= f <= away[k][1])])
        n_persons[f] = len(seen)
        for p, k in enumerate(seen):
            poses[f, p] = (BODY * scales[k] + pos[k] + rng.normal(0.0, 0.002, (J, 3))).astype(dt)
            flags[f, p] = (rng.random(J) >= 0.1) if tri else 1
    return poses, flags, n_persons


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--frames', type=int, default=1000)
    ap.add_argument('--persons', type=int, default=4)
    ap.add_argument('--reps', type=int, default=30)
    ap.add_argument('--calls', type=int, default=20)
    ap.add_argument('--out', type=str, default=None)
    args = ap.parse_args()
    if not torch.cuda.is_available():
        sys.exit('relink_time.py measures on the GPU and there is none')
    timed = importlib.import_module('smooth_time').timed
    Engine = importlib.import_module(PKG + '.pipeline').Engine
    params = importlib.import_module(PKG + '.parameters').parameters
    eng = Engine(params, max_frames=args.frames, max_persons_per_camera=args.persons)
    assert eng.J == len(BODY)
    span = args.frames // (args.persons + 1)
    away = [(span * (k + 1), span * (k + 1) + 29) for k in range(args.persons)]
    lines = []
    for tri in (False, True):
        mode = 'tri' if tri else 'mlp'
        for name, gone in (('one return per body', away), ('nobody away', None)):
            rng = np.random.default_rng(0)
            poses, flags, n_persons = (torch.from_numpy(a).cuda() for a in walk(rng, args.frames, args.persons, eng.pcap, tri, gone))
            tr, rl = eng.tracker(mode, max_gap=2, gate=0.5), eng.relinker(mode, min_gap=4)
            ids = tr.update(poses, flags, n_persons)['ids']

            def relink():
                rl.reset()
                return rl.update(poses, flags, n_persons, ids)

            def track():
                tr.reset()
                return tr.update(poses, flags, n_persons)
            fns = {'relink': relink, 'track': track}
            for fn in fns.values():                          # warm-up: code objects, the allocator's blocks
                timed(fn, args.calls)
            per_call = {}
            for k, obj in (('relink', rl), ('track', tr)):
                n0 = obj.launches()
                fns[k]()
                per_call[k] = obj.launches() - n0
            ms = {k: [] for k in fns}
            for _ in range(args.reps):
                for k, fn in fns.items():
                    ms[k].append(timed(fn, args.calls))
            out = relink()
            torch.cuda.synchronize()
            ctr = rl.counters()
            gaps = out['link_gap'][out['link_gap'] > 0]
            rec = {'shape': '5x%d' % args.persons, 'pcap': eng.pcap, 'poses': 'f64' if tri else 'f32', 'frames': args.frames, 'input': name,
                   'reps': args.reps, 'calls_per_rep': args.calls, 'launches_per_call': per_call, 'tracker_ids': int(ids.max()) + 1,
                   'births': ctr['births'], 'linked': ctr['linked'], 'over_ids': ctr['over_ids'],
                   'link_gaps': sorted(int(g) for g in gaps.cpu())}
            for k in fns:
                rec[k + '_ms_median_min_max'] = [round(float(np.median(ms[k])), 4), round(min(ms[k]), 4), round(max(ms[k]), 4)]
            rec['relink_us_per_frame'] = round(1000.0 * float(np.median(ms['relink'])) / args.frames, 4)
            rec['ratio_to_track'] = round(float(np.median(ms['relink'])) / float(np.median(ms['track'])), 3)
            lines.append(json.dumps(rec))
            print(lines[-1], flush=True)
            tr.close()
            rl.close()
    eng.close()
    if args.out:
        with open(args.out, 'w') as fh:
            fh.write('\n'.join(lines) + '\n')


if __name__ == '__main__':
    main()
