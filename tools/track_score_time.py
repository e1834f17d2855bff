"""Milliseconds per call of the track scorer (Engine.track_scorer / mpe_track_score_batch) and, as the yardstick, of the
tracker (Engine.tracker / mpe_track_batch) on the same frames, with everything already on the device.

    python tools/track_score_time.py [--frames 1000] [--persons 4] [--reps 30] [--calls 20] [--out FILE]

The benchmark shape of tools/smooth_time.py: 5 views x `persons` people (pcap = 5 * persons / 2) on random walks of 2 cm
per frame with 15 % dropouts and the rows permuted per frame, as f32 poses with person flags (the MLP route) and as f64
poses with joint flags (the triangulation route).  The ground truth is the detections' own coordinates as f32 with the
rows reversed, so mpe_eval_batch has an assignment to find; its identities come from Tracker('gt').  One repeat is
`--calls` calls enqueued back to back between two events on the current stream; the two are measured in alternation
after a warm-up and the median of the `--reps` repeats is reported with the spread (min, max).  The scorer's totals keep
growing over the repeats; the work per call does not depend on them.  Set the numbers beside the step time
`python bench.py` reports on the same board."""
import argparse
import importlib
import json
import os
import sys
import types

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, 'tools'))
PKG = '3d_multi_pose_estimator_amd'


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--frames', type=int, default=1000)
    ap.add_argument('--persons', type=int, default=4)
    ap.add_argument('--reps', type=int, default=30)
    ap.add_argument('--calls', type=int, default=20)
    ap.add_argument('--out', type=str, default=None)
    args = ap.parse_args()
    if not torch.cuda.is_available():
        sys.exit('track_score_time.py measures on the GPU and there is none')
    walk = importlib.import_module('track_rate').walk
    timed = importlib.import_module('smooth_time').timed
    Engine = importlib.import_module(PKG + '.pipeline').Engine
    params = importlib.import_module(PKG + '.parameters').parameters
    rng = np.random.default_rng(0)
    eng = Engine(params, max_frames=8, max_persons_per_camera=args.persons)
    B, P, J = args.frames, eng.pcap, eng.J
    lines = []
    for tri in (False, True):
        mode = 'tri' if tri else 'mlp'
        poses, flags, n_persons = walk(rng, B, args.persons, P, J, tri)
        gt = {'xyz': np.zeros((B, P, J, 3), np.float32), 'joint': np.zeros((B, P, J), np.uint8), 'valid': np.zeros((B, P), np.uint8),
              'n': n_persons.copy()}
        for f in range(B):
            n = int(n_persons[f])
            gt['xyz'][f, :n] = poses[f, :n][::-1].astype(np.float32)
            gt['joint'][f, :n], gt['valid'][f, :n] = 1, 1
        poses, flags, n_persons = (torch.from_numpy(a).cuda() for a in (poses, flags, n_persons))
        tr, gtr = eng.tracker(mode, max_gap=2, gate=0.5), eng.tracker('gt', max_gap=2, gate=0.5, pcap=P)
        ts = eng.track_scorer(mode, max_frames=B, gcap=P)
        ids = tr.update(poses, flags, n_persons)['ids']
        ev = eng.evaluate(types.SimpleNamespace(n_frames=B), poses, flags, n_persons, gt, mode, skip=np.zeros(B, np.uint8))
        gt_ids = gtr.update(*(torch.from_numpy(gt[k]).cuda() for k in ('xyz', 'joint', 'n')))['ids']
        gt_valid = torch.from_numpy(gt['valid']).cuda()
        track = lambda: tr.update(poses, flags, n_persons)
        score = lambda: ts.update(ev, flags, n_persons, ids, gt_ids, gt_valid)
        for fn in (track, score):                        # warm-up: code objects, the allocator's blocks of both
            timed(fn, args.calls)
        ts.reset()
        score()
        first = ts.result()
        n0 = (tr.launches(), ts.launches())
        ms = {'track': [], 'score': []}
        for _ in range(args.reps):
            ms['track'].append(timed(track, args.calls))
            ms['score'].append(timed(score, args.calls))
        per_call = [(x.launches() - n) // (args.reps * args.calls) for x, n in zip((tr, ts), n0)]
        rec = {'shape': '5x%d' % args.persons, 'pcap': P, 'poses': 'f64' if tri else 'f32', 'frames': B, 'reps': args.reps,
               'calls_per_rep': args.calls, 'tp': first['tp'], 'fp': first['fp'], 'fn': first['fn'], 'idsw': first['idsw'],
               'mota': round(first['mota'], 4), 'idf1': round(first['idf1'], 4)}
        for k, n in zip(('track', 'score'), per_call):
            rec[k + '_ms_median'] = round(float(np.median(ms[k])), 4)
            rec[k + '_ms_min_max'] = [round(min(ms[k]), 4), round(max(ms[k]), 4)]
            rec[k + '_launches_per_call'] = n
        lines.append(json.dumps(rec))
        print(lines[-1], flush=True)
        for o in (tr, gtr, ts):
            o.close()
    eng.close()
    if args.out:
        with open(args.out, 'w') as fh:
            fh.write('\n'.join(lines) + '\n')


if __name__ == '__main__':
    main()
