"""Milliseconds per call of the tracker (Engine.tracker / mpe_track_batch) on batches of poses that are already on the
device, and the kernels it enqueues per call.

    python tools/track_rate.py [--frames 1000] [--persons 4 10] [--gaps 0 2] [--reps 50] [--out FILE]

Per shape 5 x persons (pcap = 5 * persons / 2): `persons` people on random walks of 2 cm per frame with 15 % dropouts
and the rows permuted per frame, as f32 poses with person flags (the MLP route) and as f64 poses with joint flags (the
triangulation route, 10 % of the joints missing).  The time is that of `--reps` calls enqueued back to back between two
synchronisations; set it beside the step time `python bench.py` reports on the same board.  For kernel times run it
under `rocprofv3 --kernel-trace --stats -- python tools/track_rate.py ...` (k_track_*)."""
import argparse
import importlib
import json
import os
import sys
import time

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
PKG = '3d_multi_pose_estimator_amd'


def walk(rng, B, P, pcap, J, tri):
    dt = np.float64 if tri else np.float32
    pos = rng.uniform(-3, 3, (P, 3))
    shape = rng.normal(0, 0.25, (P, J, 3))
    poses = np.zeros((B, pcap, J, 3), dt)
    flags = np.zeros((B, pcap, J) if tri else (B, pcap), np.uint8)
    n_persons = np.zeros(B, np.int32)
    for f in range(B):
        step = rng.normal(size=(P, 3))
        pos = pos + 0.02 * step / np.linalg.norm(step, axis=1, keepdims=True)
        seen = rng.permutation(np.flatnonzero(rng.random(P) >= 0.15))
        n_persons[f] = len(seen)
        poses[f, :len(seen)] = (pos[seen][:, None] + shape[seen]).astype(dt)
        flags[f, :len(seen)] = (rng.random((len(seen), J)) >= 0.1) if tri else 1
    return poses, flags, n_persons


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--frames', type=int, default=1000)
    ap.add_argument('--persons', type=int, nargs='+', default=[4, 10])
    ap.add_argument('--gaps', type=int, nargs='+', default=[0, 2])
    ap.add_argument('--reps', type=int, default=50)
    ap.add_argument('--out', type=str, default=None)
    args = ap.parse_args()
    Engine = importlib.import_module(PKG + '.pipeline').Engine
    params = importlib.import_module(PKG + '.parameters').parameters
    rng = np.random.default_rng(0)
    lines = []
    for P in args.persons:
        eng = Engine(params, max_frames=8, max_persons_per_camera=P)
        for tri in (False, True):
            poses, flags, n_persons = (torch.from_numpy(a).cuda() for a in walk(rng, args.frames, P, eng.pcap, eng.J, tri))
            for gap in args.gaps:
                tr = eng.tracker('tri' if tri else 'mlp', max_gap=gap, gate=0.5)
                out = tr.update(poses, flags, n_persons)                       # warm-up
                torch.cuda.synchronize()
                issued = int(out['issued'][0])
                n0 = tr.launches()
                t0 = time.time()
                for _ in range(args.reps):
                    tr.update(poses, flags, n_persons)
                torch.cuda.synchronize()
                ms = (time.time() - t0) * 1e3 / args.reps
                lines.append(json.dumps({'shape': '5x%d' % P, 'pcap': eng.pcap, 'poses': 'f64' if tri else 'f32', 'frames': args.frames,
                                         'max_gap': gap, 'ms_per_call': round(ms, 4), 'launches_per_call': (tr.launches() - n0) // args.reps,
                                         'tracks_first_call': issued}))
                print(lines[-1], flush=True)
                tr.close()
        eng.close()
    if args.out:
        with open(args.out, 'w') as fh:
            fh.write('\n'.join(lines) + '\n')


if __name__ == '__main__':
    main()
