"""Milliseconds per call of the time-aware refinement (Engine.refine_timed / mpe_refine_timed_batch: k_refine_timed) on a batch
and a table that are already on the device, beside the untimed refinement (Engine.refine / mpe_refine_batch: k_refine) on the
same batch in the same run.

    python tools/refine_timed_time.py [--frames 1000] [--persons 4 10] [--iters 10] [--reps 9] [--inner 20] [--out FILE]

Per shape 5 x persons: `--frames` frames of bodies on seeded walks (synthetic.walking_bodies, 1 mm per frame so that they
stay in view for the whole recording; every camera at lag 0), the table is the true bodies moved by up to 1 cm per coordinate
as f64 poses with joint flags, track id = body, persons from the generator's ownership.  Two settings of the lags given to
the call: every lag zero (no offset is read: the kernel's own overhead) and every lag nonzero with alpha != 0 (every
observing camera reads an offset made of three table rows).  Both kernels run `--iters` iterations with step_tol = 0, so every
solved joint runs all of them.  Method: warm calls first; then `--reps` windows of `--inner` calls enqueued back to back
between two device events on the stream the calls go to, timed and untimed windows alternating; the figure is the median
window divided by `--inner`, the spread (min .. max) is printed beside it.  For the kernels' own time run it under
`rocprofv3 --kernel-trace --stats -- python tools/refine_timed_time.py ...`."""
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
SETTINGS = (('all zero', (0.0, 0.0, 0.0, 0.0, 0.0)), ('all nonzero', (0.5, -0.25, 1.25, -1.5, 0.75)))


def main():
    from lag_time import window_ms
    from refine_rate import persons_of
    ap = argparse.ArgumentParser()
    ap.add_argument('--frames', type=int, default=1000)
    ap.add_argument('--persons', type=int, nargs='+', default=[4, 10])
    ap.add_argument('--iters', type=int, default=10)
    ap.add_argument('--reps', type=int, default=9)
    ap.add_argument('--inner', type=int, default=20)
    ap.add_argument('--out', type=str, default=None)
    args = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit('refine_timed_time.py measures on the GPU; none is visible')
    Engine = importlib.import_module(PKG + '.pipeline').Engine
    params = importlib.import_module(PKG + '.parameters').parameters
    syn = importlib.import_module(PKG + '.synthetic')
    sm = list(params.used_cameras_skeleton_matching)
    F = args.frames
    lines = []
    for P in args.persons:
        eng = Engine(params, max_frames=F, max_persons_per_camera=P)
        frames, owners, bodies, _ = syn.lagged_recording(eng.calib, F, [0.0] * len(sm), n_bodies=P, seed=77, step=0.001, weave=0.05)
        db = eng.to_device(eng.pack([{c: [f[c][0], f[c][1]] for c in f} for f in frames]))
        persons_h = persons_of(db.host, owners, sm, eng.pcap)
        poses_h = np.zeros((F, eng.pcap, eng.J, 3))
        poses_h[:, :P] = bodies + np.random.default_rng(78).uniform(-0.01, 0.01, bodies.shape)
        flags_h = np.zeros((F, eng.pcap, eng.J), np.uint8)
        flags_h[:, :P] = 1
        ids_h = np.where(np.arange(eng.pcap) < P, np.arange(eng.pcap), -1).astype(np.int32)[None].repeat(F, axis=0)
        persons, poses, flags, ids = (torch.from_numpy(np.ascontiguousarray(a)).cuda() for a in (persons_h, poses_h, flags_h, ids_h))
        n_persons = torch.full((F,), P, dtype=torch.int32, device='cuda')
        out_u, out_t = torch.empty_like(poses), torch.empty_like(poses)
        kw = dict(max_iters=args.iters, step_tol=0.0)
        untimed = lambda: eng.refine(db, persons, n_persons, poses, flags, 'triang', out=out_u, **kw)      # noqa: E731
        for name, lags in SETTINGS:
            timed = lambda: eng.refine_timed(db, 0, persons, poses, flags, n_persons, ids, 'triang', lags, out=out_t, **kw)      # noqa: E731
            for _ in range(3):                               # warm: both code objects loaded
                res_t, res_u = timed(), untimed()
            torch.cuda.synchronize()
            t_t, t_u = [], []
            for _ in range(args.reps):                       # alternating, so that both see the same machine
                t_t.append(window_ms(timed, args.inner))
                t_u.append(window_ms(untimed, args.inner))
            ms_t, ms_u = float(np.median(t_t)), float(np.median(t_u))
            solved = int((res_t['status'] & 1).ne(0).sum())
            lines.append(json.dumps({'shape': '5x%d' % P, 'pcap': eng.pcap, 'frames': F, 'lags': name, 'iters': args.iters, 'solved': solved,
                                     'offsets_read': int(res_t['n_timed'].sum()), 'iterations_run': int(res_t['iters'].sum()),
                                     'same_bits_as_untimed': bool(torch.equal(out_t, out_u)),
                                     'timed_ms_median': round(ms_t, 4), 'timed_ms_min_max': [round(min(t_t), 4), round(max(t_t), 4)],
                                     'untimed_ms_median': round(ms_u, 4), 'untimed_ms_min_max': [round(min(t_u), 4), round(max(t_u), 4)],
                                     'timed_over_untimed': round(ms_t / ms_u, 3), 'reps': args.reps, 'inner': args.inner}))
            print(lines[-1], flush=True)
        eng.close()
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, 'w') as fh:
            fh.write('\n'.join(lines) + '\n')


if __name__ == '__main__':
    main()
