"""Milliseconds per pass of the extrinsics calibration (Calibrator.accumulate / mpe_calib_batch) on a batch that is already
on the device, beside Engine.refine (mpe_refine_batch) on the same batch and poses, and the host statement
(harness/calibrate.py) on the same data.

    python tools/calib_time.py [--frames 1000] [--persons 4 10] [--iters 10] [--distinct 100] [--reps 7] [--inner 10] [--out FILE]

Per shape 5 x persons: `--frames` synthetic frames (`--distinct` generated, repeated) with 2 px of detection noise, persons
from the generator's pairing; the poses are what Engine.triangulate returns (f64, joint flags, all joints).  Method, as
tools/refine_rate.py: one warm-up call, then `--reps` regions of `--inner` calls enqueued back to back between two
synchronisations; the figure is the median region divided by `--inner`, the spread (min .. max) is printed beside it.  A
pass is one accumulate() of the whole batch (two launches); the step is timed on its own (it synchronises and solves
on the host).  The refinement runs `--iters` iterations with step_tol = 0.  The host statement is timed once.  For the
kernels' own time run it under `rocprofv3 --kernel-trace --stats -- python tools/calib_time.py ...` (the instantiations of
csrc/normal_sums.h: k_normal_frame<CalibSums, 1>, k_normal_add<28>)."""
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
sys.path.insert(0, os.path.join(ROOT, 'tools'))
PKG = '3d_multi_pose_estimator_amd'


def main():
    from refine_rate import persons_of, regions
    ap = argparse.ArgumentParser()
    ap.add_argument('--frames', type=int, default=1000)
    ap.add_argument('--persons', type=int, nargs='+', default=[4, 10])
    ap.add_argument('--iters', type=int, default=10)
    ap.add_argument('--distinct', type=int, default=100, help='frames generated; the batch repeats them')
    ap.add_argument('--reps', type=int, default=7)
    ap.add_argument('--inner', type=int, default=10)
    ap.add_argument('--out', type=str, default=None)
    args = ap.parse_args()
    Engine = importlib.import_module(PKG + '.pipeline').Engine
    params = importlib.import_module(PKG + '.parameters').parameters
    syn = importlib.import_module(PKG + '.synthetic')
    CB = importlib.import_module(PKG + '.harness.calibrate')
    sm = list(params.used_cameras_skeleton_matching)
    lines = []
    for P in args.persons:
        eng = Engine(params, max_frames=args.frames, max_persons_per_camera=P)
        distinct = [syn.make_frame(eng.calib, i, syn.FrameSpec(persons=P, noise_px=2.0)) for i in range(min(args.frames, args.distinct))]
        made = [distinct[i % len(distinct)] for i in range(args.frames)]
        frames = [{c: [f[c][0], f[c][1]] for c in f} for f, _ in made]
        db = eng.to_device(eng.pack(frames))
        persons_h = persons_of(db.host, [g['owner'] for _, g in made], sm, eng.pcap)
        n_h = np.full(args.frames, P, np.int32)
        persons, n_persons = torch.from_numpy(persons_h).cuda(), torch.from_numpy(n_h).cuda()
        tri, jv = eng.triangulate(db, persons, n_persons, all_joints=True)
        eng.sync_status()
        cal = eng.calibrator('triang', min_obs=6)
        t_pass = regions(lambda: cal.accumulate(db, persons, n_persons, tri, jv), args.reps, args.inner)
        cal.reset()
        cal.accumulate(db, persons, n_persons, tri, jv)
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        rep = cal.step()
        t_step = (time.perf_counter() - t0) * 1e3
        out = torch.empty_like(tri)
        t_ref = regions(lambda: eng.refine(db, persons, n_persons, tri, jv, 'triang', max_iters=args.iters, step_tol=0.0, out=out),
                        args.reps, args.inner)
        t0 = time.perf_counter()
        CB.calib_pass_host(eng.calib, CB.start_extrinsics(eng.calib), db.host, persons_h, n_h, tri.cpu().numpy(), jv.cpu().numpy(), (1 << eng.J) - 1)
        t_host = (time.perf_counter() - t0) * 1e3
        lines.append(json.dumps({'shape': '5x%d' % P, 'pcap': eng.pcap, 'frames': args.frames, 'observations': int(rep['n_obs'].sum()),
                                 'calib_pass_ms_median': round(t_pass[0], 4), 'calib_pass_ms_min_max': [round(t_pass[1], 4), round(t_pass[2], 4)],
                                 'calib_step_ms': round(t_step, 3), 'refine_iters': args.iters, 'refine_ms_median': round(t_ref[0], 4),
                                 'refine_ms_min_max': [round(t_ref[1], 4), round(t_ref[2], 4)], 'host_statement_ms': round(t_host, 1),
                                 'reps': args.reps, 'inner': args.inner}))
        print(lines[-1], flush=True)
        cal.close()
        eng.close()
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, 'w') as fh:
            fh.write('\n'.join(lines) + '\n')


if __name__ == '__main__':
    main()
