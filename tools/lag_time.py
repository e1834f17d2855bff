"""Milliseconds per pass of the time-lag estimate (LagEstimator.accumulate / mpe_lag_batch: k_lag_frame, k_lag_add) on a
batch and a table that are already on the device, beside the calibrator's pass (Calibrator.accumulate / mpe_calib_batch)
over the same batch in the same run.

    python tools/lag_time.py [--frames 1000] [--persons 4 10] [--grids 4,4 8,4] [--reps 9] [--inner 20] [--out FILE]

Per shape 5 x persons: `--frames` frames of bodies on seeded walks (synthetic.walking_bodies, 1 mm per frame so that they
stay in view for the whole recording; every camera at lag 0, the kernel does the same work whatever the lags are), the table
is the true bodies as f64 poses with joint flags, track id = body, persons from the generator's ownership.  Method: warm calls first; then `--reps` windows of `--inner` calls enqueued
back to back between two device events on the stream the calls go to; the figure is the median window divided by `--inner`,
the spread (min .. max) is printed beside it.  A pass is one accumulate() of the whole batch (two launches).  The calibrator's
pass is measured the same way, alternating with the lag passes window by window.  `projections` is the number of supported
observations times K, what the pass projects; K * calib is the calibrator's time times K, the yardstick DESIGN.md 7.15
compares with.  For the kernels' own time run it under `rocprofv3 --kernel-trace --stats -- python tools/lag_time.py ...`."""
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


def window_ms(fn, inner):
    """`inner` calls between two device events -> milliseconds per call."""
    start, stop = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    start.record()
    for _ in range(inner):
        fn()
    stop.record()
    stop.synchronize()
    return start.elapsed_time(stop) / inner


def main():
    from refine_rate import persons_of
    ap = argparse.ArgumentParser()
    ap.add_argument('--frames', type=int, default=1000)
    ap.add_argument('--persons', type=int, nargs='+', default=[4, 10])
    ap.add_argument('--grids', type=str, nargs='+', default=['4,4', '8,4'], help='window,sub pairs')
    ap.add_argument('--reps', type=int, default=9)
    ap.add_argument('--inner', type=int, default=20)
    ap.add_argument('--out', type=str, default=None)
    args = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit('lag_time.py measures on the GPU; none is visible')
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
        poses_h[:, :P] = bodies
        flags_h = np.zeros((F, eng.pcap, eng.J), np.uint8)
        flags_h[:, :P] = 1
        ids_h = np.where(np.arange(eng.pcap) < P, np.arange(eng.pcap), -1).astype(np.int32)[None].repeat(F, axis=0)
        persons, poses, flags, ids = (torch.from_numpy(np.ascontiguousarray(a)).cuda() for a in (persons_h, poses_h, flags_h, ids_h))
        n_persons = torch.full((F,), P, dtype=torch.int32, device='cuda')
        cal = eng.calibrator('triang', min_obs=6)
        calib_pass = lambda: cal.accumulate(db, persons, n_persons, poses, flags)      # noqa: E731
        for window, sub in (tuple(int(x) for x in g.split(',')) for g in args.grids):
            est = eng.lag_estimator('triang', window=window, sub=sub)
            lag_pass = lambda: est.accumulate(db, 0, persons, poses, flags, n_persons, ids)      # noqa: E731
            for _ in range(3):                               # warm: both code objects loaded, the workspaces touched
                lag_pass()
                calib_pass()
            torch.cuda.synchronize()
            t_lag, t_cal = [], []
            for _ in range(args.reps):                       # alternating, so that both see the same machine
                t_lag.append(window_ms(lag_pass, args.inner))
                t_cal.append(window_ms(calib_pass, args.inner))
            est.reset()
            lag_pass()
            sums = est.read()
            K = est.K
            lag_ms, cal_ms = float(np.median(t_lag)), float(np.median(t_cal))
            lines.append(json.dumps({'shape': '5x%d' % P, 'pcap': eng.pcap, 'frames': F, 'window': window, 'sub': sub, 'K': K,
                                     'supported': int(sums['n_support'].sum()), 'projections': int(sums['n_support'].sum()) * K,
                                     'lag_pass_ms_median': round(lag_ms, 4), 'lag_pass_ms_min_max': [round(min(t_lag), 4), round(max(t_lag), 4)],
                                     'calib_pass_ms_median': round(cal_ms, 4), 'calib_pass_ms_min_max': [round(min(t_cal), 4), round(max(t_cal), 4)],
                                     'K_times_calib_ms': round(K * cal_ms, 4), 'lag_over_K_calib': round(lag_ms / (K * cal_ms), 3),
                                     'ns_per_projection': round(lag_ms * 1e6 / max(1, int(sums['n_support'].sum()) * K), 3),
                                     'reps': args.reps, 'inner': args.inner}))
            print(lines[-1], flush=True)
            est.close()
        cal.close()
        eng.close()
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, 'w') as fh:
            fh.write('\n'.join(lines) + '\n')


if __name__ == '__main__':
    main()
