"""Milliseconds per pass of the camera fit (CameraFitter.accumulate / mpe_camfit_batch) beside the extrinsics calibration
(Calibrator.accumulate / mpe_calib_batch), alternating in the same run on the same batch that is already on the device.

    python tools/camfit_time.py [--frames 1000] [--persons 4 10] [--distinct 100] [--reps 9] [--inner 50] [--out FILE]

Per shape 5 x persons: the batch and poses of tools/calib_time.py (`--frames` synthetic frames, 2 px of detection noise,
persons from the generator's pairing, the poses Engine.triangulate returns).  Method, as tools/calib_time.py: one warm-up
call each, then `--reps` rounds; a round is one region of `--inner` camera-fit passes enqueued back to back between two
synchronisations followed by one such region of calibration passes, so that the two see the same clocks and the same
neighbours.  The figure is the median region divided by `--inner`, the spread (min .. max) beside it, and the ratio of the
medians.  A pass is one accumulate() of the whole batch (two launches).  The step is timed once on its own.  For the
kernels' own time run it under `rocprofv3 --kernel-trace --stats -- python tools/camfit_time.py ...` (the instantiations of
csrc/normal_sums.h: k_normal_frame<CamfitSums, 2>, k_normal_add<105>, k_normal_frame<CalibSums, 1>, k_normal_add<28>), in a run
of its own."""
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


def region(fn, inner):
    t0 = time.perf_counter()
    for _ in range(inner):
        fn()
    torch.cuda.synchronize()
    return (time.perf_counter() - t0) * 1e3 / inner


def main():
    from refine_rate import persons_of
    ap = argparse.ArgumentParser()
    ap.add_argument('--frames', type=int, default=1000)
    ap.add_argument('--persons', type=int, nargs='+', default=[4, 10])
    ap.add_argument('--distinct', type=int, default=100, help='frames generated; the batch repeats them')
    ap.add_argument('--reps', type=int, default=9)
    ap.add_argument('--inner', type=int, default=50)
    ap.add_argument('--out', type=str, default=None)
    args = ap.parse_args()
    Engine = importlib.import_module(PKG + '.pipeline').Engine
    params = importlib.import_module(PKG + '.parameters').parameters
    syn = importlib.import_module(PKG + '.synthetic')
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
        fit, cal = eng.camera_fitter('triang', min_obs=13), eng.calibrator('triang', min_obs=6)
        passes = {'camfit': lambda: fit.accumulate(db, persons, n_persons, tri, jv), 'calib': lambda: cal.accumulate(db, persons, n_persons, tri, jv)}
        for fn in passes.values():
            fn()
        torch.cuda.synchronize()
        ms = {k: [] for k in passes}
        for _ in range(args.reps):
            for k, fn in passes.items():
                ms[k].append(region(fn, args.inner))
        fit.reset()
        fit.accumulate(db, persons, n_persons, tri, jv)
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        rep = fit.step()
        t_step = (time.perf_counter() - t0) * 1e3
        med = {k: float(np.median(v)) for k, v in ms.items()}
        lines.append(json.dumps({'shape': '5x%d' % P, 'pcap': eng.pcap, 'frames': args.frames, 'observations': int(rep['n_obs'].sum()),
                                 'camfit_pass_ms_median': round(med['camfit'], 4), 'camfit_pass_ms_min_max': [round(min(ms['camfit']), 4), round(max(ms['camfit']), 4)],
                                 'calib_pass_ms_median': round(med['calib'], 4), 'calib_pass_ms_min_max': [round(min(ms['calib']), 4), round(max(ms['calib']), 4)],
                                 'ratio_of_medians': round(med['camfit'] / med['calib'], 3), 'camfit_step_ms': round(t_step, 3),
                                 'reps': args.reps, 'inner': args.inner}))
        print(lines[-1], flush=True)
        fit.close()
        cal.close()
        eng.close()
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, 'w') as fh:
            fh.write('\n'.join(lines) + '\n')


if __name__ == '__main__':
    main()
