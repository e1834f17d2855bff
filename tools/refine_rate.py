"""Milliseconds per call of the refinement (Engine.refine / mpe_refine_batch) on batches that are already on the device,
beside the host statement (harness/refine.py) on the same data and Engine.triangulate on the same batch for scale.

    python tools/refine_rate.py [--frames 1000] [--persons 4 10] [--iters 10] [--distinct 100] [--reps 7] [--inner 10] [--out FILE]

Per shape 5 x persons: `--frames` synthetic frames (`--distinct` generated, repeated) with 2 px of detection noise, persons
from the generator's pairing;
`triang` refines what Engine.triangulate returns (f64, joint flags, all joints), `est` the bodies moved by up to 3 cm as
f32 poses with person flags (the used joints).  Method: one warm-up call, then `--reps` regions of `--inner` calls
enqueued back to back between two synchronisations; the figure is the median region divided by `--inner`, the spread
(min .. max) is printed beside it.  step_tol = 0, so every joint runs all `--iters` iterations.  The host statement is
timed once.  For the kernel's own time run it under `rocprofv3 --kernel-trace --stats -- python tools/refine_rate.py ...`
(k_refine)."""
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


def persons_of(pb, owners, sm, pcap):
    persons = np.full((pb.n_frames, pcap, pb.V), -1, np.int32)
    for f in range(pb.n_frames):
        h0, H, _, _ = pb.frame_counts(f)
        for i in range(H):
            c = int(pb.head_cam[h0 + i])
            o = owners[f][sm[c]][int(pb.skeleton_index[h0 + i])]
            if 0 <= o < pcap:
                persons[f, o, c] = i
    return persons


def regions(fn, reps, inner):
    fn()
    torch.cuda.synchronize()
    ms = []
    for _ in range(reps):
        t0 = time.perf_counter()
        for _ in range(inner):
            fn()
        torch.cuda.synchronize()
        ms.append((time.perf_counter() - t0) * 1e3 / inner)
    return float(np.median(ms)), float(min(ms)), float(max(ms))


def main():
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
    RF = importlib.import_module(PKG + '.harness.refine')
    sm = list(params.used_cameras_skeleton_matching)
    used = sum(1 << j for j in params.used_joints)
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
        rng = np.random.default_rng(0)
        est_h = np.zeros((args.frames, eng.pcap, eng.J, 3), np.float32)
        for f, (_, g) in enumerate(made):
            est_h[f, :P] = g['persons'] + rng.uniform(-0.03, 0.03, g['persons'].shape)
        ok_h = (np.arange(eng.pcap)[None, :] < n_h[:, None]).astype(np.uint8)
        est, ok = torch.from_numpy(est_h).cuda(), torch.from_numpy(ok_h).cuda()
        eng.sync_status()
        t_tri = regions(lambda: eng.triangulate(db, persons, n_persons, all_joints=True), args.reps, args.inner)
        for kind, poses, flags, mask in (('triang', tri, jv, (1 << eng.J) - 1), ('est', est, ok, used)):
            out = torch.empty_like(poses)
            t_dev = regions(lambda: eng.refine(db, persons, n_persons, poses, flags, kind, max_iters=args.iters, step_tol=0.0, out=out),
                            args.reps, args.inner)
            res = eng.refine(db, persons, n_persons, poses, flags, kind, max_iters=args.iters, step_tol=0.0)
            solved = int((res['status'] & RF.SOLVED).bool().sum())
            t0 = time.perf_counter()
            RF.refine(eng.calib, db.host, persons_h, n_h, poses.cpu().numpy(), flags.cpu().numpy(), mask, max_iters=args.iters, step_tol=0.0)
            t_host = (time.perf_counter() - t0) * 1e3
            lines.append(json.dumps({'shape': '5x%d' % P, 'pcap': eng.pcap, 'frames': args.frames, 'poses': kind, 'iters': args.iters,
                                     'joints_solved': solved, 'refine_ms_median': round(t_dev[0], 4), 'refine_ms_min_max': [round(t_dev[1], 4), round(t_dev[2], 4)],
                                     'host_statement_ms': round(t_host, 1), 'triangulate_ms_median': round(t_tri[0], 4),
                                     'reps': args.reps, 'inner': args.inner}))
            print(lines[-1], flush=True)
        eng.close()
    if args.out:
        with open(args.out, 'w') as fh:
            fh.write('\n'.join(lines) + '\n')


if __name__ == '__main__':
    main()
