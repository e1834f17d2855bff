"""Milliseconds per call of the consolidation (Engine.consolidate / mpe_consolidate_batch) on batches that are already on the
device, beside Engine.regroup and Engine.refine on the same batch and rows, and beside a device copy of half the bytes the
stage must touch.

    python tools/consolidate_time.py [--frames 1000] [--persons 4 10] [--distinct 100] [--reps 9] [--inner 20] [--out FILE]

Per shape 5 x persons: `--frames` synthetic frames (`--distinct` generated, repeated) with 2 px of detection noise, the
rows from the generator's pairing with one body split over two rows (cameras {0,1} | the rest) and one body without a row
per frame, the poses what Engine.triangulate gives on those rows (f64, joint flags, all joints).  Method: warm calls, then
`--reps` regions of `--inner` calls enqueued back to back between two HIP events; the figure is the median region divided by
`--inner`, the spread (min .. max) is printed beside it.  Bytes the stage must touch: per free head xy, vp, camera and joint
mask; per head its camera; per row the entries in and out, the change codes, the view count, the pose and its flags; the two
tables and the free list; per frame the head offset, the person counts in and out, the counts and the status.  The copy moves
half as many bytes (each is read and written).  For the kernel's own time run it under `rocprofv3 --kernel-trace --stats --
python tools/consolidate_time.py ...` (k_consolidate)."""
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


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--frames', type=int, default=1000)
    ap.add_argument('--persons', type=int, nargs='+', default=[4, 10])
    ap.add_argument('--distinct', type=int, default=100, help='frames generated; the batch repeats them')
    ap.add_argument('--reps', type=int, default=9)
    ap.add_argument('--inner', type=int, default=20)
    ap.add_argument('--out', type=str, default=None)
    args = ap.parse_args()
    rt = importlib.import_module('regroup_time')
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
        true_h = rt.persons_of(db.host, [g['owner'] for _, g in made], sm, eng.pcap)
        rows_h = true_h.copy()
        rows_h[:, P - 1] = -1                                            # the last body has no row
        for f in range(args.frames):
            b = f % (P - 1)                                               # this body is split: its cameras beyond the first two in row P - 1
            held = [c for c in range(eng.V) if rows_h[f, b, c] >= 0][2:]
            rows_h[f, P - 1, held], rows_h[f, b, held] = rows_h[f, b, held], -1
        n_h = np.full(args.frames, P, np.int32)
        want_h = true_h.copy()
        want_h[:, P - 1] = -1
        want_h[:, P] = true_h[:, P - 1]
        rows, n_persons = torch.from_numpy(rows_h).cuda(), torch.from_numpy(n_h).cuda()
        poses, jv = eng.triangulate(db, rows, n_persons, all_joints=True)
        eng.sync_status()
        out, n_out, rg_out, ref_out = torch.empty_like(rows), torch.empty_like(n_persons), torch.empty_like(rows), torch.empty_like(poses)
        res = eng.consolidate(db, rows, n_persons, poses, jv, 'triang', out=out, n_out=n_out)
        restored = int((res['persons'].cpu() == torch.from_numpy(want_h)).all(dim=2).all(dim=1).sum())
        counts = res['counts'].sum(dim=0).tolist()
        fcap = int(res['free'].shape[1])
        n_free = int((res['free'] >= 0).sum())
        t_cs = rt.regions(lambda: eng.consolidate(db, rows, n_persons, poses, jv, 'triang', out=out, n_out=n_out), args.reps, args.inner)
        t_rg = rt.regions(lambda: eng.regroup(db, rows, n_persons, poses, jv, 'triang', out=rg_out), args.reps, args.inner)
        t_rf = rt.regions(lambda: eng.refine(db, rows, n_persons, poses, jv, 'triang', out=ref_out), args.reps, args.inner)
        F, H, pcap, V, J = args.frames, db.n_heads, eng.pcap, eng.V, eng.J
        touched = (n_free * (J * 2 * 8 + J * 2 * 4 + 4 + 4) + H * 4 + F * pcap * (V * (4 + 4 + 1) + 4 + J * 3 * 8 + J) + F * pcap * pcap * 8
                   + F * fcap * fcap * 8 + F * fcap * 4 + F * (4 + 4 + 4 + 16 + 4))
        src = torch.empty(touched // 2, dtype=torch.uint8, device='cuda')
        dst = torch.empty_like(src)
        t_cp = rt.regions(lambda: dst.copy_(src), args.reps, args.inner)
        lines.append(json.dumps({'shape': '5x%d' % P, 'pcap': pcap, 'fcap': fcap, 'frames': F, 'heads': H, 'free_heads': n_free, 'poses': 'f64',
                                 'launches_per_call': 1, 'frames_restored': restored, 'counts': counts,
                                 'consolidate_ms_median': round(t_cs[0], 4), 'consolidate_ms_min_max': [round(t_cs[1], 4), round(t_cs[2], 4)],
                                 'regroup_ms_median': round(t_rg[0], 4), 'regroup_ms_min_max': [round(t_rg[1], 4), round(t_rg[2], 4)],
                                 'refine_ms_median': round(t_rf[0], 4), 'refine_ms_min_max': [round(t_rf[1], 4), round(t_rf[2], 4)],
                                 'ratio_to_regroup': round(t_cs[0] / t_rg[0], 2),
                                 'bytes_touched': touched, 'copy_ms_median': round(t_cp[0], 4), 'copy_ms_min_max': [round(t_cp[1], 4), round(t_cp[2], 4)],
                                 'reps': args.reps, 'inner': args.inner}))
        print(lines[-1], flush=True)
        eng.close()
    if args.out:
        with open(args.out, 'w') as fh:
            fh.write('\n'.join(lines) + '\n')


if __name__ == '__main__':
    main()
