"""Milliseconds per call of the body-level fit (Engine.body_refine / mpe_body_refine_batch) on batches that are already on the
device, beside the pair of launches it stands in for -- Engine.refine(max_iters=sweeps) then Skeleton.fit(iters=sweeps) on
the same batch and rows -- and beside a device copy of as many bytes as the stage must touch.

    python tools/skel_refine_time.py [--frames 1000] [--persons 4 10] [--sweeps 8 16] [--distinct 100] [--reps 9] [--inner 20] [--out FILE]

Per shape 5 x persons: `--frames` synthetic frames (`--distinct` generated, repeated) with 2 px of detection noise, the
rows from the generator's pairing, the poses what Engine.triangulate gives on them (f64, joint flags, all joints), row p
of every frame track p, the lengths those of the generator's bodies.  Method: warm calls, then `--reps` regions of
`--inner` calls enqueued back to back between two HIP events; the figure is the median region divided by `--inner`, the
spread (min .. max) is printed beside it.  Bytes the stage must touch: per head xy, vp and the joint mask; per row the
heads, the id, the pose in and out with its flags, status, views, cost, error and bone count, and the row's lengths; per
frame the head offset, the person count and the frame map.  The copy moves half as many bytes (each is read and
written).  For the kernel's own time run it under `rocprofv3 --kernel-trace --stats -- python tools/skel_refine_time.py ...`
(k_skel_refine)."""
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
    ap.add_argument('--sweeps', type=int, nargs='+', default=[8, 16])
    ap.add_argument('--distinct', type=int, default=100, help='frames generated; the batch repeats them')
    ap.add_argument('--reps', type=int, default=9)
    ap.add_argument('--inner', type=int, default=20)
    ap.add_argument('--out', type=str, default=None)
    args = ap.parse_args()
    if not torch.cuda.is_available():
        sys.exit('skel_refine_time.py measures on the GPU and there is none')
    rt = importlib.import_module('regroup_time')
    Engine = importlib.import_module(PKG + '.pipeline').Engine
    params = importlib.import_module(PKG + '.parameters').parameters
    syn = importlib.import_module(PKG + '.synthetic')
    S = importlib.import_module(PKG + '.harness.skeleton')
    sm = list(params.used_cameras_skeleton_matching)
    lines = []
    for P in args.persons:
        eng = Engine(params, max_frames=args.frames, max_persons_per_camera=P)
        distinct = [syn.make_frame(eng.calib, i, syn.FrameSpec(persons=P, noise_px=2.0)) for i in range(min(args.frames, args.distinct))]
        made = [distinct[i % len(distinct)] for i in range(args.frames)]
        frames = [{c: [f[c][0], f[c][1]] for c in f} for f, _ in made]
        db = eng.to_device(eng.pack(frames))
        F, H, pcap, V, J = args.frames, db.n_heads, eng.pcap, eng.V, eng.J
        rows = torch.from_numpy(rt.persons_of(db.host, [g['owner'] for _, g in made], sm, pcap)).cuda()
        n_persons = torch.from_numpy(np.full(F, P, np.int32)).cuda()
        poses, jv = eng.triangulate(db, rows, n_persons, all_joints=True)
        eng.sync_status()
        ids = torch.from_numpy(np.tile(np.where(np.arange(pcap) < P, np.arange(pcap), -1).astype(np.int32), (F, 1))).cuda()
        # row p is a different body in every distinct frame: the table holds the mean lengths, which is all a timing needs
        bodies = np.stack([g['persons'][:P] for _, g in distinct])                       # [distinct, P, J, 3]
        d = bodies[:, :, [b[1] for b in S.BONES_18]] - bodies[:, :, [b[0] for b in S.BONES_18]]
        table = np.zeros((256, len(S.BONES_18)))
        table[:P] = np.sqrt((d * d).sum(axis=-1)).mean(axis=0)
        sk = eng.skeleton('tri', tid_cap=256)
        sk.set_lengths(table)
        ref_out = torch.empty_like(poses)
        for sweeps in args.sweeps:
            res = eng.body_refine(sk, db, rows, n_persons, poses, jv, ids, sweeps=sweeps)
            fitted, free = int((res['n_bones'] > 0).sum()), int(((res['status'] & 1) != 0).sum())
            moved = int(((res['status'] & 2) != 0).sum())
            t_body = rt.regions(lambda: eng.body_refine(sk, db, rows, n_persons, poses, jv, ids, sweeps=sweeps), args.reps, args.inner)
            t_rf = rt.regions(lambda: eng.refine(db, rows, n_persons, poses, jv, 'triang', max_iters=sweeps, step_tol=0.0, out=ref_out), args.reps, args.inner)
            t_fit = rt.regions(lambda: sk.fit(ref_out, jv, n_persons, ids, iters=sweeps), args.reps, args.inner)

            def pair():
                eng.refine(db, rows, n_persons, poses, jv, 'triang', max_iters=sweeps, step_tol=0.0, out=ref_out)
                sk.fit(ref_out, jv, n_persons, ids, iters=sweeps)
            t_pair = rt.regions(pair, args.reps, args.inner)
            touched = (H * (J * 2 * 8 + J * 2 * 4 + 4) + F * pcap * (V * 4 + 4 + 2 * J * 3 * 8 + J + 2 * J + 4 * 8 + 2 * 8 + 1 + len(S.BONES_18) * 8)
                       + F * (4 + 4 + 4))
            src = torch.empty(touched // 2, dtype=torch.uint8, device='cuda')
            dst = torch.empty_like(src)
            t_cp = rt.regions(lambda: dst.copy_(src), args.reps, args.inner)
            r4 = lambda t: [round(t[0], 4), round(t[1], 4), round(t[2], 4)]
            lines.append(json.dumps({'shape': '5x%d' % P, 'pcap': pcap, 'frames': F, 'heads': H, 'poses': 'f64', 'sweeps': sweeps, 'launches_per_call': 1,
                                     'rows_fitted': fitted, 'free_joints': free, 'joints_moved': moved,
                                     'body_fit_ms_median_min_max': r4(t_body), 'refine_ms_median_min_max': r4(t_rf),
                                     'fit_ms_median_min_max': r4(t_fit), 'pair_ms_median_min_max': r4(t_pair),
                                     'ratio_to_pair': round(t_body[0] / t_pair[0], 3), 'bytes_touched': touched,
                                     'copy_ms_median_min_max': r4(t_cp), 'reps': args.reps, 'inner': args.inner}))
            print(lines[-1], flush=True)
        sk.close()
        eng.close()
    if args.out:
        with open(args.out, 'w') as fh:
            fh.write('\n'.join(lines) + '\n')


if __name__ == '__main__':
    main()
