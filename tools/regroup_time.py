"""Milliseconds per call of the regrouping (Engine.regroup / mpe_regroup_batch) on batches that are already on the device,
beside Engine.refine on the same batch and rows, and beside a device copy of as many bytes as the stage must touch.

    python tools/regroup_time.py [--frames 1000] [--persons 4 10] [--distinct 100] [--reps 9] [--inner 20] [--out FILE]

Per shape 5 x persons: `--frames` synthetic frames (`--distinct` generated, repeated) with 2 px of detection noise, the
rows from the generator's pairing with one exchange and one missing head per frame, the poses what Engine.triangulate
gives on the true rows (f64, joint flags, all joints).  Method: warm calls, then `--reps` regions of `--inner` calls
enqueued back to back between two HIP events; the figure is the median region divided by `--inner`, the spread (min ..
max) is printed beside it.  Bytes the stage must touch: per head xy, vp, camera and joint mask; per row the entries in and
out, the change codes, the view count, the pose and its flags; the cost table; per frame the head offset, the person
count, the counts and the status.  The copy moves half as many bytes (each is read and written).  For the kernel's own
time run it under `rocprofv3 --kernel-trace --stats -- python tools/regroup_time.py ...` (k_regroup)."""
import argparse
import importlib
import json
import os
import sys

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
    for _ in range(3):
        fn()
    torch.cuda.synchronize()
    ms = []
    for _ in range(reps):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record()
        for _ in range(inner):
            fn()
        b.record()
        b.synchronize()
        ms.append(a.elapsed_time(b) / inner)
    return float(np.median(ms)), float(min(ms)), float(max(ms))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--frames', type=int, default=1000)
    ap.add_argument('--persons', type=int, nargs='+', default=[4, 10])
    ap.add_argument('--distinct', type=int, default=100, help='frames generated; the batch repeats them')
    ap.add_argument('--reps', type=int, default=9)
    ap.add_argument('--inner', type=int, default=20)
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
        true_h = persons_of(db.host, [g['owner'] for _, g in made], sm, eng.pcap)
        n_h = np.full(args.frames, P, np.int32)
        rows_h = true_h.copy()
        for f in range(args.frames):
            c, p = f % eng.V, f % (P - 1)
            if rows_h[f, p, c] >= 0 and rows_h[f, p + 1, c] >= 0:
                rows_h[f, [p, p + 1], c] = rows_h[f, [p + 1, p], c]
            rows_h[f, (f + 2) % P, (f + 1) % eng.V] = -1
        true, rows, n_persons = torch.from_numpy(true_h).cuda(), torch.from_numpy(rows_h).cuda(), torch.from_numpy(n_h).cuda()
        poses, jv = eng.triangulate(db, true, n_persons, all_joints=True)
        eng.sync_status()
        out, ref_out = torch.empty_like(rows), torch.empty_like(poses)
        res = eng.regroup(db, rows, n_persons, poses, jv, 'triang', out=out)
        restored = int((res['persons'] == true).all(dim=2).all(dim=1).sum())
        counts = res['counts'].sum(dim=0).tolist()
        t_rg = regions(lambda: eng.regroup(db, rows, n_persons, poses, jv, 'triang', out=out), args.reps, args.inner)
        t_rf = regions(lambda: eng.refine(db, rows, n_persons, poses, jv, 'triang', out=ref_out), args.reps, args.inner)
        F, H, pcap, V, J = args.frames, db.n_heads, eng.pcap, eng.V, eng.J
        touched = H * (J * 2 * 8 + J * 2 * 4 + 4 + 4) + F * pcap * (V * (4 + 4 + 1) + 4 + J * 3 * 8 + J) + H * pcap * 8 + F * (4 + 4 + 16 + 4)
        src = torch.empty(touched // 2, dtype=torch.uint8, device='cuda')
        dst = torch.empty_like(src)
        t_cp = regions(lambda: dst.copy_(src), args.reps, args.inner)
        lines.append(json.dumps({'shape': '5x%d' % P, 'pcap': pcap, 'frames': F, 'heads': H, 'pairs': H * pcap, 'poses': 'f64', 'launches_per_call': 1,
                                 'frames_restored': restored, 'counts': counts,
                                 'regroup_ms_median': round(t_rg[0], 4), 'regroup_ms_min_max': [round(t_rg[1], 4), round(t_rg[2], 4)],
                                 'refine_ms_median': round(t_rf[0], 4), 'refine_ms_min_max': [round(t_rf[1], 4), round(t_rf[2], 4)],
                                 'bytes_touched': touched, 'copy_ms_median': round(t_cp[0], 4), 'copy_ms_min_max': [round(t_cp[1], 4), round(t_cp[2], 4)],
                                 'reps': args.reps, 'inner': args.inner}))
        print(lines[-1], flush=True)
        eng.close()
    if args.out:
        with open(args.out, 'w') as fh:
            fh.write('\n'.join(lines) + '\n')


if __name__ == '__main__':
    main()
