"""Milliseconds per call of the pose covariance (Engine.pose_covariance / mpe_posecov_batch: k_posecov) on a batch that is
already on the device, beside one iteration of the refinement (Engine.refine with max_iters = 1 / mpe_refine_batch: k_refine)
and the reprojection residuals (Engine.reproject / mpe_reproject_batch) on the same batch and poses in the same run.

    python tools/posecov_time.py [--frames 1000] [--persons 4 10] [--reps 9] [--inner 20] [--out FILE]

Per shape 5 x persons: the recording and the poses of tools/refine_timed_time.py (bodies on seeded walks, every camera at lag
0; the true bodies moved by up to 1 cm per coordinate as f64 poses with joint flags, persons from the generator's ownership).
Method, that of profiles/refine_timed_timing.txt: warm calls first; then `--reps` windows of `--inner` calls enqueued back to
back between two device events on the stream the calls go to, the three stages alternating; the figure is the median window
divided by `--inner`, the spread (min .. max) is printed beside it.  A call is the C entry point on an argument block and
output tensors made once, so a window holds no allocation.  For the kernels' own time run it under
`rocprofv3 --kernel-trace --stats -- python tools/posecov_time.py ...`."""
import argparse
import ctypes as C
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
    from lag_time import window_ms
    from refine_rate import persons_of
    ap = argparse.ArgumentParser()
    ap.add_argument('--frames', type=int, default=1000)
    ap.add_argument('--persons', type=int, nargs='+', default=[4, 10])
    ap.add_argument('--reps', type=int, default=9)
    ap.add_argument('--inner', type=int, default=20)
    ap.add_argument('--out', type=str, default=None)
    args = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit('posecov_time.py measures on the GPU; none is visible')
    Engine = importlib.import_module(PKG + '.pipeline').Engine
    params = importlib.import_module(PKG + '.parameters').parameters
    syn = importlib.import_module(PKG + '.synthetic')
    L = importlib.import_module(PKG + '.lib')
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
        persons, poses, flags = (torch.from_numpy(np.ascontiguousarray(a)).cuda() for a in (persons_h, poses_h, flags_h))
        n_persons = torch.full((F,), P, dtype=torch.int32, device='cuda')
        # the C calls themselves, on argument blocks and output tensors made once: a window is then the kernels back to back, not
        # the allocations and argument checks of the Python methods (whose results these are: `res` below)
        res = (eng.pose_covariance(db, persons, n_persons, poses, flags, 'triang', 1.0),
               eng.refine(db, persons, n_persons, poses, flags, 'triang', max_iters=1, step_tol=0.0),
               eng.reproject(db, persons, n_persons, poses, flags, 'triang'))
        blocks = []
        for struct, extra in ((L.mpe_posecov_args, dict(huber_px=0.0, sigma_px=1.0, gate_m=0.0, d_cov=res[0]['cov'], d_sigma=res[0]['sigma'],
                                                        d_status=res[0]['status'], d_n_views=res[0]['n_views'])),
                              (L.mpe_refine_args, dict(max_iters=1, step_tol=0.0, huber_px=0.0, d_poses_out=res[1]['poses'], d_status=res[1]['status'],
                                                       d_cost0=res[1]['cost0'], d_cost1=res[1]['cost1'], d_iters=res[1]['iters'],
                                                       d_n_views=res[1]['n_views'])),
                              (L.mpe_reproject_args, dict(d_res=res[2]))):
            a = struct()
            a.n_frames, a.pcap, a.n_joints, a.pose_f64, a.joint_flags, a.joint_mask, a.threshold = F, eng.pcap, eng.J, 1, 1, (1 << eng.J) - 1, 0.5
            a.d_persons, a.d_n_persons, a.d_poses, a.d_flags = persons.data_ptr(), n_persons.data_ptr(), poses.data_ptr(), flags.data_ptr()
            for k, v in extra.items():
                setattr(a, k, v.data_ptr() if torch.is_tensor(v) else v)
            blocks.append(a)
        stream = eng._stream()
        call = lambda fn, a: (lambda: eng._chk(fn(eng.ctx, stream, C.byref(db.struct), C.byref(a))))      # noqa: E731
        stages = (('posecov', call(eng.lib.mpe_posecov_batch, blocks[0])), ('refine_1_iter', call(eng.lib.mpe_refine_batch, blocks[1])),
                  ('reproject', call(eng.lib.mpe_reproject_batch, blocks[2])))
        for _ in range(3):                                   # warm: every code object loaded
            for _, fn in stages:
                fn()
        torch.cuda.synchronize()
        t = {name: [] for name, _ in stages}
        for _ in range(args.reps):                           # alternating, so that all see the same machine
            for name, fn in stages:
                t[name].append(window_ms(fn, args.inner))
        row = {'shape': '5x%d' % P, 'pcap': eng.pcap, 'frames': F, 'computed': int((res[0]['status'] & 1).ne(0).sum()),
               'solved': int((res[1]['status'] & 1).ne(0).sum()), 'residuals': int((res[2] >= 0).sum()), 'reps': args.reps, 'inner': args.inner}
        for name, _ in stages:
            row[name + '_ms_median'] = round(float(np.median(t[name])), 4)
            row[name + '_ms_min_max'] = [round(min(t[name]), 4), round(max(t[name]), 4)]
        row['posecov_over_refine_1_iter'] = round(row['posecov_ms_median'] / row['refine_1_iter_ms_median'], 3)
        lines.append(json.dumps(row))
        print(lines[-1], flush=True)
        eng.close()
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, 'w') as fh:
            fh.write('\n'.join(lines) + '\n')


if __name__ == '__main__':
    main()
