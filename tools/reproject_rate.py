"""Frames/s of the reprojection harness's scoring step: the host path (`evaluate()` of harness/reprojection_error.py as
it is without --device-metrics: persons and poses copied to the host, per-person dicts, `project()` joint by joint)
against the device path (Engine.reproject for the `est` and the `triang` row + Engine.residual_stats), on the same
1000-frame batches of synthetic 5-camera frames, 4 and 10 persons, whose matching and 3D results are already on the
device.

    python tools/reproject_rate.py [--frames 1000] [--persons 4 10] [--windows 5] [--window-seconds 0.6] [--out profiles/reproject_rate.txt]

This is the SCORING STEP only: matching and the two 3D stages are done before either clock starts, for both sides.
Method: both sides are warmed up once.  The device side is timed with a host clock around a window of repetitions that
ends in a device synchronise (every statistics call reads its results back, which synchronises); the repetition count
is sized from a first estimate so that a window lasts --window-seconds, and --windows windows are taken: their minimum,
median and maximum are recorded, the median is the figure.  The host side runs over the SAME frames of the same batch,
all of them, once (several seconds of Python: one window; --host-frames N limits it to the first N frames, which the
record then says).  The medians of both sides are in the record: they agree to about 1e-5 relative, not bit for bit,
because the host loop's project() rounds in another order than the kernel and its host statement (harness/reprojection.py).  Exit status 1 if the device path is
slower than the host path on any shape.  For kernel times run it under
`rocprofv3 --kernel-trace --stats -- python tools/reproject_rate.py ...` (k_reproject, k_res_hist, k_res_pick, k_res_sum)."""
import argparse
import contextlib
import importlib
import io
import json
import os
import sys
import time

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
PKG = '3d_multi_pose_estimator_amd'


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--frames', type=int, default=1000)
    ap.add_argument('--persons', type=int, nargs='+', default=[4, 10])
    ap.add_argument('--host-frames', type=int, default=0, help='0 = all frames of the batch')
    ap.add_argument('--windows', type=int, default=5)
    ap.add_argument('--window-seconds', type=float, default=0.6)
    ap.add_argument('--distinct', type=int, default=50, help='distinct synthetic frames (tiled up to --frames)')
    ap.add_argument('--out', type=str, default=None)
    args = ap.parse_args()
    rp = importlib.import_module(PKG + '.harness.reprojection_error')
    common = importlib.import_module(PKG + '.harness.common')
    syn = importlib.import_module(PKG + '.synthetic')
    Engine = importlib.import_module(PKG + '.pipeline').Engine
    params = importlib.import_module(PKG + '.parameters').parameters
    calib = importlib.import_module(PKG + '.calibration').Calibration(params)
    names = list(params.camera_names)
    B = args.frames
    lines, slower = [], False
    for P in args.persons:
        made = [syn.make_frame(calib, 5000 + i, syn.FrameSpec(persons=P, noise_px=1.0, float_conf=False)) for i in range(args.distinct)]
        work = [(made[i % len(made)][0], made[i % len(made)][1]['owner']) for i in range(B)]
        frames = [{c: [f[c][0], f[c][1]] for c in f} for f, _ in work]
        eng = Engine(params, calib, max_frames=B, max_persons_per_camera=max(4, P + 1))
        ns = argparse.Namespace(modelsdir='', random_weights=True)
        common.load_models(eng, ns, need_mlp=True)
        db = eng.to_device(eng.pack(frames, keep_json=True))
        persons, n_persons = eng.cluster(db, common.teacher_scores(db, [o for _, o in work]))
        poses, valid = eng.mlp3d(db, persons, n_persons)
        tri, jv = eng.triangulate(db, persons, n_persons, all_joints=True, positive_ids_only=True)
        eng.sync_status()

        def device_once():
            res = [eng.reproject(db, persons, n_persons, poses, valid, 'est'), eng.reproject(db, persons, n_persons, tri, jv, 'triang')]
            return [eng.residual_stats(r) for r in res]            # reads the results back: synchronises
        dev_stats = device_once()                                   # warm-up
        torch.cuda.synchronize()

        def window(reps):
            torch.cuda.synchronize()
            t0 = time.time()
            for _ in range(reps):
                device_once()
            torch.cuda.synchronize()
            return (time.time() - t0) / reps
        reps = max(20, int(args.window_seconds / max(window(20), 1e-6)) + 1)
        dts = sorted(window(reps) for _ in range(args.windows))
        dt_dev = dts[len(dts) // 2]

        N = min(args.host_frames, B) if args.host_frames else B

        def infer(fr, owners):                                      # the tail of run()'s infer: copies + per-person dicts
            h = [t[:N].cpu().numpy() for t in (persons, n_persons, poses, valid, tri, jv)]
            out = []
            for f in range(N):
                heads = db.host.jsons_for_head[f]
                people = []
                for p in range(int(h[1][f])):
                    skels = {cam: heads[int(h[0][f, p, c])] for c, cam in enumerate(names) if h[0][f, p, c] >= 0}
                    people.append((skels, h[2][f, p] if h[3][f, p] else None,
                                   {j: h[4][f, p, j].astype(np.float32) for j in params.joint_list if h[5][f, p, j]}))
                out.append(people)
            return out
        with contextlib.redirect_stdout(io.StringIO()):
            rp.evaluate(work[:2], lambda fr, o: infer(fr, o)[:2], calib, batch=2)          # warm-up
            t0 = time.time()
            host = rp.evaluate(work[:N], infer, calib, batch=N)
            dt_host = (time.time() - t0) / N
        rec = {'shape': '5x%d' % P, 'frames': B, 'pcap': eng.pcap, 'scope': 'scoring step only (matching and 3D stages excluded on both sides)',
               'device_frames_per_s': B / dt_dev, 'device_ms_per_batch': dt_dev * 1e3,
               'device_ms_per_batch_min_median_max': [dts[0] * 1e3, dt_dev * 1e3, dts[-1] * 1e3], 'device_windows': len(dts),
               'device_reps_per_window': reps, 'device_window_seconds': reps * dt_dev,
               'host_frames_per_s': 1.0 / dt_host, 'host_ms_per_frame': dt_host * 1e3, 'host_frames_measured': N, 'host_seconds': dt_host * N,
               'speedup': (B / dt_dev) * dt_host,
               'triang_median_px_device': [float(x) for x in dev_stats[1]['median']],
               'triang_median_px_host': [host.get(('triang', c), (None, None))[1] for c in names],
               'est_median_px_device': [float(x) for x in dev_stats[0]['median']],
               'est_median_px_host': [host.get(('est', c), (None, None))[1] for c in names]}
        slower |= rec['device_frames_per_s'] < rec['host_frames_per_s']
        lines.append(json.dumps(rec))
        print(lines[-1], flush=True)
        eng.close()
    if args.out:
        with open(args.out, 'w') as fh:
            fh.write('# tools/reproject_rate.py on one MI355X: host = evaluate() of harness/reprojection_error.py (copies, dicts, project() per joint);\n'
                     '# device = Engine.reproject (est + triang) + Engine.residual_stats per batch; scoring step only; host clock around synchronised work,\n# both warmed up; device: median of several windows of >= 0.5 s, host: one pass over the same frames\n')
            fh.write('\n'.join(lines) + '\n')
    return 1 if slower else 0


if __name__ == '__main__':
    sys.exit(main())
