"""Frames/s of the ground-truth step of a --device-metrics batch: the host path (json.load of the document, then
harness.common.pack_ground_truth and harness.partition.pack_bodies over the loaded frames) against the device path
(Engine.bodies_from_json: staging of the bodies' text, one copy, the parse kernels and the status read-back; then
Engine.ground_truth), on 1000-frame documents of synthetic 5-camera frames with 4 and 10 persons.

    python tools/gt_rate.py [--frames 1000] [--persons 4 10] [--windows 5] [--out profiles/gt_rate.txt]

Method: the document is built once per shape (json.dumps of synthetic frames); each path is run once to warm up and then
--windows times, every run timed with time.perf_counter and ended by a read-back (the device path) -- the median is the
figure, minimum and maximum are recorded.  The host figure is recorded with and without its json.load.  The device
figure includes the document index (mpe_json_index) being built for every run.  The arrays of the two paths are compared
before anything is timed.  With --loop the --device-metrics loop of harness/metrics_from_model.py runs on the same file
with and without --device-gt and its wall time is recorded.  For kernel times run the tool under `rocprofv3
--kernel-trace --stats -- python tools/gt_rate.py ...` (k_body_braces, k_body_layout, k_body_walk, k_gt_from_bodies)."""
import argparse
import contextlib
import importlib
import io
import json
import os
import statistics
import sys
import tempfile
import time

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
PKG = '3d_multi_pose_estimator_amd'


def timed(fn, windows):
    fn()
    ts = []
    for _ in range(windows):
        t0 = time.perf_counter()
        fn()
        ts.append(time.perf_counter() - t0)
    return min(ts), statistics.median(ts), max(ts)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--frames', type=int, default=1000)
    ap.add_argument('--persons', type=int, nargs='+', default=[4, 10])
    ap.add_argument('--windows', type=int, default=5)
    ap.add_argument('--distinct', type=int, default=50, help='distinct synthetic frames (tiled up to --frames)')
    ap.add_argument('--loop', action='store_true', help='also time harness/metrics_from_model.py --device-metrics with and without --device-gt')
    ap.add_argument('--out', type=str, default=None)
    args = ap.parse_args()
    common = importlib.import_module(PKG + '.harness.common')
    part = importlib.import_module(PKG + '.harness.partition')
    syn = importlib.import_module(PKG + '.synthetic')
    packing = importlib.import_module(PKG + '.packing')
    Engine = importlib.import_module(PKG + '.pipeline').Engine
    params = importlib.import_module(PKG + '.parameters').parameters
    calib = importlib.import_module(PKG + '.calibration').Calibration(params)
    B = args.frames
    T_d1 = torch.from_numpy(calib.T_d[1]).type(torch.float32)
    T_i1 = torch.from_numpy(calib.T_i32[1])
    shown = [a for i, a in enumerate(sys.argv[1:], 1) if a != '--out' and sys.argv[i - 1] != '--out']      # where the record goes is not part of it
    prop = torch.cuda.get_device_properties(0)
    lines = ['board: %s (%s, %d CUs)' % (prop.name, getattr(prop, 'gcnArchName', '?'), prop.multi_processor_count),
             'command: python tools/gt_rate.py ' + ' '.join(shown)]
    for P in args.persons:
        made = [syn.make_frame(calib, 7000 + i, syn.FrameSpec(persons=P, noise_px=1.0))[0] for i in range(args.distinct)]
        text = json.dumps([made[i % len(made)] for i in range(B)]).encode()
        eng = Engine(params, calib, max_frames=B, max_persons_per_camera=max(4, P + 1))
        scap = 2 * eng.hpf
        state = {}

        def host(load=True):
            frames = json.loads(text) if load else state['frames']
            state['frames'] = frames
            state['gt'] = common.pack_ground_truth(frames, [T_d1] * len(frames), T_i1)
            state['packed'] = part.pack_bodies(frames)

        def device():
            pb = eng.bodies_from_json(text, 0, 1, B, scap=scap)
            assert pb.status == 0, pb.status
            gt = eng.ground_truth(pb, [T_d1.numpy()], np.zeros(B, np.int32), T_i1.numpy())
            state['n'] = gt['n'].cpu()
            state['dgt'], state['pb'] = gt, pb

        host()
        device()
        gc = state['gt']['xyz'].shape[1]
        same = (np.array_equal(state['dgt']['xyz'].cpu().numpy()[:, :gc].view(np.uint32), state['gt']['xyz'].view(np.uint32)) and
                np.array_equal(state['n'].numpy(), state['gt']['n']) and np.array_equal(state['pb'].n.cpu().numpy(), state['packed']['n']))
        h_all, h_nol, d = timed(host, args.windows), timed(lambda: host(False), args.windows), timed(device, args.windows)
        lines.append('5x%d, %d frames, %.1f MB of JSON, arrays equal: %s' % (P, B, len(text) / 1e6, same))
        lines.append('  host json.load + pack_ground_truth + pack_bodies: %.1f frames/s (median of %d; %.3f / %.3f / %.3f s)' % ((B / h_all[1], args.windows) + h_all))
        lines.append('  host without json.load:                           %.1f frames/s (%.3f / %.3f / %.3f s)' % ((B / h_nol[1],) + h_nol))
        lines.append('  device index + staging + copy + kernels + status: %.1f frames/s (%.4f / %.4f / %.4f s), %.1fx the host figure' %
                     ((B / d[1],) + d + (h_all[1] / d[1],)))
        if args.loop:
            with tempfile.TemporaryDirectory() as tmp:
                path = os.path.join(tmp, 'syn_rate_test.json')
                with open(path, 'wb') as fh:
                    fh.write(text)
                from types import SimpleNamespace
                tm = SimpleNamespace(get_transform=lambda a, b: calib.T_d[1])
                common.dataset_transform = lambda d_, f_: tm
                m = importlib.import_module(PKG + '.harness.metrics_from_model')
                res = {}
                for flag in ('--device-metrics', '--device-gt'):
                    argv = ['--testfiles', path, '--tmdir', tmp, '--random-weights', '--datastep', '1', '--batch', str(B), '--persons', str(P), flag]
                    ts = []
                    for _ in range(2):
                        t0 = time.perf_counter()
                        with contextlib.redirect_stdout(io.StringIO()):
                            res[flag] = m.main(argv)
                        ts.append(time.perf_counter() - t0)
                    lines.append('  metrics_from_model %s, whole script (second of two runs): %.2f s, n_data %d' % (flag, ts[1], res[flag]['n_data']))
        eng.close()
    out = '\n'.join(lines) + '\n'
    print(out, end='')
    if args.out:
        with open(args.out, 'w') as fh:
            fh.write(out)


if __name__ == '__main__':
    main()
