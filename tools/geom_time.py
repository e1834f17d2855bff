"""Milliseconds per call of the geometric matcher (Engine.geom_scores / mpe_geom_scores_batch, Engine.geom_match /
mpe_geom_match_batch) beside the clustering alone (Engine.cluster / mpe_cluster_batch) and the GAT route it stands in for
(Engine.match / mpe_match_batch), all on the same batch, which is already on the device.

    python tools/geom_time.py [--frames 1000] [--persons 4] [--reps 30] [--calls 20] [--out FILE]

The benchmark's batch: 5 views x `persons` people, `--frames` frames (250 distinct, repeated, as bench.py builds them) and
its hash-initialised GAT weights.  One repeat is `--calls` calls enqueued back to back between two events on the current
stream; the four are measured in alternation after a warm-up and the median of the `--reps` repeats is reported with the
spread (min, max).  The output tensors are allocated once, outside the timed calls (the C entry points are called as a C
host would).  For kernel times run it under `rocprofv3 --kernel-trace --stats -- python tools/geom_time.py ...` (k_geom,
k_topology, the clustering kernels)."""
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
PKG = '3d_multi_pose_estimator_amd'


def timed(fn, calls):
    """ms per call of `calls` calls of fn between two events on the current stream"""
    start, stop = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    start.record()
    for _ in range(calls):
        fn()
    stop.record()
    stop.synchronize()
    return start.elapsed_time(stop) / calls


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--frames', type=int, default=1000)
    ap.add_argument('--persons', type=int, default=4)
    ap.add_argument('--reps', type=int, default=30)
    ap.add_argument('--calls', type=int, default=20)
    ap.add_argument('--out', type=str, default=None)
    args = ap.parse_args()
    if not torch.cuda.is_available():
        sys.exit('geom_time.py measures on the GPU and there is none')
    pipeline = importlib.import_module(PKG + '.pipeline')
    params = importlib.import_module(PKG + '.parameters').parameters
    syn = importlib.import_module(PKG + '.synthetic')
    L = importlib.import_module(PKG + '.lib')
    eng = pipeline.Engine(params, max_frames=args.frames, max_persons_per_camera=args.persons)
    nf = 2 + eng.V * eng.J * 10
    eng.load_gat(syn.gat_state_dict(7, nf, logit_gain=25.0, logit_shift=0.698 + 0.25), syn.gat_params(nf))
    uniq = max(1, min(args.frames, 250))
    distinct = [syn.make_frame(eng.calib, i, syn.FrameSpec(persons=args.persons))[0] for i in range(uniq)]
    frames = [{c: [f[c][0], f[c][1]] for c in f} for f in distinct]
    db = eng.to_device(eng.pack([frames[i % uniq] for i in range(args.frames)]))
    B, M = db.n_frames, db.n_edge_nodes
    scores = torch.empty(M, dtype=torch.float32, device=eng.device)
    persons = torch.empty((B, eng.pcap, eng.V), dtype=torch.int32, device=eng.device)
    n_persons = torch.empty((B,), dtype=torch.int32, device=eng.device)
    a = eng._geom_args(0.10, 0.5, 1, None, 0.0)
    a.d_scores = scores.data_ptr()
    lib, ctx, st, bs = eng.lib, eng.ctx, eng._stream(), C.byref(db.struct)
    ptr = pipeline._ptr
    fns = {
        'geom_scores': lambda: eng._chk(lib.mpe_geom_scores_batch(ctx, st, bs, C.byref(a))),
        'geom_match': lambda: eng._chk(lib.mpe_geom_match_batch(ctx, st, bs, C.byref(a), ptr(persons), ptr(n_persons))),
        'cluster': lambda: eng._chk(lib.mpe_cluster_batch(ctx, st, bs, ptr(scores), ptr(persons), ptr(n_persons))),
        'gat_match': lambda: eng._chk(lib.mpe_match_batch(ctx, st, bs, ptr(scores), ptr(persons), ptr(n_persons))),
    }
    fns['geom_match']()
    torch.cuda.synchronize()
    geom_persons = int(n_persons.sum())
    for fn in fns.values():                              # warm-up: code objects, the GAT workspace
        timed(fn, args.calls)
    fns['geom_scores']()                                 # (the clustering below is timed on the geometric scores)
    ms = {k: [] for k in fns}
    for _ in range(args.reps):
        for k in ('geom_scores', 'geom_match', 'cluster', 'gat_match'):
            if k == 'cluster':
                fns['geom_scores']()
            ms[k].append(timed(fns[k], args.calls))
    eng.sync_status()
    rec = {'shape': '5x%d' % args.persons, 'frames': B, 'heads': db.n_heads, 'edge_nodes': M, 'reps': args.reps, 'calls_per_rep': args.calls,
           'persons_found_by_geom_match': geom_persons}
    for k in fns:
        rec[k + '_ms_median'] = round(float(np.median(ms[k])), 4)
        rec[k + '_ms_min_max'] = [round(min(ms[k]), 4), round(max(ms[k]), 4)]
    line = json.dumps(rec)
    print(line, flush=True)
    eng.close()
    if args.out:
        with open(args.out, 'w') as fh:
            fh.write(line + '\n')


if __name__ == '__main__':
    main()
