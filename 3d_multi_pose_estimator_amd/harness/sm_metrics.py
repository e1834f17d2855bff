"""Counterpart of the reference's test/sm_metrics.py on the MI355X path: clustering quality of
the skeleton-matching stage (adjusted Rand index, homogeneity, completeness, V-measure) against
a ground-truth grouping built from the per-skeleton 3D bodies.

Kept from the reference (sm_metrics.py:107-229): frame stride; GT persons built by greedy 3D
proximity over the cameras' bodies_3D lists (a skeleton joins the nearest GT person when the
mean joint distance is <= 1 unit, else founds a new one, :128-160); frames with a body lacking
the '-1' key or without any GT are skipped (:131-132, :166-167); one label per head node:
index of the proposal containing it, or len(proposals) for unassigned heads (:208-216);
metrics averaged over frames (:218-229).  Matching itself runs batched on the device.

With --device-gt (which implies --device-metrics) the bodies are parsed on the GPU from the file's bytes
(Engine.bodies_from_json) and handed to Engine.group_bodies as they are, in place of partition.pack_bodies.
With --device-metrics the scoring runs there too: the bodies of a batch are packed (partition.pack_bodies) and grouped by
Engine.group_bodies, the proposals become labels in Engine.partition_labels, Engine.partition_scores scores the two, and
one [B,4] array comes back per batch; the totals are added here in frame order.  harness/partition.py states the
arithmetic (sklearn's, with every sum in a written order); without the flag the loop below and sklearn do the work.
"""
import copy
import json

import numpy as np
import torch
from sklearn.metrics import adjusted_rand_score, homogeneity_completeness_v_measure

from .. import synthetic
from ..calibration import Calibration
from ..parameters import parameters
from ..pipeline import Engine
from . import partition as P
from .common import build_parser, load_models, match_stage, report_matcher, teacher_scores


def gt_labels(frame):
    """-> list of GT person ids, one per skeleton in (camera, list) order, or None to skip."""
    gt_people, labels, valid = [], [], True
    for cam in frame:
        if cam not in parameters.used_cameras:
            continue
        for id_skeleton, joints_3D in enumerate(frame[cam][3]):
            if '-1' not in joints_3D:
                valid = False
            best, matched, n_joints = 1000000000., -1, 0
            for pid, person in enumerate(gt_people):
                dist, n = 0.0, 0
                for idx, p3D in person.items():
                    if idx in joints_3D:
                        dist += np.linalg.norm(np.array(joints_3D[idx]) - np.array(p3D))
                        n += 1
                if dist < best:
                    best, matched, n_joints = dist, pid, n
            if n_joints == 0 or best / n_joints > 1.:
                matched = -1
            if matched < 0:
                matched = len(gt_people)
                gt_people.append(copy.deepcopy(joints_3D))
            labels.append(matched)
    if not gt_people or not valid:
        return None
    return labels


def collect_work(args, calib, src=None):
    work = []
    if args.synthetic:
        spec = synthetic.FrameSpec(persons=args.persons, noise_px=args.noise_px)
        for i in range(args.synthetic):
            f, gt = synthetic.make_frame(calib, i, spec)
            work.append((f, gt['owner']))
        return work
    n_input = 0
    for file in args.testfiles:
        print(file)
        for k, frame in enumerate(json.load(open(file, 'rb'))):
            n_input += 1
            if (n_input - 1) % args.datastep == 0:
                if len(frame[list(frame.keys())[0]]) != 4:
                    print('There is no ground truth in the specified file')
                    raise SystemExit
                work.append((frame, None))
                if src is not None:
                    src.append((args.testfiles.index(file), k))
    return work


def evaluate(work, infer, batch=256):
    """`infer(frames, owners)` -> per frame None (no graph, reference :186-187) or
    (H, proposals) with proposals = list of lists of head ids.  Returns the four averages."""
    tot = {'rand score': 0.0, 'homogeneity': 0.0, 'completeness': 0.0, 'v_measure': 0.0}
    n_data = 0
    for start in range(0, len(work), batch):
        chunk = [(f, o, gt_labels(f)) for f, o in work[start:start + batch]]
        chunk = [c for c in chunk if c[2] is not None]
        if not chunk:
            continue
        frames = [{c: [f[c][0], f[c][1]] for c in f if json.loads(f[c][0])} for f, _, _ in chunk]
        results = infer(frames, [o for _, o, _ in chunk])
        for (_, _, labels), res in zip(chunk, results):
            if res is None:
                continue
            H, proposals = res
            if len(labels) != H:
                continue          # skeletons without joints: GT list and head list no longer align
            n_data += 1
            est = []
            for h in range(H):
                idx = len(proposals)
                for p, members in enumerate(proposals):
                    if h in members:
                        idx = p
                        break
                est.append(idx)
            tot['rand score'] += adjusted_rand_score(labels, est)
            hom, com, v = homogeneity_completeness_v_measure(labels, est)
            tot['homogeneity'] += hom
            tot['completeness'] += com
            tot['v_measure'] += v
    out = {k: v / max(1, n_data) for k, v in tot.items()}
    for k in ('rand score', 'homogeneity', 'completeness', 'v_measure'):
        print(k, out[k])
    out['n_data'] = n_data
    return out


KEYS = ('rand score', 'homogeneity', 'completeness', 'v_measure')


def device_bodies(device_gt, start, n):
    """The bodies of a batch parsed on the device (--device-gt) -> (packed: Engine.group_bodies' arrays as device tensors, S
    [n] bodies per frame, valid [n]), or None when a window of the batch has to be redone on the host."""
    parts = []
    for i, j, file_no, first in device_gt.runs(start, n):
        pb = device_gt.bodies(file_no, first, j - i)
        if pb is None:
            return None
        parts.append(pb.packed())
    packed = {k: (torch.cat([p[k] for p in parts], 0) if len(parts) > 1 else parts[0][k]) for k in parts[0]}
    S, m1 = packed['n'].cpu().numpy(), packed['m1'].cpu().numpy()
    valid = np.array([S[i] > 0 and bool(m1[i, :S[i]].all()) for i in range(n)])
    return packed, S, valid


def evaluate_on_device(work, infer, batch=256, device_gt=None):
    """evaluate() with --device-metrics.  `infer(frames, owners, packed)` -> (scores [B,4] float64 of the batch as
    Engine.partition_scores left them, H [B], M [B], finish) with finish(f) -> the frame's (proposals as rows, their
    number).  The skip rules are evaluate()'s and are known here from the counts: no GT person or a body without '-1'
    (gt_labels gives None), no graph (M == 0), len(labels) != H.  A frame that counts but came back as NaN (over a compiled
    cap of the kernels, or a batch whose bodies cannot be packed) is finished by the numpy statement.  With device_gt
    (common.DeviceGT, --device-gt) the bodies come from device_bodies() instead of pack_bodies and stay on the device."""
    tot = np.zeros(4, np.float64)
    n_data = 0
    for start in range(0, len(work), batch):
        chunk = work[start:start + batch]
        parsed = device_bodies(device_gt, start, len(chunk)) if device_gt is not None else None
        if parsed is not None:
            packed, S, valid = parsed
        else:
            try:
                packed = P.pack_bodies([f for f, _ in chunk])
                S = packed['n']
                valid = np.array([S[i] > 0 and bool(packed['m1'][i, :S[i]].all()) for i in range(len(chunk))])
            except ValueError:           # more joint keys than presence bits, or a value that is not a point: the host groups this batch
                packed = None
                gts = [gt_labels(f) for f, _ in chunk]
                S = np.array([len(g) if g is not None else 0 for g in gts], np.int32)
                valid = np.array([g is not None for g in gts])
        if not valid.any():
            continue
        # as in evaluate(): only the frames gt_labels() accepts are packed and matched
        sel = np.flatnonzero(valid)
        chunk, S = [chunk[i] for i in sel], S[sel]
        if packed is not None:
            pick = torch.from_numpy(sel)
            packed = {k: (v[sel] if isinstance(v, np.ndarray) else v.index_select(0, pick.to(v.device)) if isinstance(v, torch.Tensor) else v)
                      for k, v in packed.items()}
        frames = [{c: [f[c][0], f[c][1]] for c in f if json.loads(f[c][0])} for f, _ in chunk]
        scores, H, M, finish = infer(frames, [o for _, o in chunk], packed)
        counted = (M != 0) & (S == H)
        for i in np.flatnonzero(counted):
            row = scores[i] if scores is not None else None
            if row is None or np.isnan(row).any():
                rows, n = finish(i)
                row = P.partition_scores(gt_labels(chunk[i][0]), P.proposal_labels(rows, n, int(H[i])))
            n_data += 1
            tot += row                   # frame order, float64: the host loop's sums
    out = {k: float(tot[j]) / max(1, n_data) for j, k in enumerate(KEYS)}
    for k in KEYS:
        print(k, out[k])
    out['n_data'] = n_data
    return out


def run(args):
    from .common import max_skeletons_per_camera
    calib = Calibration(parameters)
    device_gt = getattr(args, 'device_gt', False) and not args.synthetic
    if getattr(args, 'device_gt', False):
        args.device_metrics = True
    src = [] if device_gt else None
    work = collect_work(args, calib, src)
    eng = Engine(parameters, calib, max_frames=args.batch,
                 max_persons_per_camera=max(4, args.persons + 1, max_skeletons_per_camera([(f, None, None) for f, _ in work])))
    load_models(eng, args, need_mlp=False)

    def infer(frames, owners):
        db = eng.to_device(eng.pack(frames))
        if args.teacher_scores and owners[0] is not None:
            persons, n_persons = eng.cluster(db, teacher_scores(db, owners))
        else:
            persons, n_persons = match_stage(eng, args, db)
        eng.sync_status()
        persons, n_persons = persons.cpu().numpy(), n_persons.cpu().numpy()
        out = []
        for f in range(len(frames)):
            h0, H, e0, M = db.host.frame_counts(f)
            if M == 0:
                out.append(None)
            else:
                out.append((H, [[int(h) for h in persons[f, p] if h >= 0] for p in range(int(n_persons[f]))]))
        return out

    def infer_device(frames, owners, packed):
        db = eng.to_device(eng.pack(frames))
        if args.teacher_scores and owners[0] is not None:
            persons, n_persons = eng.cluster(db, teacher_scores(db, owners))
        else:
            persons, n_persons = match_stage(eng, args, db)
        B = len(frames)
        H = np.diff(np.asarray(db.host.frame_head_off[:B + 1]))
        M = np.diff(np.asarray(db.host.frame_en_off[:B + 1]))
        scores = None
        if packed is not None:
            gt = eng.group_bodies(packed, skip_in=(M == 0))
            est = eng.partition_labels(db, persons, n_persons)
            scores, _ = eng.partition_scores(gt['labels'], est['labels'], est['count'], skip=gt['skip'], count_true=gt['count'])
        eng.sync_status()
        return (scores.cpu().numpy() if scores is not None else None), H, M, lambda f: (persons[f].cpu().numpy(), int(n_persons[f]))

    if getattr(args, 'device_metrics', False):
        from .common import DeviceGT
        dgt = DeviceGT(eng, args.testfiles, src, args.datastep) if device_gt else None
        out = evaluate_on_device(work, infer_device, args.batch, dgt)
        if dgt is not None:
            print('Ground truth on the device: %d windows, %d redone on the host' % (dgt.windows, dgt.declined))
            out['gt_windows'], out['gt_declined'] = dgt.windows, dgt.declined
            dgt.close()
    else:
        out = evaluate(work, infer, args.batch)
    opts = report_matcher(args)
    if opts is not None:
        out['matcher'] = dict(opts, name='geometric')
    eng.close()
    return out


def main(argv=None):
    return run(build_parser('Print clustering metrics of the skeleton-matching model (CMU Panoptic only)').parse_args(argv))


if __name__ == '__main__':
    main()
