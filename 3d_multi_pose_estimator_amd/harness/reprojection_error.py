"""Counterpart of the reference's test/reprojection_error.py: a ground-truth-free accuracy
check.  Every 3D result (MLP regression and triangulation) is projected back into each camera
that saw the person with the reference's radial-only lens model (`get_projected_coordinates`,
reprojection_error.py:89-107; `apply_distortion`, pose_estimator_utils.py:44-50) and compared
with the detected 2D joints whose confidence exceeds 0.5 (:333-343, 377-390); the mean and the
median pixel error are printed per camera (:422-430).  Matching and both 3D stages run batched
on the device.

Without flags the projection is host-side numpy, joint by joint (`evaluate`).  `--device-metrics` keeps everything on
the device: Engine.reproject (mpe_reproject_batch) writes the residuals of the `est` and the `triang` row of every
batch, the residual tensors of the whole run stay there, and Engine.residual_stats (mpe_residual_stats) gives count,
mean and the exact median per camera at the end -- no pose is copied to the host and there is no per-joint Python; the
lines printed and the dictionary returned are the same.

`--showgt` adds the script's third row, `GT` (:30, 181-233, 331-349, 377-398), and reads the dataset calibration from
--tmdir (tm_<a>_<b>.pickle next to the test file's name; FileNotFoundError when it is missing).  The script is replayed
statement by statement: a selected frame is skipped unless every GT body has '-1' and every joint of joint_list, and
when it has no bodies -- for all three rows; the GT goes from dataset camera 1 to world (common.ground_truth); a
person's GT body is the first one with the smallest mean distance over used_joints to its MLP pose (strict <), and
because the script's `if` sits outside its `for` (:382-390) only the LAST joint of the body's dict is compared per
(person, camera).  The GT bodies go through the same projection as a pose tensor with a one-bit joint mask.  The flag
works with and without --device-metrics; without it the vectorised host statement harness/reprojection.py does the
bookkeeping (`evaluate_arrays`).

The device path and harness/reprojection.py test `valid > 0.5` on the float32 of the packed batch, the joint-by-joint
loop on the binary64 JSON value: a `valid` strictly between 0.5 and 0.5 + 2^-24 would be booked by one and not by the
other.  Detectors write 0 / 1 or probabilities far from that interval.
"""
import json
import types

import numpy as np
import torch

from .. import synthetic
from ..calibration import Calibration
from ..parameters import parameters
from ..pipeline import Engine
from . import reprojection as R
from .common import build_parser, dataset_transform, load_models, match_stage, pack_ground_truth, report_matcher, teacher_scores


def project(calib, cam_idx, p3d):
    """world point (3,) -> pixel (2,), radial distortion k1,k2,k3 only, fp32 like the reference."""
    T = calib.T_d[cam_idx].astype(np.float32)
    pc = (T @ np.append(p3d.astype(np.float32), np.float32(1.0)))[:3]
    h = pc / pc[2]
    r = np.float32(h[0] * h[0] + h[1] * h[1])
    kd = np.asarray(calib.dist[cam_idx], np.float64)[[0, 1, 4]].astype(np.float32)     # the calibration's own, which a fitted one replaces
    f = np.float32(1) + kd[0] * r + kd[1] * r * r + kd[2] * r * r * r
    d = np.array([h[0] * f, h[1] * f, np.float32(1.0)], np.float32)
    px = calib.K32[cam_idx] @ d
    return (px / px[2])[:2]


def collect_work(args, calib):
    work = []
    if args.synthetic:
        spec = synthetic.FrameSpec(persons=args.persons, noise_px=args.noise_px, float_conf=False)
        for i in range(args.synthetic):
            f, gt = synthetic.make_frame(calib, i, spec)
            work.append((f, gt['owner']))
        return work
    n_input = 0
    for file in args.testfiles:
        print(file)
        for frame in json.load(open(file, 'rb')):
            n_input += 1
            if (n_input - 1) % args.datastep == 0:
                work.append((frame, None))
    return work


def collect_work_showgt(args, calib):
    """collect_work under --showgt: [(frame, owners, T_dataset_cam1)] of the selected frames that pass the script's GT
    filter (reprojection_error.py:181-233); raises SystemExit for a file without a GT field, like the script."""
    work = []
    if args.synthetic:
        T = torch.from_numpy(calib.T_d[1]).type(torch.float32)
        items = [(f, o, T) for f, o in collect_work(args, calib)]
    else:
        items, n_input = [], 0
        for file in args.testfiles:
            print(file)
            T = torch.from_numpy(dataset_transform(args.tmdir[0], file).get_transform('root', parameters.camera_names[1])).type(torch.float32)
            for frame in json.load(open(file, 'rb')):
                n_input += 1
                if (n_input - 1) % args.datastep == 0:
                    items.append((frame, None, T))
    for frame, owners, T in items:
        ok = R.showgt_frame_ok(frame, parameters.joint_list)
        if ok is None:
            print('There is no ground truth in the specified file')
            raise SystemExit
        if ok:
            work.append((frame, owners, T))
    return work


KINDS = ('est', 'GT', 'triang')               # the order the script prints its rows in (:426-430)
REFINED = ('est+refine', 'triang+refine')     # --refine: the rows of the refined poses, after the script's own


def report(stats_of_kind):
    """{kind: per-camera stats with 'count', 'mean', 'median'} -> the printed report and the returned dictionary."""
    names = list(parameters.camera_names)
    print('**********************  REPROJECTION ERRORS (mean and median) **********************')
    out = {}
    for c, cam in enumerate(names):
        print('------------------', 'CAMERA', cam, '------------------')
        for kind in KINDS + REFINED:
            st = stats_of_kind.get(kind)
            if st is not None and st['count'][c] > 0:
                print(kind, st['mean'][c], st['median'][c])
                out[(kind, cam)] = (float(st['mean'][c]), float(st['median'][c]), int(st['count'][c]))
    return out


def _processed(frame):
    return {c: [frame[c][0], frame[c][1]] for c in frame if json.loads(frame[c][0])}


def evaluate_arrays(work, infer_arrays, calib, showgt=False, batch=256):
    """The same report from batch arrays, by the vectorised host statement harness/reprojection.py.
    `infer_arrays(frames, owners)` -> {'pb': the packed batch, 'persons' [B,Pcap,V], 'n_persons' [B], 'poses' [B,Pcap,J,3]
    f32, 'valid' [B,Pcap], 'tri' [B,Pcap,J,3] f64, 'jv' [B,Pcap,J]} (numpy).  work: collect_work's items, or
    collect_work_showgt's with showgt."""
    J = len(parameters.joint_list)
    used_mask = sum(1 << j for j in parameters.used_joints)
    T_i1 = torch.from_numpy(calib.T_i32[1])
    res = {'est': [], 'triang': []}
    if showgt:
        res['GT'] = []
    for start in range(0, len(work), batch):
        chunk = work[start:start + batch]
        a = infer_arrays([_processed(w[0]) for w in chunk], [w[1] for w in chunk])
        res['est'].append(R.residuals(calib, a['pb'], a['persons'], a['n_persons'], a['poses'], a['valid'], used_mask))
        res['triang'].append(R.residuals(calib, a['pb'], a['persons'], a['n_persons'], a['tri'], a['jv'], (1 << J) - 1))
        if showgt:
            gt = pack_ground_truth([w[0] for w in chunk], [w[2] for w in chunk], T_i1)
            sel = R.select_gt(a['poses'], a['valid'], a['n_persons'], gt, parameters.used_joints)
            gp, gf = R.gt_pose_tensor(gt, sel)
            res['GT'].append(R.residuals(calib, a['pb'], a['persons'], a['n_persons'], gp, gf, R.gt_joint_mask(parameters.joint_list)))
    empty = np.zeros((0, 1, len(parameters.camera_names), J))
    return report({k: R.stats([x.reshape(-1, *x.shape[-2:]) for x in v] or [empty]) for k, v in res.items()})


def device_gt_poses(eng, poses, valid, n_persons, gt):
    """reprojection.select_gt + gt_pose_tensor on the device: -> (GT poses [B,Pcap,J,3] f32, flags [B,Pcap] u8).
    The script's distances person x GT body (:334-346) are mpe_eval_batch's table, whose detections are the valid
    persons of a frame in order; the table is complete whatever the frame's status says (the status bits concern the
    assignment search only, which is not used here)."""
    dev = eng.device
    B = poses.shape[0]
    ev = eng.evaluate(types.SimpleNamespace(n_frames=B), poses, valid, n_persons, gt, 'mlp', skip=np.zeros(B, np.uint8))
    table = ev['table']                                                             # [B, body, detection]
    # a body beyond the frame's count, or without a used joint (the script skips it, n_joints == 0; the table holds 0
    # there), is never the minimum
    used = np.isin(np.arange(eng.J), list(parameters.used_joints))
    has = (np.asarray(gt['joint'], bool) & used[None, None]).any(axis=2) & (np.arange(gt['joint'].shape[1])[None] < np.asarray(gt['n'])[:, None])
    if has.shape[1] == 0:
        has = np.zeros((B, 1), bool)
    table = table.masked_fill(~torch.from_numpy(has).to(dev)[:, :, None], float('inf'))
    best = torch.argmin(table, dim=1)                                               # per detection the FIRST minimum, like the script's strict <
    least = torch.gather(table, 1, best[:, None, :])[:, 0]
    live = (valid != 0) & (torch.arange(eng.pcap, device=dev)[None, :] < n_persons[:, None])
    det = (torch.cumsum(live.to(torch.int64), 1) - 1).clamp_(min=0)                 # person p is detection det[p] of its frame
    body = torch.gather(best, 1, det)                                               # [B, person]
    ok = live & (torch.gather(least, 1, det) < 10000000000.)
    gx = torch.from_numpy(np.ascontiguousarray(gt['xyz'], np.float32)).to(dev)      # [B,Gcap,J,3] world
    if gx.shape[1] == 0:
        gx = torch.zeros((B, 1, eng.J, 3), dtype=torch.float32, device=dev)
    gp = torch.gather(gx, 1, body[:, :, None, None].expand(-1, -1, gx.shape[2], 3)).contiguous()
    return gp, ok.to(torch.uint8).contiguous()


def evaluate_on_device(work, eng, infer_device, calib, showgt=False, batch=256, refine=0, huber_px=0.0):
    """--device-metrics: `infer_device(frames, owners)` -> (db, persons, n_persons, poses, valid, tri, jv) on the device;
    the residuals of every batch stay there (8 bytes x B x Pcap x V x J each) and the statistics come from one call at
    the end.  refine > 0 (--refine): both pose sets also go through Engine.refine (at most `refine` iterations) and are
    projected again -- two more rows per camera, and the dictionary gains 'squared_sum': per kind the sum over all
    counted entries of the squared residual, the quantity the refinement minimises."""
    T_i1 = torch.from_numpy(calib.T_i32[1])
    res = {'est': [], 'triang': []}
    if showgt:
        res['GT'] = []
    for start in range(0, len(work), batch):
        chunk = work[start:start + batch]
        db, persons, n_persons, poses, valid, tri, jv = infer_device([_processed(w[0]) for w in chunk], [w[1] for w in chunk])
        res['est'].append(eng.reproject(db, persons, n_persons, poses, valid, 'est'))
        res['triang'].append(eng.reproject(db, persons, n_persons, tri, jv, 'triang'))
        if showgt:
            gt = pack_ground_truth([w[0] for w in chunk], [w[2] for w in chunk], T_i1)
            gp, ok = device_gt_poses(eng, poses, valid, n_persons, gt)
            res['GT'].append(eng.reproject(db, persons, n_persons, gp, ok, 'gt'))
        if refine:
            for kind, p, f in (('est', poses, valid), ('triang', tri, jv)):
                better = eng.refine(db, persons, n_persons, p, f, kind, max_iters=refine, huber_px=huber_px)['poses']
                res.setdefault(kind + '+refine', []).append(eng.reproject(db, persons, n_persons, better, f, kind))
        eng.sync_status()
    if not work:
        empty = torch.zeros((0, eng.pcap, eng.V, eng.J), dtype=torch.float64, device=eng.device)
        res = {k: [empty] for k in res}
    out = report({k: eng.residual_stats(v) for k, v in res.items()})
    if refine:
        out['squared_sum'] = {k: float(sum((r.clamp(min=0.0) ** 2).sum() for r in v)) for k, v in res.items()}
    return out


def evaluate(work, infer, calib, batch=256):
    """`infer(frames, owners)` -> per frame a list of persons, each
    ({camera: skeleton dict}, est pose [J,3] or None, {joint idx: (3,)} triangulated).
    Bookkeeping of reprojection_error.py:350-420: per camera that saw the person, every used joint
    of the estimate / every triangulated joint whose detection has valid > 0.5."""
    names = list(parameters.camera_names)
    err = {'est': {c: [] for c in names}, 'triang': {c: [] for c in names}}
    for start in range(0, len(work), batch):
        chunk = work[start:start + batch]
        frames = [{c: [f[c][0], f[c][1]] for c in f if json.loads(f[c][0])} for f, _ in chunk]
        for persons in infer(frames, [o for _, o in chunk]):
            for skels, est, tri in persons or []:
                for cam, coords in skels.items():
                    c = names.index(cam)
                    for j in parameters.joint_list:
                        key = str(j)
                        if key not in coords or not coords[key][3] > 0.5:
                            continue
                        obs = np.array([coords[key][1], coords[key][2]])
                        if est is not None and j in parameters.used_joints:
                            err['est'][cam].append(float(np.linalg.norm(project(calib, c, est[j]) - obs)))
                        if j in tri:
                            err['triang'][cam].append(float(np.linalg.norm(project(calib, c, tri[j]) - obs)))
    print('**********************  REPROJECTION ERRORS (mean and median) **********************')
    out = {}
    for cam in names:
        print('------------------', 'CAMERA', cam, '------------------')
        for kind in ('est', 'triang'):
            if err[kind][cam]:
                a = np.array(err[kind][cam])
                print(kind, a.mean(), np.median(a))
                out[(kind, cam)] = (float(a.mean()), float(np.median(a)), len(a))
    return out


def run(args):
    from .common import max_skeletons_per_camera
    calib = Calibration(parameters)
    showgt = bool(getattr(args, 'showgt', False))
    work = collect_work_showgt(args, calib) if showgt else collect_work(args, calib)
    eng = Engine(parameters, calib, max_frames=args.batch,
                 max_persons_per_camera=max(4, args.persons + 1, max_skeletons_per_camera([(w[0], None, None) for w in work])))
    load_models(eng, args, need_mlp=True)
    names = list(parameters.camera_names)

    def infer(frames, owners):
        db = eng.to_device(eng.pack(frames, keep_json=True))
        if args.teacher_scores and owners[0] is not None:
            persons, n_persons = eng.cluster(db, teacher_scores(db, owners))
        else:
            persons, n_persons = match_stage(eng, args, db)
        poses, valid = eng.mlp3d(db, persons, n_persons)
        # the script's own gather keeps joints whose id is > 0 (reprojection_error.py:296-300)
        tri, jv = eng.triangulate(db, persons, n_persons, all_joints=True, positive_ids_only=True)
        eng.sync_status()
        persons, n_persons = persons.cpu().numpy(), n_persons.cpu().numpy()
        poses, valid, tri, jv = poses.cpu().numpy(), valid.cpu().numpy(), tri.cpu().numpy(), jv.cpu().numpy()
        out = []
        for f in range(len(frames)):
            heads = db.host.jsons_for_head[f]
            people = []
            for p in range(int(n_persons[f])):
                skels = {cam: heads[int(persons[f, p, c])] for c, cam in enumerate(names) if persons[f, p, c] >= 0}
                people.append((skels, poses[f, p] if valid[f, p] else None,
                               {j: tri[f, p, j].astype(np.float32) for j in parameters.joint_list if jv[f, p, j]}))
            out.append(people)
        return out

    def infer_device(frames, owners):
        db = eng.to_device(eng.pack(frames))
        if args.teacher_scores and owners[0] is not None:
            persons, n_persons = eng.cluster(db, teacher_scores(db, owners))
        else:
            persons, n_persons = match_stage(eng, args, db)
        poses, valid = eng.mlp3d(db, persons, n_persons)
        tri, jv = eng.triangulate(db, persons, n_persons, all_joints=True, positive_ids_only=True)
        return db, persons, n_persons, poses, valid, tri, jv

    def infer_arrays(frames, owners):
        db, *dev = infer_device(frames, owners)
        eng.sync_status()
        keys = ('persons', 'n_persons', 'poses', 'valid', 'tri', 'jv')
        return dict({k: v.cpu().numpy() for k, v in zip(keys, dev)}, pb=db.host)

    if getattr(args, 'device_metrics', False) or getattr(args, 'refine', 0):
        out = evaluate_on_device(work, eng, infer_device, calib, showgt, args.batch, int(getattr(args, 'refine', 0) or 0),
                                 float(getattr(args, 'refine_huber', 0.0)))
    elif showgt:
        out = evaluate_arrays(work, infer_arrays, calib, True, args.batch)
    else:
        out = evaluate(work, infer, calib, args.batch)
    opts = report_matcher(args)
    if opts is not None:
        out['matcher'] = dict(opts, name='geometric')
    eng.close()
    return out


def build_own_parser():
    p = build_parser('Print the reprojection error of the pose estimation model and of the triangulation')
    p.add_argument('--showgt', action='store_true', help='Show ground truth reprojection error (reads the dataset calibration from --tmdir)')
    return p


def main(argv=None):
    return run(build_own_parser().parse_args(argv))


if __name__ == '__main__':
    main()
