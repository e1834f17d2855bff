"""Evaluation harness shared by metrics_from_model.py / metrics_from_triangulation.py: the
counterpart of the reference's two callers (test/metrics_from_model.py,
test/metrics_from_triangulation.py), restated on top of the batched engine.

Kept from the reference: CLI flags (--testfiles --tmdir --modelsdir --datastep, :27-35), the
frame stride (:124), the skip rules (no GT field -> exit :129-131; no GT bodies -> skip
:137-138; no cross-camera pair -> skip :195-196), ground truth brought to world coordinates
through camera 1 of the dataset calibration (:152-161), per-person error = mean joint distance
over used_joints (:303-320), assignment by exhaustive permutation search (:322-337), MPJPE /
AP / recall bookkeeping at 25..150 mm (:339-385) and the printed quantities (:382-390), plus
frames/s.  Frames are processed in batches instead of one by one.
"""
import argparse
import itertools
import json
import os
import pickle
import sys
import time

import numpy as np
import torch

from .. import synthetic
from ..calibration import Calibration, load_intrinsics, load_transform_manager
from ..lib import MPE_EVAL_NO_ASSIGNMENT, MPE_EVAL_OVER_BUDGET, MPE_EVAL_OVER_CAP, MPE_EVAL_SKIPPED
from ..parameters import parameters
from ..pipeline import Engine
from .assignment import assign_bnb, frame_records

THRESHOLDS_MM = np.arange(25, 155, 25)
TRACK_SCORE_GCAP = 32          # --track-score: ground-truth rows per frame of the GT tracker and the scorer


def build_parser(description):
    p = argparse.ArgumentParser(description=description)
    p.add_argument('--testfiles', type=str, nargs='+', required=False, default=[], help='List of json files used as input')
    p.add_argument('--tmdir', type=str, nargs=1, required=False, default=['.'],
                   help='Directory that contains the files with the transfomation matrices')
    p.add_argument('--modelsdir', type=str, nargs='?', required=False, default='../models/',
                   help="Directory that contains the models' files")
    p.add_argument('--datastep', type=int, nargs='?', required=False, default=12, help='Data step used to compute the metrics')
    p.add_argument('--batch', type=int, default=256, help='frames per device batch')
    p.add_argument('--cameras', type=str, default=None, metavar='cams.json',
                   help='start from this camera file (harness.camfit --out, or a tm_*.json): its transforms, and its "intrinsics" list when it has '
                        'one, in the place of the packaged calibration')
    p.add_argument('--synthetic', type=int, default=0, help='generate this many synthetic Panoptic-shaped frames instead of --testfiles')
    p.add_argument('--random-weights', action='store_true', help='deterministic hash-initialised weights (no checkpoint offline)')
    p.add_argument('--teacher-scores', action='store_true',
                   help='synthetic frames only: replace the GAT scores by the ground-truth pairing (isolates the 3D stage)')
    p.add_argument('--matcher', choices=['gat', 'geometric'], default='gat',
                   help='geometric: the matching scores come from the calibration alone (mpe_geom_match_batch: distance between the back-projected '
                        'rays of two skeletons); no skeleton-matching model is loaded and one further line reports the matcher.  '
                        '--teacher-scores keeps precedence')
    p.add_argument('--geom-sigma', type=float, default=0.10, metavar='M', help='--matcher geometric: mean ray distance that scores 0.5, metres')
    p.add_argument('--geom-clip', type=float, default=0.5, metavar='M', help='--matcher geometric: largest distance a joint contributes, metres (0: no clip)')
    p.add_argument('--geom-min-joints', type=int, default=1, metavar='N', help='--matcher geometric: common joints a pair needs to score at all')
    p.add_argument('--geom-min-conf', type=float, default=0.0, metavar='C', help='--matcher geometric: detection confidence a joint needs in both views')
    p.add_argument('--noise-px', type=float, default=0.0)
    p.add_argument('--persons', type=int, default=4)
    p.add_argument('--gat-acc64', action='store_true',
                   help='f64 running sums in every GEMM of the matching network (Engine.set_precision(gat_acc64=True); default: single fp32 chains for K <= 512)')
    p.add_argument('--mlp-precision', choices=['default', 'max_accuracy', 'f64'], default='default',
                   help='MLP mode 3 (default: f64 sums every second K stage), 4 (an f64 flush per stage) or 5 (the network evaluated on the f64 matrix pipe)')
    p.add_argument('--device-metrics', action='store_true',
                   help='scoring on the GPU: error tables and pose-to-GT assignment (mpe_eval_batch) in the two metrics_from_* scripts, residuals and '
                        'medians in reprojection_error, GT grouping, labels and the four clustering scores (mpe_group_bodies, mpe_partition_labels, '
                        'mpe_partition_scores) in sm_metrics and sm_metrics_without_gt: the same report, the results stay on the device')
    p.add_argument('--device-gt', action='store_true',
                   help='implies --device-metrics; the ground truth is built on the GPU as well: the bodies_3D lists of the test files are '
                        'parsed there from the files\' bytes (mpe_json_parse_bodies_device) and turned into the arrays the scoring kernels read '
                        '(mpe_gt_from_bodies in the metrics_from_* scripts, mpe_group_bodies in sm_metrics); a window the device declines is '
                        'redone on the host')
    p.add_argument('--track', action='store_true',
                   help='implies --device-metrics; the poses of the evaluated frames go through one tracker in order (mpe_track_batch: person '
                        'identities over the frames, the state carried across --batch chunks) and one further line reports the tracks.  All '
                        '--testfiles together are one sequence, in the order given: pass one recording per run')
    p.add_argument('--track-gate', type=float, default=0.5, metavar='M', help='--track: largest mean joint distance of a link, metres')
    p.add_argument('--track-gap', type=int, default=2, metavar='N', help='--track: frames a person may go undetected and keep the identity')
    p.add_argument('--track-score', action='store_true',
                   help='implies --track; the track ids are scored against ground-truth identities (mpe_track_score_batch: MOTA, MOTP, '
                        'IDF1, ID switches, fragmentations, MT/PT/ML), the identities being those a second tracker with the same gate '
                        'and gap gives the ground-truth bodies, and one further line reports the score')
    p.add_argument('--track-score-mm', type=float, default=150., metavar='MM',
                   help='--track-score: a detection matches its ground-truth body below this error (default: the largest AP threshold)')
    p.add_argument('--smooth', type=int, default=0, metavar='W',
                   help='implies --track; the tracked poses are fitted with a line per track and joint over the current frame and the W frames '
                        'before it, 1..15 (mpe_smooth_batch, the state carried across --batch chunks), the fitted poses are scored, and one '
                        'further line reports the joints fitted, the joints filled and the mean displacement')
    p.add_argument('--smooth-decay', type=float, default=0.8, metavar='L', help='--smooth: weight ratio of consecutive frames, within [0.25, 1]')
    p.add_argument('--smooth-fill', action='store_true',
                   help='--smooth: a triangulated joint that is missing now but was seen twice or more in the window gets the value of the line')
    p.add_argument('--bones', type=int, default=0, metavar='ITERS',
                   help='implies --track; the bone lengths of every track are learned from its own poses and the poses are moved towards them '
                        'with ITERS sweeps, 1..64 (mpe_skel_*: after refine, track and smooth, before scoring; per evaluated --batch chunk '
                        'observe, update, fit, so a chunk is fitted with the lengths of the recording up to and including that chunk), the '
                        'fitted poses are scored, and one further line reports the tracks with a length, the rows and bones fitted, the '
                        'bone-length error before and after and the mean displacement.  Like --track and --smooth it acts in metrics_from_model '
                        'and metrics_from_triangulation; the other harnesses accept and ignore it')
    p.add_argument('--bones-refine', type=int, default=0, metavar='SWEEPS',
                   help='as --bones up to the length table, then the body-level fit in the place of the position-based one: every tracked pose '
                        'is fitted to the pixels and to the bone lengths of its track together with SWEEPS sweeps, 1..64 (mpe_body_refine_batch, on '
                        'the evaluated frames and their person proposals); the fitted poses are scored, and one further line reports the tracks, '
                        'rows and bones fitted, the free joints, the one-view joints moved, the mean pixel cost and bone-length error before and '
                        'after and the mean displacement.  Not together with --bones.')
    p.add_argument('--bones-weight', type=float, default=300.0, metavar='PX_PER_M',
                   help='--bones-refine: pixels of reprojection error a metre of bone-length error is worth')
    p.add_argument('--bones-huber', type=float, default=0.0, metavar='PX', help='--bones-refine: Huber threshold of the pixel term, 0: plain least squares')
    p.add_argument('--bones-min', type=int, default=10, metavar='N', help='--bones: lengths a track needs of a bone before the bone is held to one')
    p.add_argument('--relink', type=float, default=0.0, metavar='GATE_MM',
                   help='implies --track; right after the tracker a re-identifier gives a track that is born the id of a track lost '
                        'track-gap + 2 .. --relink-max-gap frames ago when their bone lengths agree within GATE_MM millimetres on average '
                        '(mpe_relink_batch: causal, the state carried across --batch chunks); its ids, not the tracker\'s, go to --smooth, '
                        '--bones, --bones-refine, --track-score and the Tracks line, and one further line reports the births, the links, the '
                        'tracks before and after and the mean and largest link gap.  The gate and the other --relink values are options, not '
                        'findings.')
    p.add_argument('--relink-max-gap', type=int, default=150, metavar='N', help='--relink: most frames since the lost track was last seen')
    p.add_argument('--relink-reach', type=float, default=0.0, metavar='M',
                   help='--relink: a returning person is at most M metres (mean joint distance) from where the lost track was last seen; 0: anywhere')
    p.add_argument('--relink-speed', type=float, default=0.0, metavar='M_PER_FRAME', help='--relink-reach grows by this per frame of gap')
    p.add_argument('--relink-min-bones', type=int, default=8, metavar='N', help='--relink: fewest bones a birth and a lost track must have in common')
    p.add_argument('--bones-bin', type=float, default=2.0, metavar='MM', help='--bones: bin width of the length histograms, millimetres')
    p.add_argument('--refine', type=int, default=0, metavar='ITERS',
                   help='implies --device-metrics; every joint is moved to the minimum of its reprojection error over the cameras that saw it '
                        '(mpe_refine_batch: at most ITERS Levenberg-Marquardt iterations per joint, 1..64) and the refined poses are scored; '
                        'one further line reports the solved joints, the share that moved and the mean cost before and after')
    p.add_argument('--refine-huber', type=float, default=0.0, metavar='PX', help='--refine: Huber threshold in pixels (0: plain least squares)')
    p.add_argument('--uncertainty', type=float, default=0.0, metavar='PX',
                   help='implies --device-metrics; every joint gets its 3 x 3 covariance from the cameras that saw it, for detections with '
                        'PX pixels of noise in x and in y (mpe_posecov_batch: PX^2 times the inverse of the normal matrix of --refine, the '
                        'Gauss-Newton approximation), right after --refine (or the time-aware refinement of --lags; on the unrefined poses '
                        'without either) and before tracking; one further line reports the joints computed and the median, 95th percentile '
                        'and maximum sigma in millimetres, and with --refine and --refine-huber 0 the pooled pixel sigma of the recording, '
                        'which says whether PX was a fair choice.  It is the covariance of the per-frame estimate: untimed (lags are '
                        'ignored, as in the DLT), and it says nothing about what --smooth and --bones do afterwards.  It acts in '
                        'metrics_from_model and metrics_from_triangulation; the other harnesses accept and ignore it')
    p.add_argument('--uncertainty-gate', type=float, default=0.0, metavar='MM',
                   help='--uncertainty, metrics_from_triangulation only (the flags of metrics_from_model are per person): a joint whose sigma is '
                        'above MM millimetres loses its flag and is then neither tracked, scored nor written; the line reports how many')
    p.add_argument('--regroup', type=float, default=0.0, metavar='PX',
                   help='after the 3D stage the person proposals are repaired by reprojection consistency (mpe_regroup_batch: a skeleton whose mean '
                        'distance from its row\'s projected pose is PX pixels or more is released, free skeletons within PX are attached to rows '
                        'that lack their camera) and the 3D stage runs again on the new rows, before --refine; one further line reports the '
                        'skeletons released, attached and left free and the rows below the minimum number of views.  It acts in '
                        'metrics_from_model, metrics_from_triangulation and calibrate; the other harnesses accept and ignore it')
    p.add_argument('--regroup-rounds', type=int, default=1, metavar='N', help='--regroup: alternations of regrouping and the 3D stage')
    p.add_argument('--regroup-min-joints', type=int, default=3, metavar='N', help='--regroup: joints a (skeleton, person) pair needs to be judged at all')
    p.add_argument('--regroup-clip', type=float, default=0.0, metavar='PX', help='--regroup: largest distance a joint contributes, pixels (0: no clip)')
    p.add_argument('--merge', type=float, default=0.0, metavar='M',
                   help='after the 3D stage (and after --regroup) two person proposals whose poses lie within M metres of each other and that '
                        'share no camera are merged into one (mpe_consolidate_batch), and the 3D stage runs again on the new rows; 0: off.  '
                        'One further line reports the rows merged and founded and the skeletons left free.  It acts in metrics_from_model, '
                        'metrics_from_triangulation and calibrate; the other harnesses accept and ignore it')
    p.add_argument('--found', type=float, default=0.0, metavar='M',
                   help='the skeletons that belong to no person proposal found new ones where their back-projected rays pass within M metres '
                        'of each other (mpe_consolidate_batch, after --merge); 0: off')
    p.add_argument('--found-min-views', type=int, default=0, metavar='N',
                   help='--found: skeletons a founded person needs (0: the larger of 2 and the minimum number of views)')
    return p


def repair_stage(eng, args, db, persons, n_persons, poses, flags, mode, log, clog, stage3d, joint_mask=None):
    """--regroup / --merge / --found: N times {regroup (--regroup), consolidate (--merge, --found), the 3D stage again on the new
    rows and the new row counts} -> (persons, n_persons, poses, flags); without the flags, the arguments.  mode 'mlp' or
    'triang'; stage3d(persons, n_persons) -> (poses, flags); log takes one list per round of the batch's regroup counts and
    status (host arrays), clog the same of consolidate.  joint_mask: the joints whose poses stage3d fills in (None: those of
    the kind -- a triangulation without all_joints flags the joints outside used_joints as emitted and leaves them at the
    origin, so its caller names the used joints here)."""
    gate = float(getattr(args, 'regroup', 0.0) or 0.0)
    merge_m, found_m = float(getattr(args, 'merge', 0.0) or 0.0), float(getattr(args, 'found', 0.0) or 0.0)
    if not gate and not merge_m and not found_m:
        return persons, n_persons, poses, flags
    kind = 'est' if mode == 'mlp' else 'triang'
    for rnd in range(max(1, int(args.regroup_rounds))):
        if gate:
            rg = eng.regroup(db, persons, n_persons, poses, flags, kind, gate_px=gate, clip_px=args.regroup_clip,
                             min_joints=args.regroup_min_joints, joint_mask=joint_mask)
            persons = rg['persons']
            while len(log) <= rnd:
                log.append([])
            log[rnd].append({k: rg[k].cpu().numpy() for k in ('counts', 'status')})
        if merge_m or found_m:
            cs = eng.consolidate(db, persons, n_persons, poses, flags, kind, merge_m=merge_m or 0.10, found_m=found_m or 0.05,
                                 min_joints=args.regroup_min_joints, found_min_views=int(getattr(args, 'found_min_views', 0) or 0) or None,
                                 joint_mask=joint_mask, merge=bool(merge_m), found=bool(found_m))
            persons, n_persons = cs['persons'], cs['n_persons']
            while len(clog) <= rnd:
                clog.append([])
            clog[rnd].append({k: cs[k].cpu().numpy() for k in ('counts', 'status')})
        poses, flags = stage3d(persons, n_persons)
    return persons, n_persons, poses, flags


def report_regroup(args, log):
    """The further report line of --regroup -> its dict: released and attached over all rounds, free and below the minimum
    number of views after the last."""
    from .regroup import summary
    every, last = summary([o for rnd in log for o in rnd]), summary(log[-1] if log else [])
    r = {'released': every['released'], 'attached': every['attached'], 'free': last['free'], 'below_min_views': last['below_min_views'],
         'copied': last['copied']}
    print('Regrouped (gate %g px, %d round%s): %d skeletons released, %d attached, %d left free, %d rows below the minimum number of views'
          % (args.regroup, len(log), '' if len(log) == 1 else 's', r['released'], r['attached'], r['free'], r['below_min_views']))
    return r


def report_consolidate(args, clog):
    """The further report line of --merge / --found -> its dict: rows merged and founded and skeletons placed over all rounds,
    skeletons left free after the last."""
    from .consolidate import summary
    every, last = summary([o for rnd in clog for o in rnd]), summary(clog[-1] if clog else [])
    r = {'merged': every['merged'], 'founded': every['founded'], 'placed': every['placed'], 'free': last['free'], 'copied': last['copied']}
    print('Consolidated (merge %g m, found %g m): %d rows merged, %d founded from %d skeletons, %d left free'
          % (args.merge, args.found, r['merged'], r['founded'], r['placed'], r['free']))
    return r


def geom_options(args):
    """The options of Engine.geom_match under --matcher geometric, else None."""
    if getattr(args, 'matcher', 'gat') != 'geometric':
        return None
    return dict(sigma=args.geom_sigma, clip=args.geom_clip, min_joints=args.geom_min_joints, min_conf=args.geom_min_conf)


def match_stage(eng, args, db):
    """The matching stage of the scripts -> (persons, n_persons): the GAT, or the ray distances under --matcher geometric."""
    opts = geom_options(args)
    if opts is not None:
        return eng.geom_match(db, want_scores=False, **opts)[1:]
    return eng.match(db, want_scores=False)[1:]


def report_matcher(args):
    """The further report line of --matcher geometric."""
    opts = geom_options(args)
    if opts is not None:
        from .geometric import report_line
        print(report_line(opts))
    return opts


def load_models(eng, args, need_mlp):
    """skeleton_matching.prms/.tch and pose_estimator.pytorch (metrics_from_model.py:89-100),
    or deterministic weights when none are available.  --matcher geometric loads no skeleton-matching model."""
    V, J = eng.V, eng.J
    nf = 2 + V * J * 10
    mdir = args.modelsdir if args.modelsdir.endswith('/') else args.modelsdir + '/'
    if geom_options(args) is not None:
        if need_mlp:
            if args.random_weights or not os.path.exists(mdir + 'pose_estimator.pytorch'):
                if not args.random_weights:
                    print('no pose_estimator.pytorch under %s: using deterministic random weights' % mdir)
                eng.load_mlp(synthetic.mlp_state_dict(11, V * J * parameters.numbers_per_joint))
            else:
                eng.load_mlp(torch.load(mdir + 'pose_estimator.pytorch', map_location='cpu')['model_state_dict'])
        return
    if args.random_weights or not os.path.exists(mdir + 'skeleton_matching.tch'):
        if not args.random_weights:
            print('no model files under %s: using deterministic random weights' % mdir)
        eng.load_gat(synthetic.gat_state_dict(7, nf, logit_gain=25.0, logit_shift=0.698), synthetic.gat_params(nf))
        if need_mlp:
            eng.load_mlp(synthetic.mlp_state_dict(11, V * J * parameters.numbers_per_joint))
        return
    params = pickle.load(open(mdir + 'skeleton_matching.prms', 'rb'))
    eng.load_gat(torch.load(mdir + 'skeleton_matching.tch', map_location='cpu'), params)
    if need_mlp:
        saved = torch.load(mdir + 'pose_estimator.pytorch', map_location='cpu')
        eng.load_mlp(saved['model_state_dict'])


def start_calibration(args):
    """The calibration a script starts from: the packaged one, or with --cameras the transforms of that file and, when
    the file has an "intrinsics" list (harness.camfit --out), its fx, fy, cx, cy and lens terms."""
    path = getattr(args, 'cameras', None)
    if not path:
        return Calibration(parameters)
    return Calibration(parameters, load_transform_manager(path), load_intrinsics(path, parameters))


def dataset_transform(tm_dir, file_name):
    """tm_<a>_<b>.pickle next to the test file's name (metrics_from_model.py:109-115)."""
    base = os.path.basename(file_name).split('_')
    stem = os.path.join(tm_dir, 'tm_' + base[0] + '_' + base[1])
    for ext in ('.pickle', '.json'):
        if os.path.exists(stem + ext):
            return load_transform_manager(stem + ext)
    raise FileNotFoundError(stem + '.pickle')


def ground_truth(frame, T_dataset_cam1, T_i_cam1):
    """-> (list of {joint idx: (3,) f32 world}, valid flags) or None to skip; raises SystemExit
    when the file has no GT field (reference :126-174)."""
    first_cam = list(frame.keys())[0]
    if len(frame[first_cam]) != 4:
        print('There is no ground truth in the specified file')
        raise SystemExit
    for c in frame:
        if len(frame[c][3]) > len(frame[first_cam][3]):
            first_cam = c
    bodies = frame[first_cam][3]
    if len(bodies) == 0:
        return None
    J = len(parameters.joint_list)
    gts, valid = [], []
    for body in bodies:
        g = torch.zeros(J * 3)
        for j in parameters.joint_list:
            if str(j) in body:
                g[j * 3: j * 3 + 3] = torch.tensor(np.array(body[str(j)]) / 100.)
        g = g.reshape((J, 3)).transpose(0, 1)
        hom = torch.cat((g, torch.ones(1, J)), 0)
        world = torch.matmul(T_i_cam1, torch.matmul(T_dataset_cam1, hom))[:-1].transpose(0, 1)
        gts.append({j: world[j].numpy() for j in parameters.joint_list if str(j) in body})
        valid.append('-1' in body)
    return gts, valid


def pack_ground_truth(frames, T_d1s, T_i1):
    """ground_truth() of every frame, packed for mpe_eval_batch: {'xyz': [B,Gcap,J,3] f32 world, 'joint': [B,Gcap,J] u8
    (joint given for the body), 'valid': [B,Gcap] u8 ('-1' in the body), 'n': [B] i32 (0: no GT bodies, the frame the
    callers skip)}; Gcap = the largest body count, at least 1.  The values are ground_truth()'s own, bit for bit; like
    it, raises SystemExit for a frame without a GT field."""
    J = len(parameters.joint_list)
    if list(parameters.joint_list) != list(range(J)):
        raise ValueError('pack_ground_truth: joint_list must be range(J)')
    per = [ground_truth(f, T, T_i1) for f, T in zip(frames, T_d1s)]
    B = len(per)
    gcap = max([1] + [len(g[0]) for g in per if g is not None])
    out = {'xyz': np.zeros((B, gcap, J, 3), np.float32), 'joint': np.zeros((B, gcap, J), np.uint8),
           'valid': np.zeros((B, gcap), np.uint8), 'n': np.zeros(B, np.int32)}
    for f, g in enumerate(per):
        if g is None:
            continue
        out['n'][f] = len(g[0])
        for b, (body, ok) in enumerate(zip(*g)):
            out['valid'][f, b] = ok
            for j, xyz in body.items():
                out['xyz'][f, b, j] = xyz
                out['joint'][f, b, j] = 1
    return out


class Metrics:
    """Bookkeeping of the two reference callers (metrics_from_model.py:303-390,
    metrics_from_triangulation.py:281-372), statement for statement.  The scripts differ in one
    place: the triangulation script marks a detection invalid when a used joint of the ground
    truth is missing from it (:297-298) and then books it as a false positive at every threshold
    (:333), while its MPJPE sum still counts it (:323-327)."""

    def __init__(self):
        self.acc_err = 0.0
        self.n_matching = 0
        self.n_poses = 0
        self.n_gt = 0
        self.TP = [[] for _ in THRESHOLDS_MM]
        self.FP = [[] for _ in THRESHOLDS_MM]

    def add_frame(self, gts, valid_gt, results, triangulation=False):
        """gts: list of {joint str or int: (3,)}; results: list of {joint idx: (3,)} in the order
        the 3D stage produced them."""
        G, R = len(gts), len(results)
        table = np.zeros((G, R))
        valid_detection = [True] * R
        for i, gt in enumerate(gts):
            for r, res in enumerate(results):
                tot, n = 0.0, 0
                for j, g in gt.items():
                    idx = int(j)
                    if idx in parameters.used_joints:
                        if idx in res:
                            tot += np.linalg.norm(np.asarray(res[idx]) - g)
                            n += 1
                        else:
                            valid_detection[r] = False
                if n > 0:
                    table[i, r] = tot / n
        perms = itertools.permutations(range(R), G) if G <= R else itertools.permutations(range(G), G)
        best, best_p = 10000., None
        for p in perms:
            acc = 0
            for i, r in enumerate(p):
                if r < R:
                    acc += table[i, r]
            if acc < best:
                best, best_p = acc, p
        self.n_poses += R
        self.n_gt += G
        for r in range(R):
            if r in best_p:
                i = best_p.index(r)
                if valid_gt[i]:
                    self.n_matching += 1
                    self.acc_err += table[i, r]
                else:
                    self.n_gt -= 1
            for k, th in enumerate(THRESHOLDS_MM):
                if r in best_p and (valid_detection[r] or not triangulation):
                    i = best_p.index(r)
                    if not valid_gt[i]:
                        continue
                    ok = table[i, r] * 1000. < th
                    self.TP[k].append(1 if ok else 0)
                    self.FP[k].append(0 if ok else 1)
                else:
                    self.TP[k].append(0)
                    self.FP[k].append(1)

    def report(self):
        out = {'ap': {}}
        for k, th in enumerate(THRESHOLDS_MM):
            tp, fp = np.cumsum(np.array(self.TP[k])), np.cumsum(np.array(self.FP[k]))
            recall = tp / (self.n_gt + 1e-5)
            precise = tp / (tp + fp + 1e-5)
            for n in range(len(self.TP[k]) - 2, -1, -1):
                precise[n] = max(precise[n], precise[n + 1])
            precise = np.concatenate(([0], precise, [0]))
            recall = np.concatenate(([0], recall, [1]))
            idx = np.where(recall[1:] != recall[:-1])[0]
            ap = np.sum((recall[idx + 1] - recall[idx]) * precise[idx + 1])
            print('AP, precise and recall for', th, ':', ap, precise[-2], recall[-2])
            out['ap'][str(int(th))] = [float(ap), float(precise[-2]), float(recall[-2])]
        if self.n_matching > 0:
            print('MEAN ERR (mm)', self.acc_err * 1000. / self.n_matching)
            out['mpjpe_mm'] = self.acc_err * 1000. / self.n_matching
        return out


class DeviceMetrics(Metrics):
    """Metrics fed by mpe_eval_batch instead of per-frame dicts: the table and the assignment come from the device
    (harness/assignment.py states them), the bookkeeping of Metrics.add_frame runs vectorised over the records of a
    batch in frame order, then detection order -- TP / FP per threshold, n_gt -= 1 for a match to an invalid GT body,
    the triangulation script's invalid detections as false positives -- and the MPJPE sum is a sequential np.cumsum
    (the host's left fold).  report() is Metrics.report()."""

    def add_batch(self, ev, gt_valid, triangulation=False):
        """ev: Engine.evaluate's tensors; gt_valid [B,Gcap] (pack_ground_truth's 'valid').  Frames the device search
        declined (over 64 rows or columns, over its node budget) are finished here by assignment.assign_bnb on the
        device's table.  -> the host records {'n_gt','n_res','status','assign','err','invalid'}."""
        h = {k: ev[k].cpu().numpy() for k in ('n_gt', 'n_res', 'status', 'assign', 'err', 'invalid')}
        for f in np.flatnonzero(h['status'] & (MPE_EVAL_OVER_CAP | MPE_EVAL_OVER_BUDGET)):
            G, R = int(h['n_gt'][f]), int(h['n_res'][f])
            table = ev['table'][f, :G, :R].cpu().numpy()
            best_p = assign_bnb(table)
            if best_p is None:
                h['status'][f] |= MPE_EVAL_NO_ASSIGNMENT
            h['assign'][f, :R], h['err'][f, :R] = frame_records(table, best_p)
        keep = (h['status'] & MPE_EVAL_SKIPPED) == 0
        if np.any(keep & (h['status'] & MPE_EVAL_NO_ASSIGNMENT != 0) & (h['n_res'] > 0)):
            raise RuntimeError('no assignment sums below 10000 (the reference loop fails on such a frame)')
        n_res = h['n_res'].astype(np.int64)
        self.n_poses += int(n_res[keep].sum())
        self.n_gt += int(h['n_gt'][keep].sum())
        rec = keep[:, None] & (np.arange(h['assign'].shape[1])[None, :] < n_res[:, None])
        fr = np.nonzero(rec)[0]
        g, e, inv = h['assign'][rec], h['err'][rec], h['invalid'][rec] != 0
        has = g >= 0
        vg = np.zeros(len(g), bool)
        vg[has] = np.asarray(gt_valid, bool)[fr[has], g[has]]
        matched = has & vg
        self.n_matching += int(matched.sum())
        if matched.any():
            self.acc_err = np.cumsum(np.concatenate(([self.acc_err], e[matched])))[-1]
        self.n_gt -= int((has & ~vg).sum())
        cond = has & ~inv if triangulation else has
        kept = ~(cond & ~vg)
        for k, th in enumerate(THRESHOLDS_MM):
            tp = (cond & (e * 1000. < th))[kept].astype(np.int64)
            self.TP[k].extend(tp.tolist())
            self.FP[k].extend((1 - tp).tolist())
        return h


def teacher_scores(db, owners):
    """Ground-truth pairing as scores: 1 for two views of one person, 0 otherwise."""
    from ..packing import pairs_of_frame
    sc = np.zeros(db.n_edge_nodes, np.float32)
    pb = db.host
    sm = list(parameters.used_cameras_skeleton_matching)
    for f in range(pb.n_frames):
        h0, H, e0, M = pb.frame_counts(f)
        own = []
        for s in range(pb.V):
            c = pb.slot_cam[f, s]
            if c < 0:
                continue
            cam_owner = owners[f][sm[c]]
            # heads of the slot follow list order; skeletons without joints were skipped
            own += [cam_owner[i] for i in pb.skeleton_index[h0 + len(own): h0 + len(own) + pb.slot_n[f, s]]]
        for m, (a, b) in enumerate(pairs_of_frame(pb.slot_n[f])):
            sc[e0 + m] = 1.0 if (own[a] == own[b] and own[a] >= 0) else 0.0
    return torch.from_numpy(sc)


class DeviceGT:
    """--device-gt: the test files as bytes behind one mpe_json_index each, and for every item of `work` the (file, frame
    index) it came from.  runs(start, n) cuts a batch into stretches of one file, each a window (first frame, --datastep
    as the stride, count) of that file's index."""

    def __init__(self, eng, files, src, datastep):
        from ..packing import JsonIndex
        self.eng, self.src, self.datastep = eng, src, int(datastep)
        self.indexes = []
        for file in files:
            with open(file, 'rb') as fh:
                self.indexes.append(JsonIndex(fh.read()))
        self.windows = self.declined = 0

    def runs(self, start, n):
        i = 0
        while i < n:
            file_no, first = self.src[start + i]
            j = i + 1
            while j < n and self.src[start + j][0] == file_no:
                j += 1
            yield i, j, file_no, first
            i = j

    def bodies(self, file_no, first, count):
        """-> ParsedBodies of the window, or None where the host path has to take over."""
        self.windows += 1
        pb = self.eng.bodies_from_json(self.indexes[file_no], first, self.datastep, count)
        if pb.status != 0 or pb.n_frames != count:
            self.declined += 1
            return None
        return pb

    def ground_truth(self, start, chunk, T_d_files, T_i1):
        """pack_ground_truth's dict for a batch as device tensors: Engine.ground_truth per stretch, pack_ground_truth (uploaded)
        for a stretch the device declines."""
        dev, parts = self.eng.device, []
        for i, j, file_no, first in self.runs(start, len(chunk)):
            pb = self.bodies(file_no, first, j - i)
            if pb is not None:
                gt = self.eng.ground_truth(pb, [T_d_files[file_no].numpy()], np.zeros(j - i, np.int32), T_i1.numpy())
            else:
                host = pack_ground_truth([w[0] for w in chunk[i:j]], [w[1] for w in chunk[i:j]], T_i1)
                gt = {k: torch.from_numpy(host[k]).to(dev) for k in ('xyz', 'joint', 'valid', 'n')}
            parts.append(gt)
        gcap = max(p['xyz'].shape[1] for p in parts)
        out = {}
        for k in ('xyz', 'joint', 'valid', 'n'):
            cols = []
            for p in parts:
                t = p[k]
                if k != 'n' and t.shape[1] < gcap:
                    pad = torch.zeros((t.shape[0], gcap - t.shape[1]) + tuple(t.shape[2:]), dtype=t.dtype, device=dev)
                    t = torch.cat((t, pad), 1)
                cols.append(t)
            out[k] = torch.cat(cols, 0) if len(cols) > 1 else cols[0]
        return out

    def close(self):
        for ix in self.indexes:
            ix.close()


def collect_work(args, calib, src=None):
    """[(frame, T_dataset_cam1, owners or None)] honouring --datastep across files (the counter
    runs over all files, metrics_from_model.py:102-124).  src, a list, receives (file number, frame index in the file) of
    every item."""
    work = []
    if args.synthetic:
        spec = synthetic.FrameSpec(persons=args.persons, noise_px=args.noise_px)
        for i in range(args.synthetic):
            f, gt = synthetic.make_frame(calib, i, spec)
            work.append((f, torch.from_numpy(calib.T_d[1]).type(torch.float32), gt['owner']))
        return work
    tm_dir = args.tmdir[0]
    n_input = 0
    for file in args.testfiles:
        print(file)
        T_d1 = torch.from_numpy(dataset_transform(tm_dir, file).get_transform('root', parameters.camera_names[1])).type(torch.float32)
        for k, frame in enumerate(json.load(open(file, 'rb'))):
            n_input += 1
            if (n_input - 1) % args.datastep == 0:
                work.append((frame, T_d1, None))
                if src is not None:
                    src.append((args.testfiles.index(file), k))
    return work


def load_frames(args):
    """The frames of --testfiles at --datastep, the counter running over all files, as they are: no ground truth is read
    (harness.calibrate, harness.camfit, harness.lag)."""
    frames, n_input = [], 0
    for file in args.testfiles:
        with open(file, 'rb') as fh:
            for frame in json.load(fh):
                n_input += 1
                if (n_input - 1) % args.datastep == 0:
                    frames.append(frame)
    if not frames:
        raise SystemExit('no frames: give --testfiles or --synthetic N')
    return frames


def held_cameras(hold, names):
    """--hold (a list of names, or None: the rig's first camera) checked against the rig's `names` -> the list."""
    hold = [names[0]] if hold is None else list(hold)
    for h in hold:
        if h not in names:
            raise SystemExit('--hold %s: not a camera of the rig (%s)' % (h, ', '.join(names)))
    return hold


def evaluate(work, infer, mode, T_i1, batch=256):
    """The callers' loop around the inference path.  `infer(frames, owners)` receives the
    pre-processed frames of one batch (cameras with an empty skeleton list dropped, :182-191) and
    returns, per frame, None when the frame has no cross-camera pair (no graph, :195-196) or the
    list of 3D results {joint idx: (3,)} in production order.  Returns (Metrics, n_data, n_results)."""
    metrics = Metrics()
    n_data = n_results = 0
    for start in range(0, len(work), batch):
        keep, gts = [], []
        for frame, T_d1, owners in work[start:start + batch]:
            gt = ground_truth(frame, T_d1, T_i1)
            if gt is None:
                continue
            keep.append((frame, owners))
            gts.append(gt)
        if not keep:
            continue
        frames = [{c: [frame[c][0], frame[c][1]] for c in frame if json.loads(frame[c][0])} for frame, _ in keep]
        per_frame = infer(frames, [o for _, o in keep])
        for f, results in enumerate(per_frame):
            if results is None:
                continue
            n_data += 1
            n_results += len(results)
            metrics.add_frame(gts[f][0], gts[f][1], results, triangulation=(mode != 'mlp'))
    return metrics, n_data, n_results


def evaluate_on_device(work, infer, mode, T_i1, batch=256, device_gt=None, T_d_files=None, scored=None):
    """evaluate() with --device-metrics: `infer(frames, owners, gt)` runs the inference path and Engine.evaluate on
    the device and returns its tensors; the frames and the skip rules are evaluate()'s.  With device_gt (a DeviceGT,
    --device-gt) the ground truth of a batch is built on the device from the files' bytes and stays there; only the body
    counts and the '-1' flags of the batch come back.  scored(ev, h): called once per batch with the device tensors and
    the host records DeviceMetrics.add_batch finished.  Returns (DeviceMetrics, n_data, n_results)."""
    metrics = DeviceMetrics()
    n_data = n_results = 0
    for start in range(0, len(work), batch):
        chunk = work[start:start + batch]
        if device_gt is not None:
            gt = device_gt.ground_truth(start, chunk, T_d_files, T_i1)
            sel = np.flatnonzero(gt['n'].cpu().numpy() > 0)
            if not len(sel):
                continue
            pick = torch.from_numpy(sel).to(gt['n'].device)
            gt = {k: v.index_select(0, pick) for k, v in gt.items() if isinstance(v, torch.Tensor)}
            gt_valid = gt['valid'].cpu().numpy()
        else:
            gt = pack_ground_truth([w[0] for w in chunk], [w[1] for w in chunk], T_i1)
            sel = np.flatnonzero(gt['n'] > 0)
            if not len(sel):
                continue
            gt = {k: v[sel] for k, v in gt.items()}
            gt_valid = gt['valid']
        keep = [chunk[i] for i in sel]
        frames = [{c: [frame[c][0], frame[c][1]] for c in frame if json.loads(frame[c][0])} for frame, _, _ in keep]
        ev = infer(frames, [o for _, _, o in keep], gt)
        h = metrics.add_batch(ev, gt_valid, triangulation=(mode != 'mlp'))
        if scored is not None:
            scored(ev, h)
        done = (h['status'] & MPE_EVAL_SKIPPED) == 0
        n_data += int(done.sum())
        n_results += int(h['n_res'][done].sum())
    return metrics, n_data, n_results


def add_lags_option(p):
    """--lags of metrics_from_model and metrics_from_triangulation (harness/lag.py has a --lags of its own) -> p"""
    p.add_argument('--lags', dest='lags_file', type=str, default=None, metavar='lags.json',
                   help='needs --track; the file harness.lag --correct N --out wrote.  Where --refine runs, the time-aware refinement runs in '
                        'its place (mpe_refine_timed_batch with --refine\'s iterations, 10 without, and Huber option): every camera looks at a '
                        'joint where the joint\'s track says it was at that camera\'s time.  The tracks are those of the --batch chunk, so a '
                        'chunk\'s first and last ceil(|lag|) frames stay untimed; one further line reports the cameras with a lag, the joints '
                        'timed and the mean cost before and after')
    return p


def add_write_option(p):
    """--write-poses of metrics_from_model and metrics_from_triangulation -> p"""
    p.add_argument('--write-poses', dest='write_poses', type=str, default=None, metavar='poses.jsonl',
                   help='implies --device-metrics; the poses that are scored (after --refine, --smooth, --bones and so on) are written to this '
                        'file as JSON on the GPU (mpe_json_write_poses), one line per frame handed to the inference path, numbered from 0 in '
                        'that order: {"frame": n, "ids": [...], "bodies": [{"<joint>": [x, y, z], ...}, ...]}, metres, "ids" (the tracker\'s, '
                        'with --relink the relinker\'s) with --track.  The lines are appended chunk by chunk in --batch order; one further '
                        'line reports the frames, rows, joints and bytes written and the joints dropped because a coordinate was not finite.  '
                        'harness.write_poses.read_lines reads the file back')
    return p


def load_lags(path, names):
    """lags.json as harness.lag --out writes it ({'lags': {camera: frames}}; a bare {camera: frames} or a list over `names`
    is taken, too) -> [lag of every camera in `names`], 0.0 for a camera the file does not name."""
    import json
    with open(path) as fh:
        doc = json.load(fh)
    if isinstance(doc, dict) and 'lags' in doc:
        doc = doc['lags']
    if isinstance(doc, dict):
        unknown = [c for c in doc if c not in names]
        if unknown:
            raise ValueError('--lags: %s names cameras the rig does not use: %s' % (path, ', '.join(unknown)))
        return [float(doc.get(c, 0.0)) for c in names]
    if not isinstance(doc, list) or len(doc) != len(names):
        raise ValueError('--lags: %s must hold one lag for each of the %d cameras' % (path, len(names)))
    return [float(x) for x in doc]


def max_skeletons_per_camera(work):
    """Largest skeleton list of any camera in the selected frames: sizes the engine's per-frame
    capacity (the reference has no such limit; its graphs simply grow)."""
    m = 1
    for frame, _, _ in work:
        for cam in frame:
            m = max(m, frame[cam][0].count('{'))       # one '{' per skeleton dict in the JSON text
    return m


def run(args, mode):
    calib = start_calibration(args)
    device_gt = getattr(args, 'device_gt', False) and not args.synthetic       # synthetic frames have no file to parse
    refine = int(getattr(args, 'refine', 0) or 0)
    smooth = int(getattr(args, 'smooth', 0) or 0)
    track_score = bool(getattr(args, 'track_score', False))
    bones = int(getattr(args, 'bones', 0) or 0)
    if bones and not (1 <= bones <= 64 and args.bones_bin > 0 and np.isfinite(args.bones_bin)):
        raise ValueError('--bones takes 1 .. 64 sweeps and --bones-bin a width > 0 (got %d, %g)' % (bones, args.bones_bin))
    bones_refine = int(getattr(args, 'bones_refine', 0) or 0)
    if bones and bones_refine:
        raise ValueError('--bones and --bones-refine are two fits of the same poses: give one')
    if bones_refine and not (1 <= bones_refine <= 64 and args.bones_bin > 0 and np.isfinite(args.bones_bin) and args.bones_weight >= 0
                             and args.bones_huber >= 0):
        raise ValueError('--bones-refine takes 1 .. 64 sweeps, --bones-bin a width > 0, --bones-weight and --bones-huber no negative value '
                         '(got %d, %g, %g, %g)' % (bones_refine, args.bones_bin, args.bones_weight, args.bones_huber))
    uncertainty = float(getattr(args, 'uncertainty', 0.0) or 0.0)
    uncertainty_gate = float(getattr(args, 'uncertainty_gate', 0.0) or 0.0)
    if uncertainty != 0.0 or uncertainty_gate != 0.0:        # a NaN as well
        if not (uncertainty > 0.0 and np.isfinite(uncertainty) and uncertainty_gate >= 0.0):
            raise ValueError('--uncertainty takes a pixel noise > 0 and --uncertainty-gate no negative value (got %g, %g)' % (uncertainty, uncertainty_gate))
        if uncertainty_gate and mode == 'mlp':
            raise ValueError('--uncertainty-gate clears joint flags: metrics_from_triangulation only (the flags of metrics_from_model are per person)')
    relink = float(getattr(args, 'relink', 0.0) or 0.0)
    if relink != 0.0:                                        # a NaN as well
        relink_options = {'gate_m': relink / 1000.0, 'min_gap': args.track_gap + 2, 'max_gap': args.relink_max_gap, 'reach_m': args.relink_reach,
                          'reach_per_frame_m': args.relink_speed, 'min_bones': args.relink_min_bones}
        from . import relink as relink_rule
        try:
            relink_rule.check_options(relink_options, len(relink_rule.S.BONES_18))
        except ValueError as e:
            raise ValueError('--relink: %s' % e)
    if smooth or track_score or bones or bones_refine or relink:
        args.track = True
    lags = None
    if getattr(args, 'lags_file', None):
        if not getattr(args, 'track', False):
            raise ValueError('--lags needs --track: the offsets of a joint come from its track')
        lags = load_lags(args.lags_file, list(parameters.used_cameras_skeleton_matching))
    write_path = getattr(args, 'write_poses', None)
    if getattr(args, 'device_gt', False) or getattr(args, 'track', False) or refine or write_path or uncertainty:
        args.device_metrics = True
    src = [] if device_gt else None
    work = collect_work(args, calib, src)
    eng = Engine(parameters, calib, max_frames=args.batch,
                 max_persons_per_camera=max(4, args.persons + 1, max_skeletons_per_camera(work)))
    if getattr(args, 'gat_acc64', False) or getattr(args, 'mlp_precision', 'default') != 'default':
        eng.set_precision(gat_acc64=bool(getattr(args, 'gat_acc64', False)), mlp_max_accuracy=getattr(args, 'mlp_precision', '') == 'max_accuracy',
                          mlp_f64=getattr(args, 'mlp_precision', '') == 'f64')
    load_models(eng, args, need_mlp=(mode == 'mlp'))
    T_i1 = torch.from_numpy(calib.T_i32[1])
    J = eng.J
    t = {'match': 0.0, '3d': 0.0}
    tracker = summary = smoother = smoothed = gt_tracker = scorer = skeleton = boned = relinker = relinked = None
    last = {}                                                # what the track score of a batch needs from infer_device
    refined = []
    timed = []                                               # --lags: the time-aware refinement's outputs of every batch
    measured = []                                            # --uncertainty: mpe_posecov_batch's sigma and status of every batch
    regrouped = []                                         # --regroup: per round, the counts of every batch
    consolidated = []                                        # --merge / --found: the same of the consolidation
    used_mask = sum(1 << int(j) for j in parameters.used_joints)     # the joints both 3D stages of this script fill in
    written = None
    if write_path:
        written = {'file': open(write_path, 'wb'), 'frames': 0, 'rows': 0, 'joints': 0, 'bytes': 0, 'dropped': 0}
    if getattr(args, 'track', False):
        from .tracking import TrackSummary
        tracker, summary = eng.tracker(mode, max_gap=args.track_gap, gate=args.track_gate), TrackSummary()
    if relink:
        relinker, relinked = eng.relinker(mode, **relink_options), relink_rule.RelinkSummary()

    def track(p_in, f_in, n_in):
        """the tracker, then with --relink the re-identifier: its ids take the place of the tracker's, and a birth it linked is
        no birth (the gap of the link stands where the tracker wrote 0)"""
        tr = tracker.update(p_in, f_in, n_in)
        if relinker is not None:
            rl = relinker.update(p_in, f_in, n_in, tr['ids'])
            relinked.add(tr['ids'].cpu().numpy(), {k: rl[k].cpu().numpy() for k in ('ids', 'link_gap')})
            tr = dict(tr, ids=rl['ids'], gap=torch.where(tr['gap'] == 0, rl['link_gap'], tr['gap']))
        return tr
    if smooth:
        from .smoothing import SmoothSummary
        smoother, smoothed = eng.smoother(mode, window=smooth, decay=args.smooth_decay, fill=args.smooth_fill), SmoothSummary(mode)
    if bones:
        from .skeleton import SkeletonSummary
        skeleton, boned = eng.skeleton(mode, bin_mm=args.bones_bin), SkeletonSummary()
    if bones_refine:
        from .skeleton_refine import RefineSummary
        skeleton, boned = eng.skeleton(mode, bin_mm=args.bones_bin), RefineSummary()
    if track_score:
        # GT identities: the GT bodies of the evaluated frames through a tracker of their own, same gate and gap
        gt_tracker = eng.tracker('gt', max_gap=args.track_gap, gate=args.track_gate, pcap=TRACK_SCORE_GCAP)
        scorer = eng.track_scorer(mode, threshold_mm=args.track_score_mm, gcap=TRACK_SCORE_GCAP)

    def infer(frames, owners):
        db = eng.to_device(eng.pack(frames))
        torch.cuda.synchronize()
        t0 = time.time()
        if args.teacher_scores and owners[0] is not None:
            persons, n_persons = eng.cluster(db, teacher_scores(db, owners))
        else:
            persons, n_persons = match_stage(eng, args, db)
        torch.cuda.synchronize()
        t1 = time.time()
        if mode == 'mlp':
            poses, valid = eng.mlp3d(db, persons, n_persons)
            persons, n_persons, poses, valid = repair_stage(eng, args, db, persons, n_persons, poses, valid, mode, regrouped, consolidated,
                                                            lambda rows, n: eng.mlp3d(db, rows, n), used_mask)
        else:
            poses, jvalid = eng.triangulate(db, persons, n_persons)
            persons, n_persons, poses, jvalid = repair_stage(eng, args, db, persons, n_persons, poses, jvalid, mode, regrouped, consolidated,
                                                             lambda rows, n: eng.triangulate(db, rows, n), used_mask)
        torch.cuda.synchronize()
        t['match'] += t1 - t0
        t['3d'] += time.time() - t1
        eng.sync_status()
        n_np, poses = n_persons.cpu().numpy(), poses.cpu().numpy()
        flags = (valid if mode == 'mlp' else jvalid).cpu().numpy()
        out = []
        for f in range(len(frames)):
            h0, H, e0, M = db.host.frame_counts(f)
            if M == 0:
                out.append(None)
                continue
            results = []
            for p in range(int(n_np[f])):
                if mode == 'mlp':
                    if flags[f, p]:
                        results.append({j: poses[f, p, j] for j in range(J)})
                else:
                    results.append({j: poses[f, p, j] for j in range(J) if flags[f, p, j]})
            out.append(results)
        return out

    def infer_device(frames, owners, gt):
        db = eng.to_device(eng.pack(frames))
        torch.cuda.synchronize()
        t0 = time.time()
        if args.teacher_scores and owners[0] is not None:
            persons, n_persons = eng.cluster(db, teacher_scores(db, owners))
        else:
            persons, n_persons = match_stage(eng, args, db)
        torch.cuda.synchronize()
        t1 = time.time()
        if mode == 'mlp':
            poses, flags = eng.mlp3d(db, persons, n_persons)
        else:
            poses, flags = eng.triangulate(db, persons, n_persons)
        persons, n_persons, poses, flags = repair_stage(eng, args, db, persons, n_persons, poses, flags, mode, regrouped, consolidated,
                                                        lambda rows, n: eng.mlp3d(db, rows, n) if mode == 'mlp' else eng.triangulate(db, rows, n),
                                                        used_mask)
        tr = None
        if tracker is not None:
            # the frames that are evaluated (a cross-camera pair, as Engine.evaluate's skip rule has it), in order
            keep = torch.from_numpy(np.flatnonzero(np.diff(np.asarray(db.host.frame_en_off[:db.n_frames + 1])) != 0)).to(poses.device)
        if lags is not None:
            # --lags: track first (the unrefined poses), then the time-aware refinement against the chunk's own frames as the table;
            # a frame that is not evaluated is a time step without ids
            tr = track(poses.index_select(0, keep), flags.index_select(0, keep), n_persons.index_select(0, keep))
            ids = torch.full(tuple(poses.shape[:2]), -1, dtype=torch.int32, device=poses.device).index_copy_(0, keep, tr['ids'])
            ref = eng.refine_timed(db, 0, persons, poses, flags, n_persons, ids, 'est' if mode == 'mlp' else 'triang', lags,
                                   max_iters=refine or 10, huber_px=args.refine_huber)
            poses = ref['poses']
            timed.append({k: ref[k].cpu().numpy() for k in ('status', 'cost0', 'cost1', 'n_timed')})
        elif refine:
            ref = eng.refine(db, persons, n_persons, poses, flags, 'est' if mode == 'mlp' else 'triang', max_iters=refine,
                             huber_px=args.refine_huber, out=poses)
            refined.append({k: ref[k].cpu().numpy() for k in ('status', 'cost0', 'cost1') + (('n_views',) if uncertainty else ())})
        if uncertainty:
            # the covariance of the poses as they are now; with a gate the joints above it lose their flag here, before tracking
            # (with --lags the tracker has already run on the unrefined poses: the gate then acts on what is smoothed, scored and written)
            pc = eng.pose_covariance(db, persons, n_persons, poses, flags, 'est' if mode == 'mlp' else 'triang', uncertainty,
                                     huber_px=args.refine_huber if (refine or lags is not None) else 0.0, gate_m=uncertainty_gate / 1000.0,
                                     flags_out=flags if uncertainty_gate else None)
            in_use = torch.arange(poses.shape[1], device=poses.device)[None, :] < n_persons.clamp(0, poses.shape[1])[:, None]
            left = (flags != 0) & (in_use[..., None] if flags.dim() == 3 else in_use)
            measured.append(dict({k: pc[k].cpu().numpy() for k in ('sigma', 'status')}, flagged=int(left.sum()) * (1 if flags.dim() == 3 else J)))
        torch.cuda.synchronize()
        t2 = time.time()
        if smoother is not None or skeleton is not None:
            # track, then smooth, then bones, then scoring: the fitted poses of the tracked frames take the place of the raw ones
            p_in, f_in, n_in = poses.index_select(0, keep), flags.index_select(0, keep), n_persons.index_select(0, keep)
            tr = tr if tr is not None else track(p_in, f_in, n_in)
            p_cur, f_cur = p_in, f_in
            if smoother is not None:
                sm = smoother.update(p_in, f_in, n_in, tr['ids'])
                p_cur, f_cur = sm['poses'], sm['flags']
            if skeleton is not None:
                # the lengths a chunk is fitted with are those of the recording up to and including the chunk
                p_sk = p_cur
                skeleton.observe(p_sk, f_cur, n_in, tr['ids'])
                skeleton.update(args.bones_min)
                if bones_refine:
                    sk = eng.body_refine(skeleton, db, persons.index_select(0, keep), n_in, p_sk, f_cur, tr['ids'], sweeps=bones_refine,
                                         bone_weight=float(args.bones_weight), huber_px=float(args.bones_huber), frames=keep.to(torch.int32))
                else:
                    sk = skeleton.fit(p_sk, f_cur, n_in, tr['ids'], iters=bones)
                p_cur = sk['poses']
            poses, flags = poses.index_copy(0, keep, p_cur), flags.index_copy(0, keep, f_cur)
            torch.cuda.synchronize()
        t3 = time.time()
        ev = eng.evaluate(db, poses, flags, n_persons, gt, mode)
        torch.cuda.synchronize()
        t['match'] += t1 - t0
        t['3d'] += t2 - t1
        t['eval'] += time.time() - t3
        eng.sync_status()
        if smoother is not None or skeleton is not None:
            summary.add(tr['ids'].cpu().numpy(), tr['gap'].cpu().numpy())
            if smoother is not None:
                smoothed.add(p_in.cpu().numpy(), f_in.cpu().numpy(), {k: sm[k].cpu().numpy() for k in ('poses', 'flags', 'n_samples')})
            if skeleton is not None:
                boned.add(p_sk.cpu().numpy(), {k: v.cpu().numpy() for k, v in sk.items()})
        elif tracker is not None:
            tr = tr if tr is not None else track(poses.index_select(0, keep), flags.index_select(0, keep), n_persons.index_select(0, keep))
            summary.add(tr['ids'].cpu().numpy(), tr['gap'].cpu().numpy())
        if scorer is not None:
            last.update(flags=flags, n_persons=n_persons, ids=tr['ids'])
        if written is not None:
            # what evaluate scored, every frame of the chunk; a frame the tracker did not see (no cross-camera pair) has the id -1
            ids = None
            if tracker is not None:
                ids = torch.full(tuple(poses.shape[:2]), -1, dtype=torch.int32, device=poses.device).index_copy_(0, keep, tr['ids'])
            w = eng.write_poses(poses, flags, n_persons, 'est' if mode == 'mlp' else 'triang', ids=ids, frame_start=written['frames'])
            data = w.bytes()
            written['file'].write(data)
            # every written joint opens one list, as do "bodies" and "ids" once per line; flagged joints of the rows in use
            n_lines = int(poses.shape[0])
            joints = data.count(b'": [') - n_lines * (1 if ids is None else 2)
            per_row = (flags != 0).sum(dim=-1) if flags.dim() == 3 else (flags != 0).to(torch.int64) * J
            in_use = torch.arange(poses.shape[1], device=poses.device)[None, :] < n_persons.clamp(0, poses.shape[1])[:, None]
            flagged = int((per_row * in_use).sum())
            written['frames'] += int(poses.shape[0])
            written['rows'] += int(w.rows_written.sum())
            written['joints'] += joints
            written['dropped'] += flagged - joints
            written['bytes'] += len(data)
        return ev

    def score_tracks(ev, h):
        """refine, track, smooth, evaluate, then this: the batch's frames through the scorer, the ones evaluate skipped
        marked as such.  Frames the device search declined carry the rows add_batch finished on the host."""
        dev = last['ids'].device
        B, P, G = len(h['status']), last['ids'].shape[1], TRACK_SCORE_GCAP
        gx, gj, gv, gn, _ = ev['_keep']
        if gx.shape[1] > G:
            raise RuntimeError('--track-score holds %d ground-truth bodies per frame, a frame has %d' % (G, gx.shape[1]))
        if (h['status'] & (MPE_EVAL_OVER_CAP | MPE_EVAL_OVER_BUDGET)).any():
            ev = dict(ev, assign=torch.from_numpy(h['assign']).to(dev), err=torch.from_numpy(h['err']).to(dev))
        skipped = (h['status'] & MPE_EVAL_SKIPPED) != 0
        keep = torch.from_numpy(np.flatnonzero(~skipped)).to(dev)
        if len(keep) != last['ids'].shape[0]:
            raise RuntimeError('the tracker saw %d frames, the evaluation %d' % (last['ids'].shape[0], len(keep)))

        def padded(t):
            out = torch.zeros((len(keep), G) + tuple(t.shape[2:]), dtype=t.dtype, device=dev)
            out[:, :t.shape[1]] = t.index_select(0, keep)
            return out
        gt_ids = torch.full((B, G), -1, dtype=torch.int32, device=dev)
        gt_ids.index_copy_(0, keep, gt_tracker.update(padded(gx), padded(gj), gn.index_select(0, keep))['ids'])
        gt_valid = torch.zeros((B, G), dtype=torch.uint8, device=dev)
        gt_valid[:, :gv.shape[1]] = gv
        ids = torch.full((B, P), -1, dtype=torch.int32, device=dev).index_copy_(0, keep, last['ids'])
        scorer.update(ev, last['flags'], last['n_persons'], ids, gt_ids, gt_valid, skip=torch.from_numpy(skipped.astype(np.uint8)).to(dev))

    if getattr(args, 'device_metrics', False):
        t['eval'] = 0.0
        dgt, T_d_files = None, None
        if device_gt:
            dgt = DeviceGT(eng, args.testfiles, src, args.datastep)
            T_d_files = [torch.from_numpy(dataset_transform(args.tmdir[0], file).get_transform('root', parameters.camera_names[1])).type(torch.float32)
                         for file in args.testfiles]
        metrics, n_data, n_results = evaluate_on_device(work, infer_device, mode, T_i1, args.batch, dgt, T_d_files,
                                                        score_tracks if scorer is not None else None)
        if dgt is not None:
            print('Ground truth on the device: %d windows, %d redone on the host' % (dgt.windows, dgt.declined))
            gt_windows = (dgt.windows, dgt.declined)
            dgt.close()
    else:
        metrics, n_data, n_results = evaluate(work, infer, mode, T_i1, args.batch)
    out = metrics.report()
    if report_matcher(args) is not None:
        out['matcher'] = dict(geom_options(args), name='geometric')
    if n_data > 0:
        print('Mean time for graph matching', t['match'] / n_data)
        print('Mean time for graph matching (per person)', t['match'] / max(1, n_results))
        print('Mean time for 3D', t['3d'] / n_data)
        print('Mean time for 3D (per person)', t['3d'] / max(1, n_results))
        print('Frames per second', n_data / max(1e-9, t['match'] + t['3d']))
        if 'eval' in t:
            print('Mean time for evaluation on the device', t['eval'] / n_data)
    if getattr(args, 'regroup', 0.0):
        out['regroup'] = report_regroup(args, regrouped)
    if getattr(args, 'merge', 0.0) or getattr(args, 'found', 0.0):
        out['consolidate'] = report_consolidate(args, consolidated)
    if lags is not None:
        from .refine_timed import summary as timed_summary
        out['refine_timed'] = r = timed_summary(timed, lags)
        print('Refined in time (%d cameras with a lag, at most %d iterations, Huber %g px): %d joints solved, %d timed, mean cost %.6g -> %.6g px^2'
              % (r['cameras_lagged'], refine or 10, args.refine_huber, r['solved'], r['joints_timed'], r['mean_cost0'], r['mean_cost1']))
    elif refine:
        from .refine import summary as refine_summary
        out['refine'] = r = refine_summary(refined)
        print('Refined (at most %d iterations, Huber %g px): %d joints solved, %.1f %% moved, mean cost %.6g -> %.6g px^2'
              % (refine, args.refine_huber, r['solved'], 100.0 * r['moved_share'], r['mean_cost0'], r['mean_cost1']))
    if uncertainty:
        from . import uncertainty as uncertainty_rule
        out['uncertainty'] = r = uncertainty_rule.summary(measured)
        r['sigma_px'], r['gate_mm'] = uncertainty, uncertainty_gate
        r['joints_flagged'] = sum(m['flagged'] for m in measured)      # what goes on to tracking, scoring and writing, after the gate
        if refine and lags is None and args.refine_huber == 0.0:
            r['pooled_sigma_px'], r['pooled_dof'] = uncertainty_rule.pixel_sigma(refined)
        print(uncertainty_rule.report_line(uncertainty, uncertainty_gate, r, r.get('pooled_sigma_px')))
    if tracker is not None:
        out['tracks'] = summary.result()
        print('Tracks (gate %g m, gap %d): %d, mean length %.3f frames, %d born after the first frame'
              % (args.track_gate, args.track_gap, out['tracks']['tracks'], out['tracks']['mean_length'], out['tracks']['late_births']))
        tracker.close()
    if relinker is not None:
        out['relink'] = r = relinked.result(relinker.counters())
        print(relink_rule.report_line(relink, args.relink_max_gap, r))
        relinker.close()
    if smoother is not None:
        out['smooth'] = r = smoothed.result()
        print('Smoothed (window %d, decay %g%s): %d joints fitted, %d filled, mean displacement %.3f mm'
              % (smooth, args.smooth_decay, ', fill' if args.smooth_fill else '', r['fitted'], r['filled'], r['mean_move_mm']))
        smoother.close()
    if skeleton is not None and bones_refine:
        from .skeleton_refine import report_line as body_line
        out['bones_refine'] = r = boned.result(skeleton.lengths())
        print(body_line(bones_refine, args.bones_weight, args.bones_huber, r))
        skeleton.close()
    elif skeleton is not None:
        from .skeleton import report_line as bones_line
        out['bones'] = r = boned.result(skeleton.lengths())
        print(bones_line(bones, args.bones_bin, args.bones_min, r))
        skeleton.close()
    if scorer is not None:
        from .track_score import report_line
        out['track_score'] = scorer.result()
        print(report_line(out['track_score'], args.track_score_mm))
        scorer.close()
        gt_tracker.close()
    if written is not None:
        written.pop('file').close()
        out['write_poses'] = written
        print('Wrote %d frames to %s: %d rows, %d joints, %d bytes, %d joints dropped as not finite'
              % (written['frames'], write_path, written['rows'], written['joints'], written['bytes'], written['dropped']))
    out['n_data'] = n_data
    if device_gt:
        out['gt_windows'], out['gt_declined'] = gt_windows
    eng.close()
    return out
