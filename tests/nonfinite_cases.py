"""Cases, poisons and checkers for the non-finite-input tests of the matching stage and the 3D stage
(test_nonfinite_cases_host.py: the yardstick and the checkers on their own, on the CPU; test_gpu_nonfinite.py: isolation of a bad
detection inside a batch and recovery of the context after it).  A bad detection is a coordinate or a probability that is inf, NaN,
or finite as a double and infinite as a float.  Everything is seeded.  Not a test module.

Frames: the synthetic recipe of test_gpu_l0_attention.py (synthetic.make_frame, then the oracle's processed_input) on the 5 x 4 rig
(at most 20 heads per frame) and one 5 x 10 set (up to 50): 1 to 4 (10) persons, dropped joints, a person missing from two cameras,
one frame with no graph.  A batch is a name of BATCHES; `batch(calib, name)` builds it once per process.

LARGE_FINITE_M: the pixel magnitude of the `large_finite` poison.  How it was found (find_large_finite_power, held by
test_nonfinite_cases_host.py): for every frame that Test D poisons (LARGE_FINITE_FRAMES), x of the poisoned joint is set to 10^e and
the oracle's fp32 forward of that frame is evaluated on the CPU, e = 38 downwards; the largest e with every score of the frame
finite is that frame's exponent, and M is 10^(the smallest of them), so that one constant serves every frame of the table.  Found:
38 for all six frames, the first exponent tried -- 10^39 is no float.  The value enters a head row as (x - W/2) / (W/2), about 1e35,
and through K^-1 as a ray of about x / f; the fixture weights shrink it from layer to layer, and the reference's softmax subtracts the
row maximum, so nothing overflows.  (3e38, the xy_3e38 poison, is finite as well in the oracle; it still moves every score.)"""
import copy
import json

import numpy as np

from conftest import oracle, pkg

KINDS = ('xy_inf', 'xy_nan', 'xy_f32_overflow', 'xy_3e38', 'prob_nan', 'masked_nan', 'large_finite')
# (every kind of the issue's table changes the oracle's scores of its frame or makes them non-finite -- test_nonfinite_cases_host.py
# checks that -- so none was dropped)
LARGE_FINITE_M = 1e38

# what a poison writes: (array, component, value); masked_nan writes three values under a CLEARED mask bit
_WRITES = {
    'xy_inf': ('xy', 0, float('inf')),
    'xy_nan': ('xy', 1, float('nan')),
    'xy_f32_overflow': ('xy', 0, 1e39),            # a finite double; inf as a float
    'xy_3e38': ('xy', 0, 3e38),                    # finite as a float, a factor 1.13 below the largest one
    'prob_nan': ('vp', 1, float('nan')),
    'large_finite': ('xy', 0, LARGE_FINITE_M),
}
_JSON_FIELD = {('xy', 0): 1, ('xy', 1): 2, ('vp', 0): 3, ('vp', 1): 4}      # joint value = [id, x, y, valid, prob]
ARRAY_NAMES = ('frame_head_off', 'frame_en_off', 'slot_cam', 'slot_n', 'head_cam', 'skeleton_index', 'joint_mask', 'tri_mask', 'xy', 'vp')


# ---- frames -----------------------------------------------------------------------------------------------------------------
def _spec(persons, drop=0.0, cameras_left=None, missing=()):
    return (persons, drop, cameras_left, tuple(missing))


# name -> (rig: persons per camera the engine is built for, first frame index, one spec per frame)
BATCHES = {
    # 18 frames, the batch path (one k_l0_attention launch).  Frame 6 has one camera: heads, no edge-node, no graph
    'A18': (4, 7500, [_spec(4, .15), _spec(2), _spec(3, .15), _spec(1), _spec(4), _spec(4, .15, missing=(1, 3)), _spec(2, .15, cameras_left=1),
                      _spec(4, .15), _spec(3), _spec(4, .15), _spec(2, .15), _spec(4), _spec(1, .3), _spec(4, .15), _spec(3, 0., missing=(0, 2)),
                      _spec(4, .15), _spec(2), _spec(4, .15)]),
    # 3 frames: the small-batch route
    'S3': (4, 7540, [_spec(4, .15), _spec(3, .15), _spec(2, .15)]),
    # 18 full frames: at least as many nodes as any other 5 x 4 batch here
    'P18': (4, 7560, [_spec(4, .1)] * 18),
    # 17 frames of another layout: node index r belongs to another frame and another kind of node than in A18 / P18
    'C17': (4, 7600, [_spec(1, .1), _spec(4), _spec(2, .15), _spec(4, .1), _spec(3), _spec(2, .15, cameras_left=2), _spec(4, .15), _spec(1),
                      _spec(3, .15, missing=(2, 4)), _spec(4), _spec(2, .1), _spec(4, .15), _spec(3), _spec(1, .2), _spec(4), _spec(2), _spec(3, .15)]),
    # 5 x 10, 17 frames: layer 0 stays on the coefficient kernel and k_gat_fused (the head rows do not fit k_l0_attention's LDS)
    'T17': (10, 7700, [_spec(10, .05), _spec(7), _spec(10, .1), _spec(4, .05), _spec(9, .05), _spec(10), _spec(2, .1), _spec(8, .05), _spec(10, .05),
                       _spec(6, .05), _spec(10, .1), _spec(3), _spec(10, .05, missing=(0, 3)), _spec(5, .1), _spec(10), _spec(1, .05), _spec(10, .05)]),
}
# Test A / Test D poison one frame: the first of the batch, and one in the middle whose rows share a 16-row tile with both neighbours
POSITIONS = {'A18': (0, 9), 'S3': (0, 1), 'T17': (0, 4)}
LARGE_FINITE_FRAMES = [(name, f) for name in ('A18', 'S3', 'T17') for f in POSITIONS[name]]

_built = {}


def raw_frame(calib, index, persons, drop=0.0, cameras_left=None, missing=()):
    """A synthetic frame in wire format; cameras_left: only the first so many cameras see anybody; missing: camera positions whose
    FIRST skeleton is taken out (a person some cameras do not see)."""
    syn = pkg('synthetic')
    cams = list(calib.params.used_cameras_skeleton_matching)
    empty = () if cameras_left is None else tuple(cams[cameras_left:])
    frame = syn.make_frame(calib, index, syn.FrameSpec(persons=persons, empty_cameras=empty, joint_drop=drop))[0]
    for c in missing:
        entry = frame[cams[c]]
        sk = json.loads(entry[0])
        entry[0] = json.dumps(sk[1:])
        entry[3] = entry[3][1:]
    return frame


def batch(calib, name):
    """-> {'name', 'rig', 'raw' (wire format), 'frames' (processed_input of them), 'pb' (PackedBatch)}; built once, left alone."""
    if name not in _built:
        rig, start, specs = BATCHES[name]
        raw = [raw_frame(calib, start + i, *s) for i, s in enumerate(specs)]
        frames = [oracle().processed_input(f) for f in raw]
        _built[name] = {'name': name, 'rig': rig, 'raw': raw, 'frames': frames, 'pb': pkg('packing').pack_frames(frames, calib.params)}
    return _built[name]


def node_ranges(pb):
    """[first node row, one past the last] of every frame: a frame's rows are its heads, then its edge-nodes."""
    return [(h0 + e0, h0 + e0 + H + M) for h0, H, e0, M in (pb.frame_counts(f) for f in range(pb.n_frames))]


def shares_tiles_with_both_neighbours(pb, f, tile=16):
    """Do frame f's node rows share a `tile`-row tile with the frame before AND the frame after (both with rows of their own)?"""
    if f <= 0 or f >= pb.n_frames - 1:
        return False
    r = node_ranges(pb)
    (a0, a1), (b0, b1), (c0, c1) = r[f - 1], r[f], r[f + 1]
    return a1 > a0 and c1 > c0 and b1 > b0 and b0 % tile != 0 and b1 % tile != 0


# ---- poisons ----------------------------------------------------------------------------------------------------------------
def copy_batch(pb):
    out = copy.copy(pb)
    for name in ARRAY_NAMES:
        setattr(out, name, np.array(getattr(pb, name), copy=True))
    return out


def poison(pb, frame, kind, head=None):
    """A copy of `pb` with ONE value replaced (masked_nan: three, all under a cleared mask bit) on one head of `frame`: on a joint
    present in both joint_mask and tri_mask, or for masked_nan on a joint ABSENT from joint_mask.  head: the frame-local head to
    poison (default: the first head of the frame that has such a joint).  Counts and masks stay as they are (asserted).
    out.poisoned = {'frame', 'head' (frame-local), 'joint', 'kind', 'writes': [(array, component, value)]}."""
    assert kind in KINDS, kind
    out = copy_batch(pb)
    h0, H, _, _ = pb.frame_counts(frame)
    J = pb.J
    heads = range(H) if head is None or kind == 'masked_nan' else [int(head)]
    pick = None
    for lh in heads:
        jm, tm = int(pb.joint_mask[h0 + lh]), int(pb.tri_mask[h0 + lh])
        js = [j for j in range(J) if (not (jm >> j & 1) if kind == 'masked_nan' else (jm >> j & 1) and (tm >> j & 1))]
        if js:
            pick = (lh, js[len(js) // 2])
            break
    assert pick is not None, 'frame %d has no head with a joint for %s' % (frame, kind)
    lh, j = pick
    nan = float('nan')
    writes = [('xy', 0, nan), ('xy', 1, nan), ('vp', 1, nan)] if kind == 'masked_nan' else [_WRITES[kind]]
    for name, comp, value in writes:
        getattr(out, name)[h0 + lh, j, comp] = value
    for name in ARRAY_NAMES[:8]:
        assert getattr(out, name).tobytes() == getattr(pb, name).tobytes(), name
    assert (out.n_frames, out.n_heads, out.n_edge_nodes) == (pb.n_frames, pb.n_heads, pb.n_edge_nodes)
    assert bool(int(pb.joint_mask[h0 + lh]) >> j & 1) == (kind != 'masked_nan')
    out.poisoned = {'frame': int(frame), 'head': int(lh), 'joint': int(j), 'kind': kind, 'writes': writes}
    return out


def poison_more(pb, frames, kind, heads=None):
    """`pb` with one head of each of `frames` poisoned (the schedules of Test B); heads: {frame: frame-local head} where the caller
    wants a certain one (a member of a person)."""
    out, marks = pb, []
    for f in frames:
        out = poison(out, f, kind, head=(heads or {}).get(f))
        marks.append(out.poisoned)
    out.poisoned_all = marks
    return out


def poisoned_frame(frames, pb, calib):
    """The oracle's view of a poisoned batch: a copy of frame pb.poisoned['frame'] (processed wire format) with the same values in
    its JSON.  A write under a cleared mask bit has no joint key to go to: the frame comes back equal (the reference never sees it)."""
    info = pb.poisoned
    frame = copy.deepcopy(frames[info['frame']])
    if info['kind'] == 'masked_nan':
        return frame
    sm = list(calib.params.used_cameras_skeleton_matching)
    h = int(pb.frame_head_off[info['frame']]) + info['head']
    cam = sm[int(pb.head_cam[h])]
    sks = json.loads(frame[cam][0])
    for name, comp, value in info['writes']:
        sks[int(pb.skeleton_index[h])][str(info['joint'])][_JSON_FIELD[name, comp]] = value
    frame[cam][0] = json.dumps(sks)                       # (json writes NaN / Infinity / 1e+39, and json.loads takes them back)
    return frame


# ---- checkers ---------------------------------------------------------------------------------------------------------------
def structural_fault(persons, n_persons, pb, f, pcap):
    """What downstream kernels rely on in frame f of a person table (persons [B, pcap, V], n_persons [B]); None, or what is wrong."""
    n = int(n_persons[f])
    if n < 0 or n > pcap:
        return 'frame %d: %d persons outside 0 .. %d' % (f, n, pcap)
    h0, H, _, _ = pb.frame_counts(f)
    seen = set()
    for p in range(n):
        for c in range(pb.V):
            lh = int(persons[f, p, c])
            if lh == -1:
                continue
            # a local head index inside the camera slot of column c: a head of this frame that belongs to camera c
            if lh < 0 or lh >= H or int(pb.head_cam[h0 + lh]) != c:
                return 'frame %d person %d: entry %d is no head of camera %d' % (f, p, lh, c)
            if lh in seen:
                return 'frame %d person %d: head %d appears twice' % (f, p, lh)
            seen.add(lh)
    return None


def structurally_valid(persons, n_persons, pb, f, pcap):
    return structural_fault(persons, n_persons, pb, f, pcap) is None


# ---- the oracle's side (CPU) ------------------------------------------------------------------------------------------------
def oracle_scores(frame, calib, gat, f64=False):
    """(heads, scores of every node: heads first, then edge-nodes) of one processed frame from the oracle's gat_forward in fp32 (the
    reference) or float64; None for a frame without a graph."""
    import torch
    onp = oracle()
    g = onp.build_graph(frame, calib)
    if g is None:
        return None
    sd, prm = gat
    return g['H'], onp.gat_forward(sd, prm, g['feats'], g['src'], g['dst'], dtype=torch.float64 if f64 else torch.float32).numpy()


def oracle_person_row(frame, person, calib):
    """The reference's MLP input row of one person (frame-local head per camera, -1 = none) of a processed frame, and what its own
    test sum(|row|) > 1 says about it, evaluated with numpy on that row.  LAPACK declines a matrix with a non-finite entry where
    OpenCV's SVD returns non-finite numbers: such a pair solve counts as NaN."""
    onp = oracle()
    sm = list(calib.params.used_cameras_skeleton_matching)
    heads = onp.parse_frame(frame, calib.params)['heads']
    jsons = {i: h[2] for i, h in enumerate(heads)}
    solve = onp.dlt_pair

    def guarded(P1, P2, x1, x2):
        try:
            with np.errstate(all='ignore'):
                return solve(P1, P2, x1, x2)
        except np.linalg.LinAlgError:
            return np.full(3, np.nan)
    onp.dlt_pair = guarded
    try:
        with np.errstate(all='ignore'):
            row = onp.mlp_input_row(onp.person_skeletons([int(x) for x in person], jsons, sm), calib)[0].numpy()
    finally:
        onp.dlt_pair = solve
    with np.errstate(all='ignore'):
        kept = bool(np.sum(np.abs(row)) > 1)
    return row, kept


def find_large_finite_power(frames, pb, f, calib, gat, top=38):
    """The largest e <= top for which the oracle's fp32 forward of frame f, with x of the poisoned joint at 10^e, is finite."""
    for e in range(top, 0, -1):
        p = poison(pb, f, 'large_finite')
        h = int(pb.frame_head_off[f]) + p.poisoned['head']
        p.xy[h, p.poisoned['joint'], 0] = 10.0 ** e
        p.poisoned['writes'] = [('xy', 0, 10.0 ** e)]
        if np.isfinite(oracle_scores(poisoned_frame(frames, p, calib), calib, gat)[1]).all():
            return e
    return 0


# ---- schedules of Test B: (batch, frames poisoned with xy_nan) per step; a step without poison is compared with a fresh engine ----
SCHEDULES = {
    1: [('A18', ()), ('P18', (0, 9)), ('A18', ()), ('S3', ()), ('C17', ())],
    2: [('A18', ()), ('S3', (0, 1, 2)), ('A18', ()), ('S3', ()), ('C17', ())],
    3: [('P18', (0, 9)), ('A18', ())],                                   # once per precision mode, the mode set around it
    4: [('A18', (0, 9)), ('P18', ()), ('S3', ())],                        # mlp3d only: NaN rows, then more persons, then fewer
    5: [('A18', ()), ('P18', (0, 9)), ('A18', ()), ('S3', ())],           # the production ring: a sibling context, run_pipelined
}
# set_precision arguments of the modes that own workspaces
GAT_MODES = {'gat_acc64': dict(gat_acc64=True), 'attn_fp16': dict(attn_fp16=True), 'gat_reduced': dict(gat_reduced=True)}
MLP_MODES = {0: dict(mlp_acc64=False, mlp_split=False), 1: dict(mlp_acc64=True, mlp_split=False), 2: dict(mlp_bf16=True), 3: dict(),
             4: dict(mlp_max_accuracy=True), 5: dict(mlp_f64=True)}
