"""Non-finite detections in the matching stage and the 3D stage (cases: nonfinite_cases.py; the contract: include/mpe.h, "Non-finite
input" under mpe_match_batch and the five entry points beside it).  A coordinate that is inf, NaN, or finite as a double and infinite
as a float reaches the device (a 1e39 in a document goes through the host packer's strtod).  Two things are held here:

  A. isolation in space: one bad detection in one frame of a batch moves no bit of any other frame, on every attention route;
  B. recovery in time: the batches that follow a bad one on the same context give the bits a FRESH context gives -- the activation
     workspaces (act[3], mlp_act[2], the split planes gat_pl) hold layers of 400, 320, 150 columns in rows of act_ld, and a NaN a
     poisoned batch leaves behind a narrow layer's columns would meet the zero padding of the weights (0 * NaN is NaN);
  C. the wire format: a document whose middle frame holds 1e39, through stream_json;
  D. a joint at 1e38 pixels, large but finite for the reference's fp32 network: finite on the device, and no noisier.

Expected bits are a fresh engine's for the clean batch, themselves held to the oracle once (scores 2e-5, MLP input rows 3e-7)."""
import json
import os

import numpy as np
import pytest
import torch

import nonfinite_cases as nc
from conftest import ROOT, oracle, pkg

pytestmark = pytest.mark.gpu

ROUTE_ENV = ('MPE_LATENCY_PATH', 'MPE_NO_FUSED_ATTENTION', 'MPE_FUSED_NO_OVERLAP', 'MPE_NO_COEF_EPILOGUE', 'MPE_NO_HEAD_SRC_TABLE')
# route -> (batch, environment, k_l0_attention launches one match of it takes; None: not asserted)
ROUTES = {
    'small3': ('S3', {}, 0),                                          # k_lat_l0a / k_lat_attention / k_lat_gemm / k_lat_tail
    'batch3': ('S3', {'MPE_LATENCY_PATH': '0'}, None),
    'l0attn18': ('A18', {}, 1),                                       # k_l0_attention, k_gat_fused, k_last_fused
    'general18': ('A18', {'MPE_NO_FUSED_ATTENTION': '1'}, 0),         # k_attn_coef + k_aggregate_*
    'nooverlap18': ('A18', {'MPE_FUSED_NO_OVERLAP': '1'}, 0),
    'fused17_5x10': ('T17', {}, 0),                                   # layer 0 on k_gat_fused
}
MARGIN, FLOOR = 2.5, 2e-6                                             # test_score_noise_against_the_f64_network's: the same launches


@pytest.fixture(autouse=True)
def _default_route(monkeypatch):
    for name in ROUTE_ENV:
        monkeypatch.delenv(name, raising=False)


def _engine(calib, gat_weights, mlp_weights, rig, frames, precision=None):
    eng = pkg('pipeline').Engine(calib.params, calib, max_frames=frames, max_persons_per_camera=rig)
    eng.load_gat(*gat_weights)
    eng.load_mlp(mlp_weights)
    if precision:
        eng.set_precision(**precision)
    return eng


@pytest.fixture(scope='module')
def engines(calib, gat_weights, mlp_weights):
    """rig (persons per camera) -> the engine Test A, C and D run on, made at first use."""
    made = {}

    def get(rig):
        if rig not in made:
            made[rig] = _engine(calib, gat_weights, mlp_weights, rig, 18)
        return made[rig]
    yield get
    for e in made.values():
        e.close()


def _np(t):
    return t.cpu().numpy()


def _layer_rows(name, n_nodes, width):
    """Seeded finite input rows of the last layer for batch `name` (mpe_gat_layer with caller rows: copy_rows_in into act[0])."""
    seed = sum(ord(c) for c in name) + 4242
    return torch.from_numpy(np.random.default_rng(seed).standard_normal((n_nodes, width)).astype(np.float32))


def _run(eng, pb, persons=None, name=None, layer_first=False):
    """Every call of this file on one batch, in fresh device arrays -> numpy.  persons: (table, counts) the 3D calls take (default:
    what this match wrote).  name: also the last layer on caller rows (Test B) -- after the matching calls, or with layer_first as
    the FIRST call on the batch, so that it is the one to meet whatever the batch before left in act[0]."""
    db = eng.to_device(pb)
    out = {}

    def layer_last():
        last = len(eng.gat_dims) - 1
        out['layer_last'] = _np(eng.gat_layer(db, last, _layer_rows(name, pb.n_heads + pb.n_edge_nodes, eng.gat_dims[last][0])))
    if name is not None and layer_first:
        layer_last()
    before = eng.l0_attention_launches()
    sc, p, n = eng.match(db, want_scores=True)
    out['l0_launches'] = eng.l0_attention_launches() - before
    sc2, sh = eng.gat_scores(db, heads=True)
    out['layer0'] = _np(eng.gat_layer(db, 0, None))
    gs, gp, gn = eng.geom_match(db)
    if name is not None and not layer_first:
        layer_last()
    if persons is None:
        pp, nn = p, n
    else:
        pp, nn = torch.from_numpy(persons[0]).to(eng.device), torch.from_numpy(persons[1]).to(eng.device)
    out['mlp'] = tuple(_np(t) for t in eng.mlp3d(db, pp, nn))
    out['tri'] = tuple(_np(t) for t in eng.triangulate(db, pp, nn))
    out['rows'] = tuple(_np(t) for t in eng.mlp_input_rows(db, pp, nn))
    eng.sync_status()                                                  # raises on any status bit
    out.update(scores=_np(sc), scores_fwd=_np(sc2), head_scores=_np(sh), geom_scores=_np(gs), persons=(_np(p), _np(n)),
               geom_persons=(_np(gp), _np(gn)), persons_3d=(_np(pp), _np(nn)))
    return out


def _bits(a):
    a = np.ascontiguousarray(a)
    return a.view({4: np.int32, 8: np.int64, 1: np.uint8}[a.dtype.itemsize])


def _same(a, b):
    return a.shape == b.shape and np.array_equal(_bits(a), _bits(b))


def _compare(got, want, pb, frames, what, skip_head=None, parts=('graph', '3d')):
    """Frames `frames` of two runs of one batch.  'graph': scores, head scores and layer rows bit for bit (head scores and rows: frames
    with a graph -- the reference builds none otherwise and the kernels differ in what they leave there) and the person tables equal;
    '3d': every 3D slot's flags and the values under them bit for bit.  skip_head = (frame, head): the 3D slots of that frame whose
    person holds that head are left out."""
    for f in frames:
        h0, H, e0, M = pb.frame_counts(f)
        if 'graph' in parts:
            for key in ('scores', 'scores_fwd', 'geom_scores'):
                assert _same(got[key][e0:e0 + M], want[key][e0:e0 + M]), '%s: %s of frame %d' % (what, key, f)
            if M:
                assert _same(got['head_scores'][h0:h0 + H], want['head_scores'][h0:h0 + H]), '%s: head scores of frame %d' % (what, f)
                r0 = h0 + e0
                for key in ('layer0', 'layer_last'):
                    if key in want:
                        assert _same(got[key][r0:r0 + H + M], want[key][r0:r0 + H + M]), '%s: %s rows of frame %d' % (what, key, f)
            for key in ('persons', 'geom_persons'):
                n = int(want[key][1][f])
                assert int(got[key][1][f]) == n and np.array_equal(got[key][0][f, :n], want[key][0][f, :n]), '%s: %s of frame %d' % (what, key, f)
        if '3d' not in parts:
            continue
        table, counts = want['persons_3d']
        assert np.array_equal(got['persons_3d'][1], counts) and np.array_equal(got['persons_3d'][0][f, :counts[f]], table[f, :counts[f]])
        for p in range(table.shape[1]):
            if skip_head is not None and skip_head[0] == f and p < int(counts[f]) and skip_head[1] in table[f, p]:
                continue
            for key in ('mlp', 'tri', 'rows'):
                gv, gf = got[key][0][f, p], got[key][1][f, p]
                wv, wf = want[key][0][f, p], want[key][1][f, p]
                assert np.array_equal(gf, wf), '%s: %s flags of frame %d person %d' % (what, key, f, p)
                if np.ndim(wf) == 0:
                    same = not wf or _same(gv, wv)
                else:
                    same = _same(gv[wf != 0], wv[wf != 0])
                assert same, '%s: %s values of frame %d person %d' % (what, key, f, p)


def _member_head(run, f):
    """A frame-local head that frame f's first matched person holds."""
    table, n = run['persons']
    assert int(n[f]) >= 1, 'frame %d has no person' % f
    return int([x for x in table[f, 0] if x >= 0][0])


# ---- expected bits: a fresh engine per batch (and per precision mode), held to the oracle once ---------------------------------
_expected = {}


def _fresh(calib, gat_weights, mlp_weights, name, precision_key=None, precision=None):
    """The bits of every call on clean batch `name` from an engine that has done nothing else (in the default environment)."""
    key = (name, precision_key)
    if key not in _expected:
        assert not any(os.environ.get(v) for v in ROUTE_ENV)
        b = nc.batch(calib, name)
        eng = _engine(calib, gat_weights, mlp_weights, b['rig'], b['pb'].n_frames, precision)
        try:
            persons = None if precision_key is None else _fresh(calib, gat_weights, mlp_weights, name)['persons']
            _expected[key] = _run(eng, b['pb'], persons=persons, name=name)
        finally:
            eng.close()
    return _expected[key]


@pytest.mark.parametrize('name', ['A18', 'S3', 'C17', 'P18', 'T17'])
def test_a_fresh_engines_bits_are_the_oracles(calib, gat_weights, mlp_weights, name):
    """The yardstick of Test B is RIGHT, not only history-free: on the clean batches the edge-node scores against the oracle's fp32
    scores (2e-5, test_gat_scores_vs_golden's bound) and the MLP input rows of the frames whose persons are the oracle's against the
    oracle's rows (3e-7, test_ring23_full_shape_frame_vs_oracle's bound)."""
    onp = oracle()
    sd, prm = gat_weights
    b = nc.batch(calib, name)
    w = _fresh(calib, gat_weights, mlp_weights, name)
    pb = b['pb']
    scored = rows_used = 0
    for f, frame in enumerate(b['frames']):
        h0, H, e0, M = pb.frame_counts(f)
        res = onp.run_frame(frame, calib, sd, prm, mlp_weights, mode='mlp')
        if res is None:
            assert M == 0 and int(w['persons'][1][f]) == 0
            continue
        assert np.abs(w['scores'][e0:e0 + M] - res['scores']).max() < 2e-5, f
        assert np.abs(w['scores_fwd'][e0:e0 + M] - res['scores']).max() < 2e-5, f
        scored += 1
        want = np.array(res['persons'], np.int32).reshape(-1, pb.V)
        n = int(w['persons'][1][f])
        if n == 0 or n != len(want) or not np.array_equal(w['persons'][0][f, :n], want) or len(res['mlp_in']) != n:
            continue
        assert w['rows'][1][f, :n].all()
        np.testing.assert_allclose(w['rows'][0][f, :n], res['mlp_in'].numpy(), rtol=0, atol=3e-7)
        rows_used += 1
    assert scored >= pb.n_frames - 1 and rows_used >= pb.n_frames // 2, (scored, rows_used)


# ---- A: isolation in space ------------------------------------------------------------------------------------------------------
_clean = {}


def _clean_run(engines, calib, route, monkeypatch):
    """The clean batch of `route` on the route's engine with the route's environment (set by the caller), computed once."""
    name, envs, l0 = ROUTES[route]
    b = nc.batch(calib, name)
    for k, v in envs.items():
        monkeypatch.setenv(k, v)
    eng = engines(b['rig'])
    if route not in _clean:
        _clean[route] = _run(eng, b['pb'])
        if l0 is not None:
            assert _clean[route]['l0_launches'] == l0, (route, _clean[route]['l0_launches'])
    return eng, b, _clean[route]


@pytest.mark.parametrize('position', ['first', 'middle'])
@pytest.mark.parametrize('route', list(ROUTES))
@pytest.mark.parametrize('kind', nc.KINDS)
def test_A_one_bad_detection_stays_in_its_frame(engines, calib, kind, route, position, monkeypatch):
    """One frame of the batch poisoned, on a head that the clean batch's match put into a person; every call of the two stages.
    Every other frame: no bit moves.  The poisoned frame: MPE_OK, no status bit, structurally valid person tables; its other
    persons keep their 3D bits; the poisoned person's row flag is what the reference's sum(|row|) > 1 says on the oracle's row.
    masked_nan (NaN under a cleared mask bit): the whole batch keeps its bits."""
    eng, b, clean = _clean_run(engines, calib, route, monkeypatch)
    pb = b['pb']
    f = nc.POSITIONS[b['name']][position == 'middle']
    if position == 'middle':
        # its node rows share a 16-row GEMM tile with both neighbours; 5 x 4: and a frame slab of the attention launches
        assert nc.shares_tiles_with_both_neighbours(pb, f), (b['name'], f)
    lh = _member_head(clean, f)
    bad = nc.poison(pb, f, kind, head=lh)
    got = _run(eng, bad, persons=clean['persons'])
    if ROUTES[route][2] is not None:
        assert got['l0_launches'] == ROUTES[route][2]
    what = '%s, %s in frame %d' % (route, kind, f)
    if kind == 'masked_nan':
        _compare(got, clean, pb, range(pb.n_frames), what)
        return
    assert bad.poisoned['head'] == lh
    h0, H, e0, M = pb.frame_counts(f)
    assert not _same(got['layer0'][h0 + e0:h0 + e0 + H + M], clean['layer0'][h0 + e0:h0 + e0 + H + M]), what + ': the poison reached nothing'
    _compare(got, clean, pb, [g for g in range(pb.n_frames) if g != f], what)
    _compare(got, clean, pb, [f], what + ' (its other persons)', skip_head=(f, lh), parts=('3d',))
    for key in ('persons', 'geom_persons'):
        fault = nc.structural_fault(got[key][0], got[key][1], pb, f, eng.pcap)
        assert fault is None, '%s: %s: %s' % (what, key, fault)
    table, n = clean['persons']
    slots = [p for p in range(int(n[f])) if lh in table[f, p]]
    assert len(slots) == 1
    row, kept = nc.oracle_person_row(nc.poisoned_frame(b['frames'], bad, calib), table[f, slots[0]], calib)
    assert int(got['mlp'][1][f, slots[0]]) == int(kept), '%s: mlp3d flag %d, the reference keeps the row: %s' % (what, got['mlp'][1][f, slots[0]], kept)
    assert int(got['rows'][1][f, slots[0]]) == int(kept), '%s: row flag %d, the reference keeps the row: %s' % (what, got['rows'][1][f, slots[0]], kept)


# ---- B: recovery in time ---------------------------------------------------------------------------------------------------------
@pytest.fixture(scope='module')
def veteran(calib, gat_weights, mlp_weights):
    """ONE long-lived 5 x 4 engine for every schedule of Test B, in file order."""
    eng = _engine(calib, gat_weights, mlp_weights, 4, 18)
    yield eng
    eng.close()


def _step_batch(calib, gat_weights, mlp_weights, name, bad_frames):
    """(PackedBatch of the step, persons for its 3D calls, expected bits or None): a poisoned step takes the clean batch's persons, so
    that the poisoned heads are members of persons and the MLP workspaces really receive non-finite rows."""
    w = _fresh(calib, gat_weights, mlp_weights, name)
    pb = nc.batch(calib, name)['pb']
    if not bad_frames:
        return pb, None, w
    heads = {f: _member_head(w, f) for f in bad_frames}
    return nc.poison_more(pb, bad_frames, 'xy_nan', heads=heads), w['persons'], None


def _walk(eng, calib, gat_weights, mlp_weights, schedule, what, layer_first=False):
    for i, (name, bad_frames) in enumerate(schedule):
        pb, persons, want = _step_batch(calib, gat_weights, mlp_weights, name, bad_frames)
        got = _run(eng, pb, persons=persons, name=name, layer_first=layer_first)
        if want is None:
            assert not np.isfinite(got['scores']).all() and not np.isfinite(got['rows'][0]).all(), '%s: step %d poisons nothing' % (what, i)
            assert not np.isfinite(got['layer0']).all()
        else:
            _compare(got, want, pb, range(pb.n_frames), '%s, step %d (%s)' % (what, i, name))


@pytest.mark.parametrize('first_call', ['match', 'gat_layer'])
@pytest.mark.parametrize('schedule', [1, 2])
def test_B_clean_batches_after_a_poisoned_one(veteran, calib, gat_weights, mlp_weights, schedule, first_call):
    """1: A (18 frames), P (18 full frames, two of them with a NaN: at least as many nodes as anything later), A, B (3 frames: the
    small-batch route), C (17 frames of another layout).  2: the same with P on the small-batch route (3 frames, all poisoned).
    first_call: what a batch's first call is -- mpe_match_batch (production), or mpe_gat_layer with 150-wide caller rows of the last
    layer, which copy_rows_in lays over the 400-wide layer-0 rows the batch before left in act[0].  (With copy_rows_in's clear of the
    pad columns taken out, the gat_layer variants fail at step 2 of both schedules: NaN rows where P's poisoned frames were.)"""
    _walk(veteran, calib, gat_weights, mlp_weights, nc.SCHEDULES[schedule], 'schedule %d, %s first' % (schedule, first_call),
          layer_first=first_call == 'gat_layer')


@pytest.mark.parametrize('mode', list(nc.GAT_MODES))
def test_B_precision_modes_of_the_matching_stage(veteran, calib, gat_weights, mlp_weights, mode):
    """3. The mode is set, P is run, A is run (against a fresh engine in the same mode), the mode is set back -- and A once more."""
    prec = nc.GAT_MODES[mode]
    (pname, bad_frames), (aname, _) = nc.SCHEDULES[3]
    want = _fresh(calib, gat_weights, mlp_weights, aname, mode, prec)
    a = nc.batch(calib, aname)['pb']
    try:
        veteran.set_precision(**prec)
        pb, persons, _ = _step_batch(calib, gat_weights, mlp_weights, pname, bad_frames)
        got = _run(veteran, pb, persons=persons, name=pname)
        assert not np.isfinite(got['scores']).all()
        _compare(_run(veteran, a, persons=want['persons_3d'], name=aname), want, a, range(a.n_frames), 'schedule 3, %s' % mode)
    finally:
        veteran.set_precision()
    _walk(veteran, calib, gat_weights, mlp_weights, [(aname, ())], 'schedule 3, back from %s' % mode)


def _mlp3d(eng, pb, persons):
    db = eng.to_device(pb)
    out = tuple(_np(t) for t in eng.mlp3d(db, torch.from_numpy(persons[0]).to(eng.device), torch.from_numpy(persons[1]).to(eng.device)))
    eng.sync_status()
    return out


def _same_poses(got, want, what):
    assert np.array_equal(got[1], want[1]), '%s: flags' % what
    sel = want[1] != 0
    assert _same(got[0][sel], want[0][sel]), '%s: poses' % what


@pytest.mark.parametrize('mode', list(nc.MLP_MODES))
def test_B_precision_modes_of_the_mlp(veteran, calib, gat_weights, mlp_weights, mode):
    """3. MLP modes 0 .. 5: mlp3d on P's persons (NaN rows in mlp_rows and mlp_act), then on A, against a fresh engine in the mode."""
    prec = nc.MLP_MODES[mode]
    (pname, bad_frames), (aname, _) = nc.SCHEDULES[3]
    want = _fresh(calib, gat_weights, mlp_weights, aname, ('mlp', mode), prec)
    a = nc.batch(calib, aname)['pb']
    try:
        veteran.set_precision(**prec)
        pb, persons, _ = _step_batch(calib, gat_weights, mlp_weights, pname, bad_frames)
        poses, flags = _mlp3d(veteran, pb, persons)
        assert not np.isfinite(poses).all()
        _same_poses(_mlp3d(veteran, a, want['persons_3d']), want['mlp'], 'schedule 3, MLP mode %d' % mode)
    finally:
        veteran.set_precision()


def test_B_mlp_rows_after_nan_rows_with_more_and_fewer_persons(veteran, calib, gat_weights, mlp_weights):
    """4. mlp3d alone: a batch with NaN rows, then a clean batch with MORE persons (its compact rows cover the NaN rows and go
    beyond), then one with FEWER (the NaN rows' places lie behind its last row, inside its last tile)."""
    (pname, bad_frames), (more, _), (fewer, _) = nc.SCHEDULES[4]
    pb, persons, _ = _step_batch(calib, gat_weights, mlp_weights, pname, bad_frames)
    counts = [int(_fresh(calib, gat_weights, mlp_weights, n)['persons'][1].sum()) for n in (pname, more, fewer)]
    assert counts[1] > counts[0] > counts[2] > 0, counts
    poses, flags = _mlp3d(veteran, pb, persons)
    assert not np.isfinite(poses).all()
    for name in (more, fewer, more):
        want = _fresh(calib, gat_weights, mlp_weights, name)
        _same_poses(_mlp3d(veteran, nc.batch(calib, name)['pb'], want['persons']), want['mlp'], 'schedule 4, %s' % name)


class _Slot:
    """One arena as the production hosts keep it (test_gpu_history.py): a device BatchArena laid out for the largest batch and ONE
    DeviceBatch bound to it; a batch arrives with rebind + upload, at the addresses the batch before it had."""

    def __init__(self, eng, template):
        packing = pkg('packing')
        self.packing, self.template = packing, template
        self.db = packing.DeviceBatch(template, eng.device, arena=packing.BatchArena(template, eng.device))
        self.pinned = []

    def load(self, pb):
        ar = self.packing.BatchArena(self.template, 'pinned')
        host = ar.buf.numpy()
        host[:] = 0
        for name, (off, n, dt) in ar.offsets.items():
            src = np.ascontiguousarray(getattr(pb, name)).reshape(-1).view(dt)
            assert src.size <= n, name
            host[off: off + src.nbytes].view(dt)[:] = src
        self.pinned.append(ar)                                             # (stays alive while its copy is in flight)
        self.db.rebind(pb)
        self.db.upload(ar)
        return self.db


def test_B_the_production_ring(veteran, calib, gat_weights, mlp_weights):
    """5. [A, P, A, B] on a sibling context, then through run_pipelined over two arenas with one context and with two."""
    steps = nc.SCHEDULES[5]
    sib = veteran.sibling(1)
    _walk(sib, calib, gat_weights, mlp_weights, steps, 'schedule 5, sibling context')
    sib.sync_status()
    batches = [_step_batch(calib, gat_weights, mlp_weights, name, bad) for name, bad in steps]
    template = nc.batch(calib, 'P18')['pb']
    for contexts in (1, 2):
        slots = [_Slot(veteran, template), _Slot(veteran, template)]
        feed = (slots[i % 2].load(pb) for i, (pb, _, _) in enumerate(batches))
        seen = 0
        for (pb, _, want), (poses, n_persons, persons, _) in zip(batches, veteran.run_pipelined(feed, contexts=contexts)):
            what = 'schedule 5, run_pipelined(contexts=%d), window %d' % (contexts, seen)
            if want is not None:
                n = _np(n_persons)
                assert np.array_equal(n, want['persons'][1]), what
                for f in range(pb.n_frames):
                    assert np.array_equal(_np(persons)[f, :n[f]], want['persons'][0][f, :n[f]]), what
                sel = want['mlp'][1] != 0
                assert _same(_np(poses)[sel], want['mlp'][0][sel]), what
            else:
                for f in range(pb.n_frames):
                    assert nc.structurally_valid(_np(persons), _np(n_persons), pb, f, veteran.pcap), what
            seen += 1
        assert seen == len(batches)
        veteran.sync_status()


# ---- C: the wire format ---------------------------------------------------------------------------------------------------------
def test_C_a_document_with_1e39_in_its_middle_frame(engines, calib):
    """1e39 is a legal JSON number, finite as a double and infinite as a float.  The device parser converts it itself (1 x 10^39 lies
    inside the exact range of el_double.h, 10^-27 .. 10^55 -- the window does NOT fall back to the host packer, as was supposed), and
    the packed xy holds float('1e39'); 1e60 lies outside, the device declines it and the window goes through the host packer's
    strtod.  Either way the outer frames' poses are those of the same document with an ordinary pixel in that place."""
    eng = engines(4)
    b = nc.batch(calib, 'S3')
    bad = nc.poison(b['pb'], 1, 'xy_f32_overflow')
    h = int(b['pb'].frame_head_off[1]) + bad.poisoned['head']
    docs = {}
    for key, value in (('1e39', 1e39), ('1e60', 1e60), ('plain', 640.25)):
        raw = [dict(f) for f in b['raw']]
        bad.poisoned['writes'] = [('xy', 0, value)]
        raw[1] = nc.poisoned_frame(b['raw'], bad, calib)
        docs[key] = json.dumps(raw)
    assert '1e+39' in docs['1e39'] and '1e+60' in docs['1e60'] and 'e+' not in docs['plain']
    got = {}
    for key, text in docs.items():
        windows = []
        for info, poses, n in eng.stream_json(text, chunk_frames=3, parser='device'):
            host = info if type(info).__name__ == 'PackedBatch' else info.download()
            windows.append((type(info).__name__, poses.copy(), n.copy(), float(host.xy[h, bad.poisoned['joint'], 0])))
        assert len(windows) == 1
        got[key] = windows[0]
    eng.sync_status()
    assert [got[k][0] for k in ('1e39', '1e60', 'plain')] == ['ParsedOnDevice', 'PackedBatch', 'ParsedOnDevice']
    assert got['1e39'][3] == float('1e39') and got['1e60'][3] == float('1e60') and got['plain'][3] == 640.25
    for key in ('1e39', '1e60'):
        for f in (0, 2):
            n = int(got['plain'][2][f])
            assert n >= 1 and int(got[key][2][f]) == n, (key, f)
            assert _same(got[key][1][f, :n], got['plain'][1][f, :n]), (key, f)
        assert 0 <= int(got[key][2][1]) <= eng.pcap


# ---- D: large but finite --------------------------------------------------------------------------------------------------------
_report = {}


@pytest.mark.parametrize('position', ['first', 'middle'])
@pytest.mark.parametrize('route', list(ROUTES))
def test_D_a_joint_at_1e38_pixels(engines, calib, gat_weights, route, position, monkeypatch):
    """x = LARGE_FINITE_M on one joint: the reference's fp32 network stays finite (its softmax subtracts the maximum), so the device's
    must; and its scores sit no further from the oracle's float64 network than MARGIN times the reference's own fp32 scores do
    (e_gpu <= 2.5 * max(e_ref, 2e-6): test_score_noise_against_the_f64_network's arithmetic, on the same launches).  The other frames
    keep their bits.  Figures: nonfinite_isolation.json in the report directory (MPE_REPORT_DIR, default reports/ in the tree).
    Measured on an MI355X: finite on all six routes; ratio 0.11 on the 3-frame batch's first frame (e_ref 9.3e-7, e_gpu 2.2e-7), 0 elsewhere
    (the scores saturate and both distances are 0): DESIGN.md 5.1."""
    eng, b, clean = _clean_run(engines, calib, route, monkeypatch)
    pb = b['pb']
    f = nc.POSITIONS[b['name']][position == 'middle']
    bad = nc.poison(pb, f, 'large_finite', head=_member_head(clean, f))
    db = eng.to_device(bad)
    sc, sh = eng.gat_scores(db, heads=True)
    eng.sync_status()
    sc, sh = _np(sc), _np(sh)
    h0, H, e0, M = pb.frame_counts(f)
    gpu = np.concatenate([sh[h0:h0 + H], sc[e0:e0 + M]])
    frame = nc.poisoned_frame(b['frames'], bad, calib)
    exact = nc.oracle_scores(frame, calib, gat_weights, f64=True)[1]
    ref = nc.oracle_scores(frame, calib, gat_weights)[1]
    assert np.isfinite(ref).all() and np.isfinite(exact).all()
    finite = bool(np.isfinite(gpu).all())
    e_ref = float(np.abs(ref - exact).max())
    e_gpu = float(np.abs(gpu - exact).max()) if finite else float('inf')
    ratio = e_gpu / max(e_ref, FLOOR)
    _report['%s/%s' % (route, position)] = {'batch': b['name'], 'frame': f, 'M': nc.LARGE_FINITE_M, 'device_finite': finite, 'e_ref': e_ref,
                                           'e_gpu': e_gpu if finite else None, 'ratio': ratio if finite else None}
    out = os.environ.get('MPE_REPORT_DIR') or os.path.join(ROOT, 'reports')
    os.makedirs(out, exist_ok=True)
    with open(os.path.join(out, 'nonfinite_isolation.json'), 'w') as fh:
        json.dump(_report, fh, indent=1)
    print(json.dumps({route + '/' + position: _report['%s/%s' % (route, position)]}))
    for g in range(pb.n_frames):
        if g != f:
            g0, GH, ge0, GM = pb.frame_counts(g)
            assert _same(sc[ge0:ge0 + GM], clean['scores_fwd'][ge0:ge0 + GM]), g
            if GM:
                assert _same(sh[g0:g0 + GH], clean['head_scores'][g0:g0 + GH]), g
    assert finite, 'device scores of the poisoned frame are not finite'
    assert e_gpu <= MARGIN * max(e_ref, FLOOR), (e_gpu, e_ref, ratio)
