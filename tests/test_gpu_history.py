"""One rule, for everything a context keeps between calls (workspaces, the sticky status word, the pair solves mpe_match_batch leaves
for mpe_mlp3d_batch): the output of a call is a function of the CONTENTS of its arguments, not of what the context did before.

The production hosts reuse device addresses on purpose (capacity arenas, DeviceBatch.upload / rebind, fixed staging buffers), and
batches of equal counts are the normal case on a fixed rig: Panoptic frames [s, s+1, s+2] of four persons pack to 60 heads and 480
edge-nodes for s = 500, 700, 800, 900, 1000 with different pixels in each.  So every scenario here puts a second batch of the same
counts where a first one was, takes some route to its persons and poses, and asks for the bits of the same calls on a context that
has no history to speak of: MPE_LATENCY_PATH=0 (no hand-off exists on that route), every batch in device arrays of its own that stay
allocated (no address is shared).  That yardstick is itself held to the oracle once.  A seeded schedule of calls at the end is the net
for the next piece of cross-call state.  tests/native/pair_handoff_test.cpp walks the same scenarios through the hand-off's
bookkeeping alone, on the host."""
import json

import numpy as np
import pytest
import torch

from conftest import oracle, pkg

pytestmark = pytest.mark.gpu

STARTS = {'A': 500, 'B': 700, 'C': 800, 'D': 900, 'E': 1000, 'G': 600}      # G: the control, 59 heads / 464 edge-nodes
KINDS = ('gat', 'geo')                                                       # whose persons: mpe_match_batch's, mpe_geom_match_batch's


def _raw(calib, start, persons=(4, 4, 4)):
    syn = pkg('synthetic')
    return [syn.make_frame(calib, start + i, syn.FrameSpec(persons=p))[0] for i, p in enumerate(persons)]


def _mixed(calib, n, start):
    """n frames of mixed shape (1 ... 6 persons, dropped joints, an empty camera now and then) for the batches of 1, 16 and 17 frames."""
    syn = pkg('synthetic')
    persons = (4, 2, 5, 1, 3, 4, 6, 4)
    return [syn.make_frame(calib, start + i, syn.FrameSpec(persons=persons[i % 8], empty_cameras=('trackerc',) if i % 5 == 3 else (),
                                                         joint_drop=0.15 if i % 2 else 0.0))[0] for i in range(n)]


def _np(t):
    return t.cpu().numpy()


def _expect(eng, calib, raw):
    """The bits of every call of this file on one batch, from a batch in arrays of its own (kept: 'db').  The caller has switched
    the small-batch route off."""
    import os
    assert os.environ.get('MPE_LATENCY_PATH') == '0'
    frames = [oracle().processed_input(f) for f in raw]
    pb = eng.pack(frames)
    db = eng.to_device(pb)
    w = {'raw': raw, 'frames': frames, 'pb': pb, 'db': db}
    _, p, n = eng.match(db)
    _, pg, ng = eng.geom_match(db)
    pc, nc = eng.cluster(db, eng.gat_scores(db))
    w['gat'], w['geo'] = (_np(p), _np(n)), (_np(pg), _np(ng))
    _same_persons((pc, nc), w['gat'], 'gat_scores + cluster against match, both without history')
    for kind, (pp, nn) in (('gat', (p, n)), ('geo', (pg, ng))):
        w['mlp', kind] = tuple(_np(t) for t in eng.mlp3d(db, pp, nn))
        w['tri', kind] = tuple(_np(t) for t in eng.triangulate(db, pp, nn))
        w['rows', kind] = tuple(_np(t) for t in eng.mlp_input_rows(db, pp, nn))
    eng.sync_status()
    return w


def _same_persons(got, want, what):
    p, n = _np(got[0]), _np(got[1])
    assert np.array_equal(n, want[1]), '%s: persons per frame %s, expected %s' % (what, n.tolist(), want[1].tolist())
    for f in range(len(n)):
        assert np.array_equal(p[f, :n[f]], want[0][f, :n[f]]), '%s: persons of frame %d' % (what, f)


def _same_rows(got, want, what):
    """(values, flags) of mlp3d / triangulate / mlp_input_rows: the flags, and the values under them, bit for bit."""
    v, m = _np(got[0]), _np(got[1])
    assert np.array_equal(m, want[1]), '%s: validity flags differ' % what
    sel = want[1] != 0
    if not np.array_equal(v[sel], want[0][sel]):
        d = np.abs(v[sel].astype(np.float64) - want[0][sel].astype(np.float64))
        raise AssertionError('%s: %d of %d kept values differ, by up to %.6g (poses: metres)' % (what, int((d != 0).sum()), d.size, float(np.nanmax(d))))


def _device_persons(eng, w, kind):
    """The expected persons of a batch from the host, in fresh tensors."""
    return torch.from_numpy(w[kind][0]).to(eng.device), torch.from_numpy(w[kind][1]).to(eng.device)


def _twins(a, b, equal_counts=True):
    """What a scenario relies on: two batches of the same counts (or, for the control, not) and different pixels."""
    pa, pb = a['pb'], b['pb']
    assert pa.n_frames == pb.n_frames
    assert ((pa.n_heads, pa.n_edge_nodes) == (pb.n_heads, pb.n_edge_nodes)) == equal_counts, (pa.n_heads, pa.n_edge_nodes, pb.n_heads, pb.n_edge_nodes)
    if equal_counts:
        assert not np.array_equal(pa.xy, pb.xy) and not np.array_equal(a['mlp', 'gat'][0], b['mlp', 'gat'][0])


def _pinned_like(template, pb):
    """pb in a page-locked BatchArena laid out for `template` (a batch with at least as many heads: the control has one fewer)."""
    packing = pkg('packing')
    ar = packing.BatchArena(template, 'pinned')
    host = ar.buf.numpy()
    host[:] = 0
    for name, (off, n, dt) in ar.offsets.items():
        src = np.ascontiguousarray(getattr(pb, name)).reshape(-1).view(dt)
        assert src.size <= n, name
        host[off: off + src.nbytes].view(dt)[:] = src
    return ar


class _Slot:
    """One arena as the production hosts keep it: a device BatchArena and ONE DeviceBatch bound to it; a batch arrives with
    rebind + upload, at the addresses the batch before it had."""

    def __init__(self, eng, template):
        packing = pkg('packing')
        self.template = template
        self.db = packing.DeviceBatch(template, eng.device, arena=packing.BatchArena(template, eng.device))
        self.d_xy = self.db.struct.d_xy
        self.holds = None

    def load(self, w):
        if ('pinned', id(self.template)) not in w:
            w['pinned', id(self.template)] = _pinned_like(self.template, w['pb'])
        self.db.rebind(w['pb'])
        self.db.upload(w['pinned', id(self.template)])
        assert self.db.struct.d_xy == self.d_xy == self.db.arena.ptr('xy')      # the same arrays as whatever was here before
        self.holds = w
        return self.db


@pytest.fixture(scope='module')
def engine(calib, gat_weights, mlp_weights):
    eng = pkg('pipeline').Engine(calib.params, calib, max_frames=16, max_persons_per_camera=10)
    sd, prm = gat_weights
    eng.load_gat(sd, prm)
    eng.load_mlp(mlp_weights)
    yield eng
    eng.close()


def _layout(calib, start, heads):
    """First index >= start from which three clean frames of heads // 5 persons each pack to exactly `heads` heads per frame."""
    packing = pkg('packing')
    persons = tuple(h // 5 for h in heads)
    for s in range(start, start + 50):
        raw = _raw(calib, s, persons)
        pb = packing.pack_frames([oracle().processed_input(f) for f in raw], calib.params)
        if tuple(np.diff(pb.frame_head_off)) == tuple(heads):
            return raw
    raise AssertionError('no frames of layout %s from %d on' % (heads, start))


@pytest.fixture(scope='module')
def world(engine, calib):
    """Expected bits of every batch of the named scenarios, computed once and left alone."""
    with pytest.MonkeyPatch.context() as mp:
        mp.setenv('MPE_LATENCY_PATH', '0')
        w = {name: _expect(engine, calib, _raw(calib, s)) for name, s in STARTS.items()}
        w['hA'] = _expect(engine, calib, _layout(calib, 500, (25, 15, 20)))
        w['hB'] = _expect(engine, calib, _layout(calib, 700, (15, 25, 20)))
    return w


@pytest.fixture(autouse=True)
def _small_batch_route_on(monkeypatch):
    monkeypatch.delenv('MPE_LATENCY_PATH', raising=False)


def _third_stage(eng, db, persons, n_persons, w, kind, what):
    """mlp3d, triangulate and mlp_input_rows of a batch against its expected bits (mlp3d first: it is the one with a memory)."""
    _same_rows(eng.mlp3d(db, persons, n_persons), w['mlp', kind], what + ': mlp3d')
    _same_rows(eng.triangulate(db, persons, n_persons), w['tri', kind], what + ': triangulate')
    _same_rows(eng.mlp_input_rows(db, persons, n_persons), w['rows', kind], what + ': mlp_input_rows')


def test_the_yardstick_is_the_oracles(engine, world, calib, gat_weights, mlp_weights):
    """The expected bits are history-free by construction; here they are also RIGHT: the MLP input rows of batch A's GAT-matched
    persons against the oracle's, on the frames whose persons are the oracle's, to the bound test_ring23_full_shape_frame_vs_oracle
    uses (3e-7).  Pairs of another batch move these rows by centimetres to metres."""
    onp = oracle()
    sd, prm = gat_weights
    w = world['A']
    used = 0
    for f, frame in enumerate(w['frames']):
        res = onp.run_frame(frame, calib, sd, prm, mlp_weights, mode='mlp')
        want = np.array(res['persons'], np.int32).reshape(-1, engine.V)
        n = int(w['gat'][1][f])
        if n == 0 or n != len(want) or not np.array_equal(w['gat'][0][f, :n], want):
            continue
        assert w['rows', 'gat'][1][f, :n].all()
        np.testing.assert_allclose(w['rows', 'gat'][0][f, :n], res['mlp_in'].numpy(), rtol=0, atol=3e-7)
        used += 1
    assert used >= 1, 'no frame of batch A has the oracle\'s persons'


def test_a_geom_match_of_a_batch_uploaded_over_a_matched_one(engine, world):
    """a. match(A); B uploaded into the same arena; geom_match(B); mlp3d(B)."""
    A, B = world['A'], world['B']
    _twins(A, B)
    slot = _Slot(engine, A['pb'])
    _same_persons(engine.match(slot.load(A))[1:], A['gat'], 'match(A)')
    db = slot.load(B)
    _, p, n = engine.geom_match(db)
    _same_persons((p, n), B['geo'], 'geom_match(B)')
    _third_stage(engine, db, p, n, B, 'geo', 'B over A')
    engine.sync_status()


def test_b_scores_and_clustering_of_a_batch_uploaded_over_a_matched_one(engine, world):
    """b. match(A); B uploaded into the same arena; gat_scores(B) + cluster(B); mlp3d(B)."""
    A, B = world['A'], world['B']
    _twins(A, B)
    slot = _Slot(engine, A['pb'])
    _same_persons(engine.match(slot.load(A))[1:], A['gat'], 'match(A)')
    db = slot.load(B)
    p, n = engine.cluster(db, engine.gat_scores(db))
    _same_persons((p, n), B['gat'], 'gat_scores + cluster (B)')
    _third_stage(engine, db, p, n, B, 'gat', 'B over A')
    engine.sync_status()


@pytest.mark.parametrize('kind', KINDS)
def test_c_no_call_between_the_upload_and_the_mlp_stage(engine, world, kind):
    """c. match(A); B uploaded; B's persons from the host in fresh tensors (the allocator may hand out the addresses of the ones
    match wrote, freed here on purpose); mlp3d(B) with no other call between."""
    A, B = world['A'], world['B']
    _twins(A, B)
    slot = _Slot(engine, A['pb'])
    got = engine.match(slot.load(A), want_scores=False)
    _same_persons(got[1:], A['gat'], 'match(A)')
    del got
    db = slot.load(B)
    p, n = _device_persons(engine, B, kind)
    _third_stage(engine, db, p, n, B, kind, 'B over A, persons from the host')
    engine.sync_status()


def test_d_a_batch_copied_in_place_without_an_arena(engine, world):
    """d. No arena: B's bytes copied over A's in A's own buffer (DeviceBatch.buf.copy_ + rebind); then as a."""
    A, B = world['A'], world['B']
    _twins(A, B)
    db = engine.to_device(A['pb'])
    d_xy = db.struct.d_xy
    _same_persons(engine.match(db)[1:], A['gat'], 'match(A)')
    assert db.buf.numel() == B['db'].buf.numel()
    db.buf.copy_(B['db'].buf)
    db.rebind(B['pb'])
    assert db.struct.d_xy == d_xy
    _, p, n = engine.geom_match(db)
    _same_persons((p, n), B['geo'], 'geom_match(B)')
    _third_stage(engine, db, p, n, B, 'geo', 'B copied over A')
    engine.sync_status()


@pytest.mark.parametrize('order', [(0, 1), (1, 0)])
def test_e_both_ring_slots(engine, world, order):
    """e. Two arenas: match(A) in arena 0, match(B) in arena 1 (both pair buffers written); C uploaded into arena 0, D into arena 1;
    geom_match + mlp3d on both, in both orders."""
    A, B, C, D = (world[k] for k in 'ABCD')
    for x in (B, C, D):
        _twins(A, x)
    _twins(B, D)
    slots = [_Slot(engine, A['pb']), _Slot(engine, A['pb'])]
    _same_persons(engine.match(slots[0].load(A))[1:], A['gat'], 'match(A)')
    _same_persons(engine.match(slots[1].load(B))[1:], B['gat'], 'match(B)')
    slots[0].load(C)
    slots[1].load(D)
    for r in order:
        db, w = slots[r].db, slots[r].holds
        _, p, n = engine.geom_match(db)
        _same_persons((p, n), w['geo'], 'geom_match in arena %d' % r)
        _third_stage(engine, db, p, n, w, 'geo', 'arena %d' % r)
    engine.sync_status()


def test_f_what_does_not_change_the_data_changes_no_result(engine, world):
    """f. match(A), geom_match(A), mlp3d(A, geometric persons), mlp3d(A, GAT persons): whether or not the hand-off survives calls
    that leave the data alone, the bits are the expected ones (that the plain match -> mlp3d still fetches is a matter of time, not
    of bits: tools/pair_handoff_time.py, profiles/pair_handoff_timing.txt)."""
    A = world['A']
    slot = _Slot(engine, A['pb'])
    db = slot.load(A)
    _, p, n = engine.match(db)
    _same_persons((p, n), A['gat'], 'match(A)')
    _, pg, ng = engine.geom_match(db)
    _same_persons((pg, ng), A['geo'], 'geom_match(A)')
    _same_rows(engine.mlp3d(db, pg, ng), A['mlp', 'geo'], 'mlp3d(A, geometric persons)')
    _same_rows(engine.mlp3d(db, p, n), A['mlp', 'gat'], 'mlp3d(A, GAT persons)')
    _, p, n = engine.match(db)
    _third_stage(engine, db, p, n, A, 'gat', 'match(A); the third stage')
    _same_rows(engine.mlp3d(db, p, n), A['mlp', 'gat'], 'mlp3d(A) a second time')
    engine.sync_status()


def test_g_control_a_batch_of_other_counts(engine, world):
    """g. match(A); the s = 600 batch (59 heads, 464 edge-nodes) uploaded; geom_match + mlp3d."""
    A, G = world['A'], world['G']
    _twins(A, G, equal_counts=False)
    slot = _Slot(engine, A['pb'])
    _same_persons(engine.match(slot.load(A))[1:], A['gat'], 'match(A)')
    db = slot.load(G)
    _, p, n = engine.geom_match(db)
    _same_persons((p, n), G['geo'], 'geom_match(G)')
    _third_stage(engine, db, p, n, G, 'geo', 'G over A')
    engine.sync_status()


def test_h_equal_totals_in_another_layout(engine, world):
    """h. (25, 15, 20) heads per frame, then (15, 25, 20) in the same arrays: 60 heads and 500 edge-nodes both.  An index into another
    layout's pair solves stays inside the buffer (a global head < n_heads, a local head < max_heads_per_frame): wrong bits, no fault."""
    A, B = world['hA'], world['hB']
    _twins(A, B)
    assert tuple(np.diff(A['pb'].frame_head_off)) == (25, 15, 20) and tuple(np.diff(B['pb'].frame_head_off)) == (15, 25, 20)
    assert A['pb'].n_heads == 60 and A['pb'].n_edge_nodes == 500 and max(25, 15, 20) <= engine.hpf
    slot = _Slot(engine, A['pb'])
    _same_persons(engine.match(slot.load(A))[1:], A['gat'], 'match(A)')
    db = slot.load(B)
    _, p, n = engine.geom_match(db)
    _same_persons((p, n), B['geo'], 'geom_match(B)')
    _third_stage(engine, db, p, n, B, 'geo', 'B over A')
    engine.sync_status()


def test_i_sibling_contexts(engine, world):
    """i. match(A) on context 0; mlp3d on context 1 (Engine.sibling), for A itself and for B in A's arena."""
    A, B = world['A'], world['B']
    _twins(A, B)
    sib = engine.sibling(1)
    slot = _Slot(engine, A['pb'])
    db = slot.load(A)
    _, p, n = engine.match(db)
    _same_persons((p, n), A['gat'], 'match(A)')
    _same_rows(sib.mlp3d(db, p, n), A['mlp', 'gat'], 'mlp3d(A) on the sibling')
    db = slot.load(B)
    pb_, nb_ = _device_persons(engine, B, 'gat')
    _same_rows(sib.mlp3d(db, pb_, nb_), B['mlp', 'gat'], 'mlp3d(B over A) on the sibling')
    engine.sync_status()
    sib.sync_status()


def _ring(slots, wants):
    """The production feed of run_pipelined: batch i uploaded into arena i % 2 when the pipeline asks for it."""
    for i, w in enumerate(wants):
        yield slots[i % 2].load(w)


def test_j_run_pipelined_over_a_ring_of_arenas(engine, world):
    """j. run_pipelined with the GAT over one recording, then with the geometric matcher over a second one whose windows have the
    same counts, through the same two arenas on the same engine."""
    first, second = [world[k] for k in 'ABCD'], [world[k] for k in 'EABC']
    for a, b in zip(first, second):
        _twins(a, b)
    slots = [_Slot(engine, world['A']['pb']), _Slot(engine, world['A']['pb'])]
    for matcher, kind, wants in (('gat', 'gat', first), ('geometric', 'geo', second)):
        got = 0
        for w, (poses, n_persons, persons, _) in zip(wants, engine.run_pipelined(_ring(slots, wants), matcher=matcher)):
            what = 'run_pipelined(%s), window %d' % (matcher, got)
            _same_persons((persons, n_persons), w[kind], what)
            _same_rows((poses, torch.from_numpy(w['mlp', kind][1])), w['mlp', kind], what)
            got += 1
        assert got == len(wants)
    engine.sync_status()


@pytest.mark.parametrize('parser', ['device', 'host'])
def test_j_stream_json_twice_on_one_engine(engine, world, parser):
    """j. stream_json in windows of three frames with the GAT, then with the geometric matcher over a second recording of equal
    window counts on the same engine (its arenas are the engine's, or reused by its allocator)."""
    first, second = [world[k] for k in 'ABCD'], [world[k] for k in 'EABC']
    for matcher, kind, wants in (('gat', 'gat', first), ('geometric', 'geo', second)):
        text = json.dumps([f for w in wants for f in w['raw']]).encode()
        got = 0
        for info, poses, n_persons in engine.stream_json(text, chunk_frames=3, parser=parser, matcher=matcher):
            w = wants[got]
            what = 'stream_json(%s, %s), window %d' % (parser, matcher, got)
            assert (info.n_frames, info.n_heads, info.n_edge_nodes) == (3, w['pb'].n_heads, w['pb'].n_edge_nodes), what
            assert np.array_equal(n_persons, w[kind][1]), what
            _same_rows((torch.from_numpy(poses), torch.from_numpy(w['mlp', kind][1])), w['mlp', kind], what)
            got += 1
        assert got == len(wants)
    engine.sync_status()


# ---- a seeded schedule ------------------------------------------------------------------------------------------------------
OPS = ('upload', 'match', 'geom_match', 'gat_cluster', 'mlp3d', 'triangulate', 'rows', 'fresh', 'precision', 'sync_status')
OP_WEIGHTS = (0.05, 0.15, 0.12, 0.08, 0.25, 0.08, 0.08, 0.09, 0.05, 0.05)
FRESH_SIZES = (1, 3, 16, 17)


def _schedule(seed, steps, n_batches):
    """[(op, arena, batch uploaded first or -1, draws)]: drawn before anything runs, so that a seed names the same calls everywhere.
    An 'upload' step only uploads; every other step on an arena may upload first and still ends in a compared output."""
    rng = np.random.default_rng(seed)
    out = []
    for _ in range(steps):
        op = OPS[int(rng.choice(len(OPS), p=OP_WEIGHTS))]
        up = int(rng.integers(n_batches)) if op == 'upload' or (op in OPS[1:7] and rng.random() < 0.45) else -1
        out.append((op, int(rng.integers(2)), up, (float(rng.random()), int(rng.integers(2)), int(rng.integers(len(FRESH_SIZES))))))
    return out


def test_a_seeded_schedule_of_calls_on_one_engine(calib, gat_weights, mlp_weights):
    """One long-lived engine, two arenas and freshly allocated batches of 1, 3, 16 and 17 frames; 90 steps drawn from: upload batch k
    into arena r, match, geom_match, gat_scores + cluster, mlp3d, triangulate, mlp_input_rows (on persons the arena's last matching
    call wrote, or on expected ones from the host), a fresh batch through match + mlp3d, set_precision on and back, sync_status.
    Every output is compared with the expected bits of whatever batch the arrays hold at that moment."""
    seed, steps = 20261020, 90
    eng = pkg('pipeline').Engine(calib.params, calib, max_frames=17, max_persons_per_camera=10)
    sd, prm = gat_weights
    eng.load_gat(sd, prm)
    eng.load_mlp(mlp_weights)
    try:
        with pytest.MonkeyPatch.context() as mp:
            mp.setenv('MPE_LATENCY_PATH', '0')
            wants = [_expect(eng, calib, _raw(calib, s)) for s in STARTS.values()]
            fresh = {n: _expect(eng, calib, _raw(calib, 500) if n == 3 else _mixed(calib, n, 2000 + 40 * n)) for n in FRESH_SIZES}
        plan = _schedule(seed, steps, len(wants))
        assert 10 * sum(op == 'upload' for op, _, _, _ in plan) <= steps and {op for op, _, _, _ in plan} == set(OPS)
        slots = [_Slot(eng, wants[0]['pb']) for _ in range(2)]
        for r in range(2):
            slots[r].load(wants[r])
        live = [None, None]                       # (persons, n_persons, kind) the last matching call on the arena wrote, while its batch stays
        compared = 0
        for step, (op, r, up, (u, bit, size)) in enumerate(plan):
            what = 'seed %d, step %d: %s in arena %d%s' % (seed, step, op, r, ' after uploading batch %d' % up if up >= 0 else '')
            slot = slots[r]
            if up >= 0:
                slot.load(wants[up])
                live[r] = None
            db, w = slot.db, slot.holds
            if op == 'match':
                _, p, n = eng.match(db, want_scores=bool(bit))
                _same_persons((p, n), w['gat'], what)
                live[r] = (p, n, 'gat')
            elif op == 'geom_match':
                _, p, n = eng.geom_match(db, want_scores=bool(bit))
                _same_persons((p, n), w['geo'], what)
                live[r] = (p, n, 'geo')
            elif op == 'gat_cluster':
                p, n = eng.cluster(db, eng.gat_scores(db))
                _same_persons((p, n), w['gat'], what)
                live[r] = (p, n, 'gat')
            elif op in ('mlp3d', 'triangulate', 'rows'):
                if live[r] is not None and u < 0.7:
                    p, n, kind = live[r]
                else:
                    kind = KINDS[bit]
                    p, n = _device_persons(eng, w, kind)
                call = {'mlp3d': eng.mlp3d, 'triangulate': eng.triangulate, 'rows': eng.mlp_input_rows}[op]
                _same_rows(call(db, p, n), w[{'mlp3d': 'mlp', 'triangulate': 'tri', 'rows': 'rows'}[op], kind], what + ' (%s persons)' % kind)
            elif op == 'fresh':
                fw = fresh[FRESH_SIZES[size]]
                fdb = eng.to_device(fw['pb'])
                _, p, n = eng.match(fdb, want_scores=bool(bit))
                _same_persons((p, n), fw['gat'], what + ', %d frames' % fdb.n_frames)
                _same_rows(eng.mlp3d(fdb, p, n), fw['mlp', 'gat'], what + ', %d frames: mlp3d' % fdb.n_frames)
            elif op == 'precision':
                eng.set_precision(mlp_max_accuracy=True)
                eng.set_precision()
            elif op == 'sync_status':
                eng.sync_status()
            compared += op not in ('upload', 'precision', 'sync_status')
        assert compared >= 60
        eng.sync_status()
    finally:
        eng.close()
