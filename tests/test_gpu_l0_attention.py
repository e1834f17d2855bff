"""Layer 0 of the matching network on the batch path: the coefficients of the head rows and the attention stage in ONE launch that
writes whole rows (csrc/gat.hip: k_l0_attention), against the small-batch route (chunks of at most sixteen frames run
k_lat_attention, which shares no kernel with it and computes layer 0's coefficients itself), against the general kernels
(MPE_NO_FUSED_ATTENTION=1: k_attn_coef + k_aggregate_*), and against every switch that keeps layer 0 on the coefficient kernel and
k_gat_fused: the same arithmetic in the same order, so the same bits."""
import json

import numpy as np
import pytest

from conftest import pkg

pytestmark = pytest.mark.gpu

SWITCHES = ['MPE_NO_FUSED_ATTENTION', 'MPE_NO_COEF_EPILOGUE', 'MPE_FUSED_NO_OVERLAP', 'MPE_NO_HEAD_SRC_TABLE']


def _engine(calib, gat_weights, mlp_weights, **kw):
    eng = pkg('pipeline').Engine(calib.params, calib, **kw)
    sd, prm = gat_weights
    eng.load_gat(sd, prm)
    eng.load_mlp(mlp_weights)
    return eng


@pytest.fixture(scope='module')
def engine(calib, gat_weights, mlp_weights):
    """5 x 4: at most 20 heads per frame -- the frames whose head rows and tables fit the new launch's LDS budget."""
    eng = _engine(calib, gat_weights, mlp_weights, max_frames=64, max_persons_per_camera=4)
    yield eng
    eng.close()


def _raw(calib, index, persons, cameras_left=None, joint_drop=0.0):
    syn = pkg('synthetic')
    cams = list(calib.params.used_cameras_skeleton_matching)
    empty = () if cameras_left is None else tuple(cams[cameras_left:])
    return syn.make_frame(calib, index, syn.FrameSpec(persons=persons, empty_cameras=empty, joint_drop=joint_drop))[0]


def _frame(calib, index, persons, cameras_left=None, joint_drop=0.0, missing=()):
    """A synthetic frame of `persons` persons; cameras_left: only the first so many cameras see anybody (0: an empty frame);
    missing: camera positions whose FIRST skeleton is taken out (a person some cameras do not see)."""
    from conftest import oracle
    frame = _raw(calib, index, persons, cameras_left, joint_drop)
    cams = list(calib.params.used_cameras_skeleton_matching)
    for c in missing:
        entry = frame[cams[c]]
        sk = json.loads(entry[0])
        entry[0] = json.dumps(sk[1:])
        entry[3] = entry[3][1:]
    return oracle().processed_input(frame)


@pytest.fixture(scope='module')
def mixed_frames(calib):
    """46 frames: 5 x 4 with and without dropped joints, frames of 1, 2 and 3 persons, a frame with nobody, a one-camera frame (heads,
    no edge-node) and frames with a person missing from two / three cameras (camera slots of different sizes)."""
    frames = []
    for i in range(36):
        frames.append(_frame(calib, 7100 + i, 4, joint_drop=0.15 if i % 3 == 1 else 0.0))
    extra = [_frame(calib, 7200, 1), _frame(calib, 7201, 2), _frame(calib, 7202, 3),
             _frame(calib, 7203, 3, cameras_left=0),                  # nobody anywhere
             _frame(calib, 7204, 2, cameras_left=1),                  # one camera: no graph
             _frame(calib, 7205, 4, missing=(1, 3)), _frame(calib, 7206, 3, missing=(0, 2, 4)),
             _frame(calib, 7207, 2, cameras_left=2), _frame(calib, 7208, 1, joint_drop=0.3), _frame(calib, 7209, 4, missing=(4,))]
    for k, fr in enumerate(extra):
        frames.insert(3 + 4 * k, fr)
    assert len(frames) == 46
    return frames


def _match(engine, frames):
    db = engine.to_device(engine.pack(frames))
    scores, persons, n_persons = engine.match(db, want_scores=True)
    engine.sync_status()
    counts = [db.host.frame_counts(f) for f in range(len(frames))]               # (first head, heads, first edge-node, edge-nodes)
    return scores.cpu().numpy(), persons.cpu().numpy(), n_persons.cpu().numpy(), counts


def _same_bits(a, b):
    return a.shape == b.shape and np.array_equal(a.view(np.int32), b.view(np.int32))


def _assert_chunks_equal_batch(engine, frames, big, chunk=16):
    """The frames again in chunks of at most `chunk` (the small-batch route): every frame's scores (bit for bit), persons and
    person count against `big`."""
    sc, pe, npers, counts = big
    seen = 0
    for i in range(0, len(frames), chunk):
        s2, p2, n2, c2 = _match(engine, frames[i:i + chunk])
        for j in range(len(c2)):
            _, _, e0, m = counts[i + j]
            _, _, f0, m2 = c2[j]
            assert m2 == m and _same_bits(s2[f0:f0 + m], sc[e0:e0 + m]), (i + j, m)
            cnt = int(npers[i + j])
            assert int(n2[j]) == cnt and np.array_equal(p2[j, :cnt], pe[i + j, :cnt]), i + j
            seen += 1
    assert seen == len(frames)


def _clear(monkeypatch):
    for name in SWITCHES + ['MPE_LATENCY_PATH']:
        monkeypatch.delenv(name, raising=False)


@pytest.fixture(scope='module')
def mixed_result(engine, mixed_frames):
    """The mixed batch on the new route, computed once; (result, launches of k_l0_attention it took)."""
    import os
    assert not any(os.environ.get(n) for n in SWITCHES)
    before = engine.l0_attention_launches()
    big = _match(engine, mixed_frames)
    return big, engine.l0_attention_launches() - before


def test_mixed_batch_against_the_small_batch_route(engine, mixed_frames, mixed_result, monkeypatch):
    """46 frames in one batch take the new launch once; the same frames in chunks of at most sixteen take k_lat_attention and do not."""
    _clear(monkeypatch)
    big, taken = mixed_result
    assert taken == 1
    heads = sorted({c[1] for c in big[3]})
    assert heads[0] == 0 and 20 in heads and len(heads) >= 6, heads
    assert any(c[1] > 0 and c[3] == 0 for c in big[3])                            # heads without a graph
    assert int(big[2].sum()) >= 36
    before = engine.l0_attention_launches()
    _assert_chunks_equal_batch(engine, mixed_frames, big)
    assert engine.l0_attention_launches() == before


@pytest.mark.parametrize('n', [17, 33])
def test_odd_frame_counts(engine, mixed_frames, n, monkeypatch):
    """17 and 33 frames: the grid of the launch is no multiple of the eight-way workgroup order, the last slab ragged."""
    _clear(monkeypatch)
    frames = mixed_frames[46 - n:]
    before = engine.l0_attention_launches()
    big = _match(engine, frames)
    assert engine.l0_attention_launches() == before + 1
    _assert_chunks_equal_batch(engine, frames, big)


@pytest.mark.parametrize('switch', SWITCHES)
def test_switches_keep_the_two_launches(engine, mixed_frames, mixed_result, switch, monkeypatch):
    """Each cross-check switch of the routing list keeps layer 0 on k_attn_coef + the kernels it names: the new launch is not taken
    (the context's counter stands still) and no bit of the result changes."""
    _clear(monkeypatch)
    monkeypatch.setenv(switch, '1')
    before = engine.l0_attention_launches()
    old = _match(engine, mixed_frames)
    assert engine.l0_attention_launches() == before
    big, _ = mixed_result
    assert _same_bits(old[0], big[0])
    assert np.array_equal(old[1], big[1]) and np.array_equal(old[2], big[2])


def test_precision_modes_keep_the_two_launches(engine, mixed_frames, monkeypatch):
    """fp16 feature rows in the attention stage (set_precision(attn_fp16=True)) are not what the new launch reads: not taken."""
    _clear(monkeypatch)
    try:
        engine.set_precision(attn_fp16=True)
        before = engine.l0_attention_launches()
        _match(engine, mixed_frames[:20])
        assert engine.l0_attention_launches() == before
    finally:
        engine.set_precision()


def test_layer0_activations_against_the_general_kernels(engine, mixed_frames, monkeypatch):
    """The rows layer 0 leaves for layer 1 (mpe_gat_layer with device-featurised rows) from the new launch and from k_attn_coef + the
    general kernels: every row of a frame with a graph has the same bits.  (Head rows of frames without a graph are left alone by
    the fused kernels and written by the general ones: not compared.)"""
    _clear(monkeypatch)
    db = engine.to_device(engine.pack(mixed_frames))
    before = engine.l0_attention_launches()
    new = engine.gat_layer(db, 0, None).cpu().numpy()
    assert engine.l0_attention_launches() == before + 1
    monkeypatch.setenv('MPE_NO_FUSED_ATTENTION', '1')
    old = engine.gat_layer(db, 0, None).cpu().numpy()
    assert engine.l0_attention_launches() == before + 1
    engine.sync_status()
    assert new.shape == old.shape == (db.n_heads + db.n_edge_nodes, 400)
    rows = 0
    for f in range(len(mixed_frames)):
        h0, H, e0, M = db.host.frame_counts(f)
        if M == 0:
            assert not new[h0 + e0:h0 + e0 + H].any()
            continue
        r0 = h0 + e0
        assert _same_bits(new[r0:r0 + H + M], old[r0:r0 + H + M]), f
        assert np.isfinite(new[r0:r0 + H + M]).all() and new[r0:r0 + H + M].any(axis=1).all(), f
        rows += H + M
    assert rows > 6000


def test_frame_beyond_capacity(calib, gat_weights, mlp_weights, monkeypatch):
    """One frame with more heads than max_heads_per_frame in a batch of eighteen (the batch path): k_topology raises the status flag,
    the frame's scores are zero and it has no persons, its neighbours are untouched -- on the new launch as on k_gat_fused."""
    _clear(monkeypatch)
    L = pkg('lib')
    small = _engine(calib, gat_weights, mlp_weights, max_frames=20, max_heads_per_frame=14)
    big = _engine(calib, gat_weights, mlp_weights, max_frames=20, max_persons_per_camera=4)
    try:
        frames = [_frame(calib, 7300 + i, 2, joint_drop=0.1 * (i % 2)) for i in range(18)]
        frames[11] = _frame(calib, 7311, 4)                                       # 20 heads > 14
        pb = big.pack(frames)
        want_s, want_p, want_n = big.match(big.to_device(pb))
        big.sync_status()
        db = pb.to(small.device)                                                  # (the C ABI alone: device-side detection)
        assert pb.n_heads <= small.max_frames * small.hpf
        results = []
        for switch in (None, 'MPE_FUSED_NO_OVERLAP'):
            if switch:
                monkeypatch.setenv(switch, '1')
            before = small.l0_attention_launches()
            s, p, n = small.match(db)
            with pytest.raises(L.MpeError) as ei:
                small.sync_status()
            assert ei.value.code == -2
            small.sync_status()                                                   # the sticky bit was cleared
            assert small.l0_attention_launches() - before == (0 if switch else 1)
            results.append((s.cpu().numpy(), p.cpu().numpy(), n.cpu().numpy()))
        (s, p, n), (s_old, p_old, n_old) = results
        assert _same_bits(s, s_old) and np.array_equal(n, n_old)
        e_off = pb.frame_en_off
        assert n[11] == 0 and not s[e_off[11]:e_off[12]].any()
        ws, wn, wp = want_s.cpu().numpy(), want_n.cpu().numpy(), want_p.cpu().numpy()
        for f in range(18):
            if f == 11:
                continue
            assert _same_bits(s[e_off[f]:e_off[f + 1]], ws[e_off[f]:e_off[f + 1]]), f
            assert n[f] == wn[f] and np.array_equal(p[f, :n[f]], wp[f, :n[f]]) and np.array_equal(p[f, :n[f]], p_old[f, :n[f]]), f
    finally:
        small.close()
        big.close()


def test_five_by_ten_falls_back(calib, gat_weights, mlp_weights, monkeypatch):
    """5 x 10 (up to 50 heads per frame: 80 KB of head rows, beyond the launch's 64 KB of LDS): twenty frames keep the coefficient
    kernel and k_gat_fused, and their scores are those of the small-batch route."""
    _clear(monkeypatch)
    eng = _engine(calib, gat_weights, mlp_weights, max_frames=20, max_persons_per_camera=10)
    try:
        frames = [_frame(calib, 7400 + i, 10, joint_drop=0.05 * (i % 3)) for i in range(20)]
        big = _match(eng, frames)
        assert eng.l0_attention_launches() == 0
        assert max(c[1] for c in big[3]) == 50
        _assert_chunks_equal_batch(eng, frames, big, chunk=10)
    finally:
        eng.close()
