"""The last GAT layer of the batch path (fc1 150 -> 150 + LeakyReLU and the one-wide fc2 in ONE launch, csrc/lat.hip: k_last_fused)
against the small-batch route, whose kernels it does not share: the same arithmetic in the same order, so the same bits -- with
workgroups that walk several row tiles, with a ragged last tile, with fewer rows than one tile, and with the switches and precision
modes that keep the layer on its two launches."""
import numpy as np
import pytest

from conftest import pkg

pytestmark = pytest.mark.gpu


@pytest.fixture(scope='module')
def engine(calib, gat_weights, mlp_weights):
    eng = pkg('pipeline').Engine(calib.params, calib, max_frames=64, max_persons_per_camera=10)
    sd, prm = gat_weights
    eng.load_gat(sd, prm)
    eng.load_mlp(mlp_weights)
    yield eng
    eng.close()


def _frame(calib, index, persons, cameras_left=None, joint_drop=0.0):
    """A synthetic frame of `persons` persons; cameras_left: only the first so many cameras see anybody (0: an empty frame)."""
    syn = pkg('synthetic')
    from conftest import oracle
    cams = list(calib.params.used_cameras_skeleton_matching)
    empty = () if cameras_left is None else tuple(cams[cameras_left:])
    return oracle().processed_input(syn.make_frame(calib, index, syn.FrameSpec(persons=persons, empty_cameras=empty, joint_drop=joint_drop))[0])


@pytest.fixture(scope='module')
def mixed_frames(calib):
    """48 frames of 5 x 4 with, between them, frames of 0, 1 and 2 persons and frames without a graph (one camera: heads, no edge-node)."""
    frames, k = [], 0
    for i in range(48):
        frames.append(_frame(calib, 9100 + i, 4, joint_drop=0.15 if i % 3 == 1 else 0.0))
        if i % 4 == 1:
            kind = k % 4
            k += 1
            if kind == 0:
                frames.append(_frame(calib, 9200 + i, 1))
            elif kind == 1:
                frames.append(_frame(calib, 9200 + i, 2))
            elif kind == 2:
                frames.append(_frame(calib, 9200 + i, 3, cameras_left=0))       # nobody anywhere
            else:
                frames.append(_frame(calib, 9200 + i, 2, cameras_left=1))       # one camera: no graph
    return frames


def _match(engine, frames):
    db = engine.to_device(engine.pack(frames))
    scores, persons, n_persons = engine.match(db, want_scores=True)
    engine.sync_status()
    counts = [db.host.frame_counts(f) for f in range(len(frames))]               # (first head, heads, first edge-node, edge-nodes)
    return scores.cpu().numpy(), persons.cpu().numpy(), n_persons.cpu().numpy(), counts, db.n_heads + db.n_edge_nodes


def _same_bits(a, b):
    return a.shape == b.shape and np.array_equal(a.view(np.int32), b.view(np.int32))


def _assert_chunks_equal_batch(engine, frames, big, chunk=16):
    """The frames again in chunks of at most `chunk`: every frame's scores (bit for bit), persons and person count against `big`."""
    sc, pe, npers, counts, _ = big
    seen = 0
    for i in range(0, len(frames), chunk):
        s2, p2, n2, c2, _ = _match(engine, frames[i:i + chunk])
        for j in range(len(c2)):
            _, _, e0, m = counts[i + j]
            _, _, f0, m2 = c2[j]
            assert m2 == m and _same_bits(s2[f0:f0 + m], sc[e0:e0 + m]), (i + j, m)
            cnt = int(npers[i + j])
            assert int(n2[j]) == cnt and np.array_equal(p2[j, :cnt], pe[i + j, :cnt]), i + j
            seen += 1
    assert seen == len(frames)


def test_workgroups_walk_several_row_tiles_and_the_last_tile_is_ragged(engine, mixed_frames, monkeypatch):
    """About 8 700 node rows in one batch: more 16-row tiles than twice the persistent grid, so every workgroup of k_last_fused takes two
    to three tiles (both LDS images, fc2 dealt to several waves, the fc2 behind the loop), and a row count that is no multiple of 16.
    Against the same frames in chunks of at most sixteen on the small-batch route (k_lat_gemm / k_lat_tail)."""
    monkeypatch.delenv('MPE_LATENCY_PATH', raising=False)
    big = _match(engine, mixed_frames)
    n_nodes = big[4]
    assert n_nodes > 2 * 16 * 256 and n_nodes % 16 != 0, n_nodes
    assert int(big[2].sum()) >= 48
    _assert_chunks_equal_batch(engine, mixed_frames, big)


@pytest.fixture(scope='module')
def edge_batches(calib):
    """(name, frames, node rows): fewer rows than a tile, 15 / 16 / 17 rows, and the largest batch the small-batch route takes."""
    pair = [_frame(calib, 9400, 1, cameras_left=2)]                               # one person in two cameras: 2 heads + 1 edge-node
    r15 = [_frame(calib, 9401, 1)]                                                # 5 heads + 10 edge-nodes
    r16 = r15 + [_frame(calib, 9402, 1, cameras_left=1)]                          # + 1 head without a graph
    r17 = r15 + [_frame(calib, 9403, 2, cameras_left=1)]                          # + 2 heads without a graph
    largest = [_frame(calib, 9410 + i, 10, joint_drop=0.05 * (i % 3)) for i in range(15)] + [_frame(calib, 9430, 7)]
    return [('pair', pair, 3), ('15', r15, 15), ('16', r16, 16), ('17', r17, 17), ('largest', largest, None)]


def test_tile_edges_on_either_route(engine, edge_batches, monkeypatch):
    """Small batches through the batch path (MPE_LATENCY_PATH=0: k_last_fused with one partial tile, exactly one tile, one tile and one
    row, and 1019 tiles with the general attention path behind it) and through the small-batch route: the same bits."""
    for name, frames, rows in edge_batches:
        monkeypatch.setenv('MPE_LATENCY_PATH', '0')
        off = _match(engine, frames)
        monkeypatch.delenv('MPE_LATENCY_PATH', raising=False)
        lat = _match(engine, frames)
        assert off[4] == lat[4] and (off[4] == rows if rows else 15 * 1050 < off[4] <= 16384), (name, off[4])
        assert len(frames) <= 16                                                  # (<= 16 frames, <= 16384 rows: what the small-batch route takes)
        assert _same_bits(off[0], lat[0]), name
        assert np.array_equal(off[1], lat[1]) and np.array_equal(off[2], lat[2]), name


@pytest.mark.parametrize('setting', ['skinny_waves_0', 'gat_acc64'])
def test_switches_and_other_precisions_keep_the_two_launches(engine, mixed_frames, setting, monkeypatch):
    """MPE_SKINNY_WAVES (a cross-check switch of the batch path; the routing reads it per call) and f64 sums in the GAT keep the last
    layer on fc1 + fc2 as two launches, for the large batch and for its chunks alike (neither takes the small-batch route then):
    a frame's bits do not depend on the batch it travels in."""
    monkeypatch.delenv('MPE_LATENCY_PATH', raising=False)
    _match(engine, mixed_frames[:2])                                              # (the kernels' own switches are read once per process: before the change)
    try:
        if setting == 'skinny_waves_0':
            monkeypatch.setenv('MPE_SKINNY_WAVES', '0')
        else:
            engine.set_precision(True, True)
        big = _match(engine, mixed_frames)
        _assert_chunks_equal_batch(engine, mixed_frames, big)
    finally:
        engine.set_precision()
