"""mpe_geom_scores_batch / mpe_geom_match_batch (csrc/geom.hip, Engine.geom_scores / geom_match) against the host
statement harness/geometric.py, bit for bit; the matcher argument of the pipelines; --matcher geometric of the harness
scripts end to end.  No engine of this file has weights loaded."""
import importlib
import json
import os
import random

import numpy as np
import pytest

import geom_cases as gc
from conftest import env, generated_fixture, pkg

pytestmark = pytest.mark.gpu
HARNESS = '3d_multi_pose_estimator_amd.harness.'
_made = {}


class Setup:
    def __init__(self, name, **engine_kw):
        self.case = case = gc.case(name)
        kw = dict(max_frames=max(17, case.pb.n_frames), max_persons_per_camera=max(4, case.most))
        kw.update(engine_kw)
        self.eng = eng = pkg('pipeline').Engine(case.params, case.calib, **kw)
        assert eng.gat_dims is None and eng.mlp_out is None and not eng._state
        self.db = eng.to_device(case.pb)

    def device(self, **opts):
        sc, nv, mean = self.eng.geom_scores(self.db, details=True, **opts)
        return {'scores': sc.cpu().numpy(), 'n_votes': nv.cpu().numpy(), 'mean': mean.cpu().numpy()}


def setup(name):
    if name not in _made:
        _made[name] = Setup(name)
    return _made[name]


def teardown_module(module):
    for s in _made.values():
        s.eng.close()
    _made.clear()


def assert_same(got, want, what):
    for k in ('scores', 'n_votes', 'mean'):
        g, w = got[k], want[k]
        assert g.shape == w.shape and g.dtype == w.dtype, (what, k, g.shape, w.shape, g.dtype, w.dtype)
        if not gc.same_bits(g, w):
            bad = np.argwhere(g != w)
            print(what, k, 'differing', len(bad), 'of', g.size, 'first', bad[:3].ravel().tolist(), g[tuple(bad[0])], w[tuple(bad[0])])
        assert gc.same_bits(g, w), (what, k)


def rows(persons, n_persons, f):
    return persons[f, :int(n_persons[f])].tolist()


@pytest.mark.parametrize('name', gc.NAMES)
def test_bit_equal_to_host_statement(name):
    """1: scores, votes and means of every edge-node under the three option sets."""
    s = setup(name)
    for opts in gc.option_sets(s.case.params):
        got, want = s.device(**opts), s.case.statement(**opts)
        print(name, opts, 'edge-nodes', len(want['scores']), 'scored', int((want['scores'] > 0).sum()), 'above 0.5', int((want['scores'] > 0.5).sum()))
        assert_same(got, want, (name, opts))
    s.eng.sync_status()
    assert len(want['scores']) == s.case.pb.n_edge_nodes > 0


@pytest.mark.parametrize('name', gc.NAMES)
def test_match_is_scores_then_cluster(name):
    """2: geom_match = cluster(geom_scores) = the oracle's clustering of the statement's scores; want_scores=False (the
    context's own score buffer) gives the same persons."""
    s = setup(name)
    sc, persons, n_persons = s.eng.geom_match(s.db)
    p2, n2 = s.eng.cluster(s.db, s.eng.geom_scores(s.db))
    none, p3, n3 = s.eng.geom_match(s.db, want_scores=False)
    s.eng.sync_status()
    assert none is None and gc.same_bits(sc.cpu().numpy(), s.case.statement()['scores'])
    persons, n_persons = persons.cpu().numpy(), n_persons.cpu().numpy()
    want = gc.oracle_persons(s.case, s.case.statement()['scores'])
    for f in range(s.case.pb.n_frames):
        assert rows(persons, n_persons, f) == rows(p2.cpu().numpy(), n2.cpu().numpy(), f) == rows(p3.cpu().numpy(), n3.cpu().numpy(), f)
        assert rows(persons, n_persons, f) == [list(p) for p in want[f]], (name, f)
    if name in ('clean', 'noisy', '5x10'):
        for f in range(s.case.pb.n_frames):
            assert {frozenset(h for h in p if h >= 0) for p in rows(persons, n_persons, f)} == gc.true_partition(s.case, f)


def test_frames_apart_and_empty_batch():
    """4: the batch frame by frame gives the bits of the whole batch; a batch of no frames is accepted."""
    s = setup('messy')
    whole = s.device()
    _, persons, n_persons = s.eng.geom_match(s.db)
    persons, n_persons = persons.cpu().numpy(), n_persons.cpu().numpy()
    packing = pkg('packing')
    for f in range(s.case.pb.n_frames):
        pb = packing.pack_frames(s.case.processed[f:f + 1], s.case.params)
        db = s.eng.to_device(pb)
        sc, nv, mean = s.eng.geom_scores(db, details=True)
        e0, e1 = int(s.case.pb.frame_en_off[f]), int(s.case.pb.frame_en_off[f + 1])
        assert_same({'scores': sc.cpu().numpy(), 'n_votes': nv.cpu().numpy(), 'mean': mean.cpu().numpy()},
                    {k: whole[k][e0:e1] for k in whole}, ('frame', f))
        _, p1, n1 = s.eng.geom_match(db)
        assert rows(p1.cpu().numpy(), n1.cpu().numpy(), 0) == rows(persons, n_persons, f)
    empty = s.eng.to_device(packing.pack_frames([], s.case.params))
    sc, nv, mean = s.eng.geom_scores(empty, details=True)
    m_sc, p0, n0 = s.eng.geom_match(empty)
    s.eng.sync_status()
    assert sc.numel() == nv.numel() == mean.numel() == m_sc.numel() == 0 and tuple(p0.shape) == (0, s.eng.pcap, s.eng.V) and n0.numel() == 0


def test_ray_table_route_gives_the_lds_bits():
    """5: an engine whose max_heads_per_frame puts the rays of a frame beyond the LDS budget (120 heads x 18 joints x 24 B
    > 48 KiB) takes the ray table in context workspace: same bits as the LDS route and as the statement, same persons."""
    s = setup('5x10')
    big = Setup('5x10', max_frames=4, max_heads_per_frame=120)
    try:
        for opts in gc.option_sets(s.case.params):
            got = big.device(**opts)
            assert_same(got, s.device(**opts), ('table against LDS', opts))
            assert_same(got, s.case.statement(**opts), ('table against the statement', opts))
        _, p_big, n_big = big.eng.geom_match(big.db)
        _, p, n = s.eng.geom_match(s.db)
        big.eng.sync_status()
        for f in range(s.case.pb.n_frames):
            assert rows(p_big.cpu().numpy(), n_big.cpu().numpy(), f) == rows(p.cpu().numpy(), n.cpu().numpy(), f)
    finally:
        big.eng.close()


def test_ring23_rig_capacity_takes_the_ray_table_route():
    """The 23-camera rig at its own capacity of 230 heads a frame (230 x 18 x 24 B > 48 KiB): the ray table in context
    workspace gives the bits of the LDS route of the small engine and of the statement, 2277 edge-nodes a frame."""
    s = setup('ring23')
    assert s.eng.hpf * gc.J * 24 <= 48 * 1024
    big = Setup('ring23', max_frames=4, max_heads_per_frame=230)
    try:
        assert big.eng.hpf == 230 and big.eng.hpf * gc.J * 24 > 48 * 1024
        for opts in gc.option_sets(s.case.params):
            got = big.device(**opts)
            assert_same(got, s.device(**opts), ('table against LDS', opts))
            assert_same(got, s.case.statement(**opts), ('table against the statement', opts))
        big.eng.sync_status()
    finally:
        big.eng.close()


def test_frames_over_capacity_score_zero_and_are_reported():
    """Frames beyond max_heads_per_frame (the host check skipped): zeros, means -1, and the sticky status bit."""
    MpeError = pkg('lib').MpeError
    c = gc.case('clean')
    eng = pkg('pipeline').Engine(c.params, c.calib, max_frames=64, max_heads_per_frame=16)
    try:
        db = c.pb.to(eng.device)
        sc, nv, mean = eng.geom_scores(db, details=True)
        with pytest.raises(MpeError) as err:
            eng.sync_status()
        assert err.value.code == -2, str(err.value)
        assert not sc.cpu().numpy().any() and not nv.cpu().numpy().any() and np.all(mean.cpu().numpy() == -1.0)
    finally:
        eng.close()


def test_arguments():
    """What the entry points refuse, with a message."""
    MpeError = pkg('lib').MpeError
    s = setup('c1')
    for kw, word in (({'sigma': 0.0}, 'sigma_m'), ({'sigma': float('nan')}, 'sigma_m'), ({'clip': -1.0}, 'clip_m'), ({'min_joints': 0}, 'min_joints'),
                     ({'min_joints': gc.J + 1}, 'min_joints'), ({'min_conf': -0.1}, 'min_conf')):
        for call in (s.eng.geom_scores, s.eng.geom_match):
            with pytest.raises(MpeError) as err:
                call(s.db, **kw)
            assert err.value.code == -1 and word in str(err.value), str(err.value)
    import ctypes as C
    L = pkg('lib')
    a = L.mpe_geom_args()
    a.sigma_m, a.clip_m, a.min_joints = 0.1, 0.5, 1
    with pytest.raises(MpeError) as err:
        s.eng._chk(s.eng.lib.mpe_geom_scores_batch(s.eng.ctx, s.eng._stream(), C.byref(s.db.struct), C.byref(a)))
    assert err.value.code == -1 and 'NULL' in str(err.value)
    with pytest.raises(ValueError):
        list(s.eng.run_pipelined([s.db], mode='tri', matcher='nearest'))


def test_pipelines_with_the_geometric_matcher():
    """6: run_pipelined and stream_json (both parsers, one and two contexts) with matcher='geometric' over `clean` give the
    bits of geom_match + triangulate called one after the other."""
    s = setup('clean')
    opts = {'sigma': 0.08, 'min_joints': 2}
    _, persons, n_persons = s.eng.geom_match(s.db, **opts)
    poses = s.eng.triangulate(s.db, persons, n_persons)[0].cpu().numpy()
    persons, n_persons = persons.cpu().numpy(), n_persons.cpu().numpy()
    s.eng.sync_status()
    F = s.case.pb.n_frames
    assert n_persons.min() >= 1
    parts = [s.case.processed[0:8], s.case.processed[8:16], s.case.processed[16:17]]
    for contexts in (1, 2):
        f0 = 0
        for got_poses, got_n, got_persons, _ in s.eng.run_pipelined([s.eng.pack(p) for p in parts], mode='tri', contexts=contexts, matcher='geometric', geom=opts):
            k = got_n.shape[0]
            assert np.array_equal(got_n.cpu().numpy(), n_persons[f0:f0 + k]) and np.array_equal(got_persons.cpu().numpy(), persons[f0:f0 + k])
            for f in range(k):
                assert gc.same_bits(got_poses[f, :n_persons[f0 + f]].cpu().numpy(), poses[f0 + f, :n_persons[f0 + f]])
            f0 += k
        assert f0 == F
    text = json.dumps(s.case.frames).encode()
    for parser, contexts in (('device', 1), ('device', 2), ('host', 1)):
        f0 = 0
        for info, got_poses, got_n in s.eng.stream_json(text, chunk_frames=8, mode='tri', parser=parser, contexts=contexts, matcher='geometric', geom=opts):
            k = len(got_n)
            assert np.array_equal(got_n, n_persons[f0:f0 + k]), (parser, contexts, f0)
            for f in range(k):
                assert gc.same_bits(np.array(got_poses[f, :n_persons[f0 + f]]), poses[f0 + f, :n_persons[f0 + f]]), (parser, contexts, f0 + f)
            f0 += k
        assert f0 == F


def metric_lines(text):
    return [ln for ln in text.splitlines() if ln.startswith('AP, precise and recall') or ln.startswith('MEAN ERR')]


def test_harness_triangulation_without_a_models_directory(tmp_path, capsys):
    """7: metrics_from_triangulation --matcher geometric with an empty models directory prints the metric lines of the
    --teacher-scores run on the same frames, plus the line that states the matcher."""
    tri = importlib.import_module(HARNESS + 'metrics_from_triangulation')
    capsys.readouterr()
    teacher = tri.main(['--synthetic', '16', '--random-weights', '--teacher-scores', '--batch', '16'])
    want = metric_lines(capsys.readouterr().out)
    empty = tmp_path / 'models'
    empty.mkdir()
    got = tri.main(['--synthetic', '16', '--matcher', 'geometric', '--modelsdir', str(empty), '--batch', '16'])
    text = capsys.readouterr().out
    print(text)
    assert len(want) == 7 and metric_lines(text) == want
    assert got['ap'] == teacher['ap'] and got['mpjpe_mm'] == teacher['mpjpe_mm'] and got['n_data'] == teacher['n_data'] == 16
    assert len([ln for ln in text.splitlines() if ln.startswith('Matcher: geometric')]) == 1 and 'no model files' not in text
    assert got['matcher'] == {'name': 'geometric', 'sigma': 0.10, 'clip': 0.5, 'min_joints': 1, 'min_conf': 0.0}
    both = tri.main(['--synthetic', '16', '--matcher', 'geometric', '--teacher-scores', '--modelsdir', str(empty), '--batch', '16'])
    assert both['ap'] == teacher['ap'] and both['mpjpe_mm'] == teacher['mpjpe_mm']


def test_harness_sm_metrics_scores_one(tmp_path):
    """7: sm_metrics --synthetic 16 --matcher geometric groups every frame as the ground truth does."""
    m = importlib.import_module(HARNESS + 'sm_metrics')
    for extra in ([], ['--device-metrics']):
        out = m.main(['--synthetic', '16', '--matcher', 'geometric', '--modelsdir', str(tmp_path), '--batch', '16'] + extra)
        print(extra, {k: out[k] for k in ('rand score', 'homogeneity', 'completeness', 'v_measure')})
        assert out['rand score'] == pytest.approx(1.0, abs=1e-12) and out['v_measure'] == pytest.approx(1.0, abs=1e-12)


def test_harness_without_gt_on_explicit_lists(tmp_path, monkeypatch):
    """7: sm_metrics_without_gt --matcher geometric on the generated fixture (explicit edge-node lists): the proposals of
    every graph are the oracle's clustering of the statement's scores."""
    exp, _, files, probs = generated_fixture()
    monkeypatch.chdir(tmp_path)
    m = importlib.import_module(HARNESS + 'sm_metrics_without_gt')
    out = m.main(['--testfiles'] + files + ['--modelsdir', str(tmp_path), '--datastep', '1', '--batch', '5', '--seed', str(exp['seed']),
                                            '--matcher', 'geometric'])
    assert out['n_data'] == exp['n_graphs'] and out['matcher']['name'] == 'geometric'
    random.seed(exp['seed'])
    ds = pkg('graph_generator').MergedMultipleHumansDataset(files, probs, limit=1000, mode='test_generated', alt='3', raw_dir='.')
    e = env()
    G = pkg('harness.geometric')
    c = gc.Case.__new__(gc.Case)
    c.params = e.params
    linked = 0
    for i in range(len(ds)):
        c.pb = ds[i][0].packed
        assert c.pb.en_pair is not None and c.pb.n_frames == 1
        want = gc.oracle_persons(c, G.scores(e.calib, c.pb)['scores'])[0]
        assert out['per_graph'][i]['est'] == [list(p) for p in want], i
        linked += len(want)
    assert linked > 0
